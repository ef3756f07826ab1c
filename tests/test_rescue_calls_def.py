"""The brute force of the rescued reads in assigned coverage (tests/rescue_calls_def.py) on hand-worked cases, and the floor of every input
class of the batch that tests/test_rescue_calls.py feeds the device: the nine graphs and the batch of test_rescue_ec.py plus, where that
batch misses a floor, reads added here.  CPU only."""
import numpy as np
import pytest

from rescue_calls_def import exact_rows, rescued_records, table_of
from rescue_def import Tables, _rc, path_texts
from rescue_sets_def import Rescued, rescued_sets
from test_counter_edges import _of_reads
from test_rescue import _has_record, _mut, _reads_of
from test_rescue_ec import FLOOR, _Case


class CallsCase(_Case):
    """test_rescue_ec's case, with reads added for the classes of the pileup, and per M the definition's table"""

    def __init__(self, tmp):
        super().__init__(tmp)
        texts = path_texts(self.index)
        rng = np.random.default_rng(19)
        more = []
        plen = self.index.arrays["path_len"].astype(np.int64)
        for k in range(60):           # the first / the last 48 bases inside path_len of a path of graph 0 .. 6, one substitution in the middle
            p = int(rng.choice([0, 70, 134, 199, 329, 457]))
            t, first = texts[p]
            n = min(len(t), int(plen[p]) - first)
            r = _mut(rng, t[:48] if k & 1 else t[n - 48:n], [20 + int(rng.integers(8))])
            more.append(("end%d" % (k & 1), _rc(r) if k & 2 else r))
        for k in range(60):           # 48 bases from anywhere on a path of the seven graphs: sets of paths that no read with a record has
            p = int(rng.integers(0, len(texts) - 3))
            t, first = texts[p]
            x = int(rng.integers(0, min(len(t), int(plen[p]) - first) - 48))
            r = _mut(rng, t[x:x + 48], [20 + int(rng.integers(8))])
            more.append(("anywhere", _rc(r) if k & 1 else r))
        self.names = self.names + [n for n, _ in more]
        self.batch = _of_reads("classes and ends", self.reads + [r for _, r in more])
        self.reads = _reads_of(self.batch)
        self._rec, self._rows = {}, None

    def records(self, M):
        if M not in self._rec:
            self._rec[M] = rescued_records(self.index, M, self.reads, _has_record(self.batch, self.index), self._tables)
        return self._rec[M]

    def rows(self):
        if self._rows is None:
            self._rows = exact_rows(self.index, self.batch.want(self.index).alns, self.batch.off)
        return self._rows

    def table(self, M, reads=None, on=True):
        """the definition's table over `reads` of the batch; on=False: the exact records and their classes alone"""
        return table_of(self.exact(), self.rows(), self.rescued(M)[0] if on else {}, self.records(M) if on else {}, reads)

    def n_records(self, M, reads=None, max_segs=4):
        """(rescued records, those of reads whose set lies in more than max_segs graphs) over `reads`"""
        res, rec = self.rescued(M)[0], self.records(M)
        reads = range(self.batch.n) if reads is None else reads
        mine = [i for i in reads if i in rec]
        return sum(len(rec[i]) for i in mine), sum(len(rec[i]) for i in mine if self.graphs_of(res[i].paths) > max_segs)


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return CallsCase(tmp_path_factory.mktemp("rescue_calls"))


# ---- hand-worked --------------------------------------------------------------------------------------------------------------------------

def _hand(case, texts, lens, reads, M=1):
    t = Tables(case.index, M)
    t.texts = texts + [None] * (len(t.texts) - len(texts))
    t.plen = np.array(lens + [0] * (len(t.plen) - len(lens)), dtype=np.int64)
    t.base = np.r_[0, np.cumsum(t.plen)]
    has = np.zeros(len(reads), dtype=bool)
    res, _ = rescued_sets(case.index, M, reads, has, t)
    return res, rescued_records(case.index, M, reads, has, t)


def test_two_placements_on_one_path(case):
    """path 0 = U . R . V . R with the 32 bases of R twice, first Position 3: R with one substitution lies at both copies -- two records
    of one read on one path, a tuple each; a read across U and R lies once, exactly"""
    u, r, v = b"ACGTTGCAAGGCTTAACCGG", b"ATCAGGTTACAGTCATGCAACCGTAGGTCTAA", b"TTGACCGTAAGC"
    text = u + r + v + r                                         # R at 20 and at 64; 96 bases
    assert r[9:10] == b"C"
    res, rec = _hand(case, [(text, 3)], [99], [r[:9] + b"G" + r[10:], u[4:20] + r[:16]])
    assert res[0] == Rescued(1, (0,), frozenset({0}), 2, True)
    assert rec[0].tolist() == [[0, 23, 54, 0], [0, 67, 98, 0]]   # X = 3 + 20 and 3 + 64, last = X + 31
    assert rec[1].tolist() == [[0, 7, 38, 0]] and res[1].d == 0  # 32 bases from text offset 4
    tab = table_of({}, np.zeros((0, 4), dtype=np.int64), res, rec)
    assert tab.ecs == [((0,), 2)]
    assert tab.rows.tolist() == [[0, 0, 7, 38], [0, 0, 23, 54], [0, 0, 67, 98]] and tab.n.tolist() == [1, 1, 1]


def test_both_strands_of_one_path_and_a_shared_tuple(case):
    """a 32-base reverse-complement palindrome P inside path 0: P with one substitution is at distance 1 on strand 0 and -- the substitution
    mirrored -- on strand 1, at the same X: two records, ONE tuple with n = 2.  Two more reads the same, one of them reverse-complemented:
    n = 6.  Path 1 holds P with another base changed: distance 2, above d*, not kept.  An exact record of the EC {0} on path 0 is a tuple
    of the same (EC, path)."""
    half = b"ACGTTGCAAGGCTTAC"
    pal = half + _rc(half)
    assert _rc(pal) == pal and pal[3:4] == b"T" and pal[5:6] == b"G"
    t0, t1 = b"GGATCCTTAGGCAT" + pal + b"TTGACCGTAAGCAA", b"CATTAG" + pal[:3] + b"A" + pal[4:] + b"GGA"
    read = pal[:5] + b"A" + pal[6:]
    res, rec = _hand(case, [(t0, 0), (t1, 2)], [60, 43], [read, read, _rc(read)])
    for i in range(3):
        assert res[i] == Rescued(1, (0,), frozenset({0, 1}), 2, False)
        assert sorted(rec[i].tolist()) == [[0, 14, 45, 0], [0, 14, 45, 1]]
    ex = np.array([[3, 0, 10, 39]])                              # read 3: an exact record on path 0, S(r) = {0}
    tab = table_of({3: (0,)}, ex, res, rec)
    assert tab.ecs == [((0,), 4)]
    assert tab.rows.tolist() == [[0, 0, 10, 39], [0, 0, 14, 45]] and tab.n.tolist() == [1, 6]


def test_a_read_on_two_paths_and_at_either_end(case):
    """two paths that share their first 32 bases: a read over them with one substitution has one record on each, at X = the path's first
    Position, under the EC {0, 1}; the last window of path 1 ends at path_len - 1"""
    head = b"ACGTTGCAAGGCTTAACCGGATCAGTCATGCA"
    t0, t1 = head + b"GGTTACAGTC", head + b"TTGACCGTAAGCAATGCCTAGGATTC"
    assert head[11:12] == b"C" and t1[-3:-2] == b"T" and len(t1) == 58
    res, rec = _hand(case, [(t0, 0), (t1, 5)], [42, 63], [head[:11] + b"A" + head[12:], t1[-32:-3] + b"C" + t1[-2:]])
    assert res[0].paths == (0, 1) and rec[0].tolist() == [[0, 0, 31, 0], [1, 5, 36, 0]]
    assert res[1].paths == (1,) and rec[1].tolist() == [[1, 31, 62, 0]]
    tab = table_of({}, np.zeros((0, 4), dtype=np.int64), res, rec)
    assert tab.ecs == [((0, 1), 1), ((1,), 1)]
    assert tab.rows.tolist() == [[0, 0, 0, 31], [0, 1, 5, 36], [1, 1, 31, 62]] and tab.n.tolist() == [1, 1, 1]


# ---- the batch of the device tests --------------------------------------------------------------------------------------------------------

def classes(case, M=1):
    res, rec = case.rescued(M)[0], case.records(M)
    ex, rows = case.exact(), case.rows()
    texts = path_texts(case.index)
    plen = case.index.arrays["path_len"].astype(np.int64)
    tab = case.table(M)
    ecs = [ids for ids, _ in tab.ecs]
    index = {ids: i for i, ids in enumerate(ecs)}
    by_tuple = {}
    for i, r in rec.items():
        for p, x, last in set(map(tuple, r[:, :3].tolist())):
            by_tuple.setdefault((res[i].paths, p, x, last), set()).add(i)
    ex_ep = set((index[ex[int(r)]], int(p)) for r, p in rows[:, :2].tolist())
    res_ep = set((index[res[i].paths], int(p)) for i, r in rec.items() for p in np.unique(r[:, 0]))

    def two_x(r):
        px = np.unique(r[:, 0] * (1 << 32) + r[:, 1])
        return (np.bincount(np.unique(px >> 32, return_inverse=True)[1].reshape(-1)) > 1).any()

    def both_strands(r):
        return len(set((r[r[:, 3] == 0][:, 0]).tolist()) & set((r[r[:, 3] == 1][:, 0]).tolist())) > 0

    exact_sets = set(ex.values())
    return {"two_x_on_a_path": sum(bool(two_x(r)) for r in rec.values()),
            "both_strands_of_a_path": sum(both_strands(r) for r in rec.values()),
            "shared_tuples": sum(len(v) >= 2 for v in by_tuple.values()),
            "exact_and_rescued_on_an_ec_path": len(ex_ep & res_ep),
            "at_the_start": sum(bool((r[:, 1] == np.array([texts[p][1] for p in r[:, 0]])).any()) for r in rec.values()),
            "at_the_end": sum(bool((r[:, 2] == plen[r[:, 0]] - 1).any()) for r in rec.values()),
            "slow_when_forced": sum(case.graphs_of(r.paths) > 1 for r in res.values()),
            "slow": sum(case.graphs_of(r.paths) > 4 for r in res.values()),
            "rescued_only_ecs": len(set(r.paths for r in res.values()) - exact_sets)}


def test_inputs_hold_every_class(case):
    c = classes(case)
    print(c, "records", case.n_records(1), "tuples", len(case.table(1).n), "of them exact", len(case.table(1, on=False).n))
    assert all(v >= FLOOR for v in c.values()), c
    tab = case.table(1)
    assert int(tab.n.sum()) == len(case.rows()) + case.n_records(1)[0]
    assert [ids for ids, _ in tab.ecs] == sorted(case.expect(1)[0]) and dict(tab.ecs) == case.expect(1)[0]
    for M in (2, 3):
        n, slow = case.n_records(M)
        assert n >= 10 * FLOOR and len(case.table(M).n) > len(case.table(M, on=False).n)
