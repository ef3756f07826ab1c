"""The rule of the rescued mates in assigned coverage over fragments (tests/calls_rescued_pairs_def.py) on the CPU: hand-worked cases with
the tuples written out, the three consequences of the rule against the definitions it joins (acov_pairs_def.paired_table_of_alns,
rescue_calls_def.table_of), and the floors of the batch tests/test_calls_rescued_paired.py feeds the device: test_rescue_pairs._CaseA's
fragments, imported and not copied.  Every expectation comes from the CPU oracle's records and the brute forces, never from device output."""
import numpy as np
import pytest

from acov_pairs_def import paired_table_of_alns
from calls_rescued_pairs_def import STATS, expect, rows_by_read, unit_sets
from groot_amd import device
from rescue_calls_def import exact_rows, rescued_records, table_of
from rescue_sets_def import rescued_sets
from test_calls import merge_tables
from test_rescue_pairs import _Frags, case_a, case_b      # noqa: F401  (fixtures)

FLOOR = 20
GPO1 = [0, 10]             # one graph of ten paths


def _rec(*rows):
    return np.array(rows, dtype=np.int64).reshape(-1, 4)


def _tab(w):
    return w.table.ecs, w.table.rows.tolist(), w.table.n.tolist()


# ---- hand-worked ------------------------------------------------------------------------------------------------------------------

def test_exact_mate_and_rescued_mate_share_one_path():
    """an exact mate on {p, q} = {1, 2}, a rescued mate on {q, s} = {2, 3}: the unit is {q}; the record on p and the placement on s are left out"""
    ex_rows = [(0, 1, 5, 40), (0, 2, 7, 42)]
    records = {1: _rec((2, 10, 45, 0), (3, 11, 46, 1))}
    w = expect(GPO1, {0: (1, 2)}, {1: (2, 3)}, ex_rows, records, 2)
    assert _tab(w) == ([((2,), 1)], [[0, 2, 7, 42], [0, 2, 10, 45]], [1, 1])
    assert w.unit == {0: (2,), 1: (2,)}
    assert w.stats == dict(exact_records=1, exact_left_out=1, rescued_records=1, rescued_left_out=1, host_records=0) and w.log == 0 and w.ee_left == 0
    # the mates the other way round: the same table
    sw = expect(GPO1, {1: (1, 2)}, {0: (2, 3)}, [(1, 1, 5, 40), (1, 2, 7, 42)], {0: records[1]}, 2)
    assert _tab(sw) == _tab(w) and sw.stats == w.stats


def test_two_rescued_mates_joined_one_with_two_placements_on_one_path():
    """R = {4, 5} with two placements on 4 (both strands of a repeat, two x) and R = {4}: unit {4}; every placement on 4 counts once, the
    one on 5 is left out; the two mates' placements at the same place fall into one tuple"""
    records = {0: _rec((4, 3, 38, 0), (4, 20, 55, 1), (5, 3, 38, 0)), 1: _rec((4, 20, 55, 0))}
    w = expect(GPO1, {}, {0: (4, 5), 1: (4,)}, [], records, 2)
    assert _tab(w) == ([((4,), 1)], [[0, 4, 3, 38], [0, 4, 20, 55]], [1, 2])
    assert w.stats == dict(exact_records=0, exact_left_out=0, rescued_records=3, rescued_left_out=1, host_records=0)


def test_split_fragment():
    """disjoint sets: two units, every record and placement counts under its own mate's set"""
    w = expect(GPO1, {0: (1,)}, {1: (6, 7)}, [(0, 1, 0, 36)], {1: _rec((6, 2, 37, 1), (7, 2, 37, 1))}, 2)
    assert _tab(w) == ([((1,), 1), ((6, 7), 1)], [[0, 1, 0, 36], [1, 6, 2, 37], [1, 7, 2, 37]], [1, 1, 1])
    assert w.stats == dict(exact_records=0, exact_left_out=0, rescued_records=2, rescued_left_out=0, host_records=0)      # (the exact record is the ordinary count's)
    assert w.units.cls == dict(joined=0, split=1, single=0, none=0)


def test_rescued_mate_beside_an_n_mate():
    """the partner has a non-ACGT base: the empty set and no record; the rescued mate is a single unit"""
    w = expect(GPO1, {}, {0: (8,)}, [], {0: _rec((8, 1, 36, 0))}, 2)
    assert _tab(w) == ([((8,), 1)], [[0, 8, 1, 36]], [1])
    assert w.units.cls == dict(joined=0, split=0, single=1, none=0) and w.stats["rescued_records"] == 1


def test_a_fragment_on_bitmaps_goes_through_the_log():
    """max_segs = 1 and an exact mate in two graphs: every record of the fragment, counting or not, is a log entry and folded on the host"""
    w = expect([0, 5, 10], {0: (1, 6)}, {1: (6, 7)}, [(0, 1, 5, 40), (0, 6, 7, 42)], {1: _rec((6, 9, 44, 0), (7, 9, 44, 0))}, 2, max_segs=1)
    assert _tab(w) == ([((6,), 1)], [[0, 6, 7, 42], [0, 6, 9, 44]], [1, 1])
    assert w.stats == dict(exact_records=1, exact_left_out=1, rescued_records=1, rescued_left_out=1, host_records=2) and w.log == 4


# ---- the batch of the device test --------------------------------------------------------------------------------------------------

class CallsFrags:
    """a test_rescue_pairs._Frags and what the definition needs beside its sets: the exact rows and the rescued reads' kept placements"""

    def __init__(self, frags):
        self.f, self.index, self.n, self.batch, self.reads, self.gpo = frags, frags.index, frags.n, frags.batch, frags.reads, frags.gpo
        self._rows, self._by_read, self._rec, self._full, self._want = None, None, {}, {}, {}

    def exact(self):
        return self.f.exact()

    def rescued(self, M):
        return self.f.rescued(M)

    def alns(self):
        return self.batch.want(self.index).alns.astype(device.ALN_DTYPE)

    def ex_rows(self):
        if self._rows is None:
            self._rows = exact_rows(self.index, self.alns(), self.batch.off)
        return self._rows

    def _by_seq(self, M, fn):
        ex = self.exact()
        self.f.rescued(M)                                           # (builds the tables once)
        uniq = sorted({r for i, r in enumerate(self.reads) if i not in ex})
        return uniq, fn(self.index, M, uniq, np.zeros(len(uniq), dtype=bool), self.f._tables)

    def records(self, M):
        """{read: rows (path, X, last, strand)}: the brute force once per distinct sequence"""
        if M not in self._rec:
            uniq, rec = self._by_seq(M, rescued_records)
            by = {uniq[i]: v for i, v in rec.items()}
            ex = self.exact()
            self._rec[M] = {i: by[r] for i, r in enumerate(self.reads) if i not in ex and r in by}
        return self._rec[M]

    def rescued_full(self, M):
        """{read: rescue_sets_def.Rescued}, for rescue_calls_def.table_of"""
        if M not in self._full:
            uniq, (res, _) = self._by_seq(M, rescued_sets)
            by = {uniq[i]: v for i, v in res.items()}
            ex = self.exact()
            self._full[M] = {i: by[r] for i, r in enumerate(self.reads) if i not in ex and r in by}
        return self._full[M]

    def want(self, M=1, max_segs=4, frags=None, on=True):
        key = (M, max_segs, None if frags is None else tuple(frags), on)
        if key not in self._want:
            if self._by_read is None:
                self._by_read = rows_by_read(self.ex_rows())
            self._want[key] = expect(self.gpo, self.exact(), self.rescued(M) if on else {}, self._by_read, self.records(M) if on else {}, self.n, max_segs, frags)
        return self._want[key]


@pytest.fixture(scope="module")
def calls_a(case_a):
    return CallsFrags(case_a.frags)


@pytest.fixture(scope="module")
def calls_b(case_b):
    return CallsFrags(case_b)


def test_inputs_hold_every_kind_of_record(case_a, calls_a, calls_b):
    c = calls_a
    w = c.want(1)
    ex, res, rec, rows = c.exact(), c.rescued(1), c.records(1), c.ex_rows()
    print(c.n, "mates", w.kinds, w.stats, "log", w.log, "tuples", len(w.table.n), "records", int(w.table.n.sum()))
    assert 1300 <= c.n <= 1600
    # every "ER subset" fragment: the sets overlap and neither holds the other, so the exact mate has a record outside the unit, and the
    # rescued mate a kept placement outside it
    sub = case_a.of_class("ER subset")
    assert len(sub) == 44
    for f in sub:
        e, r = (2 * f, 2 * f + 1) if 2 * f in ex else (2 * f + 1, 2 * f)
        u = set(w.unit[e])
        assert w.unit[e] == w.unit[r] and e in ex and r in res
        assert sum(1 for x in rows[rows[:, 0] == e].tolist() if x[1] not in u) >= 1 and sum(1 for x in rec[r].tolist() if x[0] not in u) >= 1
    assert w.stats["exact_left_out"] >= 44 and w.stats["rescued_left_out"] >= 44
    for kind in ("exact beside rescued", "placements, exact + rescued joined", "placements, rescued + rescued joined", "split fragments", "single fragments",
                 "bitmap records"):
        assert w.kinds.get(kind, 0) >= FLOOR, (kind, w.kinds)
    assert w.ee_left >= FLOOR                                         # the exact + exact fragments leave records out too: the ordinary count's rule
    assert int(w.table.n.sum()) == len(rows) + sum(len(v) for v in rec.values()) - w.ee_left - w.stats["exact_left_out"] - w.stats["rescued_left_out"]
    slow = c.want(1, max_segs=1)
    assert slow.log >= 10 * FLOOR and slow.stats["host_records"] > w.stats["host_records"] >= FLOOR and _tab(slow) == _tab(w)
    for M in (2, 3):
        assert c.want(M).stats["rescued_records"] >= 10 * FLOOR and _tab(c.want(M)) != _tab(w)      # (another M: other mates rescued, other tables)
    # case (b): the unit {T1:(a,d)} of a mate on {0, 2} and a rescued mate on {1, 2} leaves T0 without a path
    wb = calls_b.want(1)
    assert wb.stats["exact_left_out"] >= FLOOR and wb.stats["rescued_left_out"] >= FLOOR and wb.stats["exact_records"] >= FLOOR


def test_no_rescued_mate_is_the_table_over_fragments(calls_a):
    """consequence 1: without a rescued mate the table and the ECs are those of --calls --callsPaired"""
    c = calls_a
    w = c.want(1, on=False)
    t, left = paired_table_of_alns(c.index, c.alns(), c.batch.off)
    assert _tab(w) == (t.ecs, t.rows.tolist(), t.n.tolist()) and w.ee_left == left
    # (what is left of the one-pass kinds: the lone exact mates in more than four graphs, which take a bitmap and lose nothing)
    assert w.stats["rescued_records"] == w.stats["rescued_left_out"] == w.stats["exact_left_out"] == 0 and w.log == w.stats["host_records"] == w.stats["exact_records"]


def test_split_and_single_fragments_are_the_unpaired_run(calls_a):
    """consequence 2: over fragments that are split or single the table and the ECs are those of the unpaired --calls --callsRescued run"""
    c = calls_a
    w_all = c.want(1)
    ex = c.exact()
    _, cls = unit_sets(ex, c.rescued(1), c.n)
    frags = [f for f in range(c.n // 2) if cls[f] in ("split", "single", "none")]
    assert len(frags) >= 10 * FLOOR and len(frags) < c.n // 2
    w = c.want(1, frags=frags)
    reads = [r for f in frags for r in (2 * f, 2 * f + 1)]
    t = table_of(ex, c.ex_rows(), c.rescued_full(1), c.records(1), reads)
    assert _tab(w) == (t.ecs, t.rows.tolist(), t.n.tolist())
    assert w.stats["exact_left_out"] == w.stats["rescued_left_out"] == w.ee_left == 0 and w_all.stats["rescued_left_out"] > 0


def test_doubled_reads_double_the_unpaired_table(calls_a):
    """consequence 3: fragments (r, r) give the ECs of the unpaired --callsRescued run with every n doubled"""
    c = calls_a
    k = 600
    dbl = CallsFrags(_Frags(c.index, "doubled", [r for r in c.reads[:k] for _ in (0, 1)], c.f._tables))
    w = dbl.want(1)
    t = table_of(c.exact(), c.ex_rows(), c.rescued_full(1), c.records(1), range(k))
    assert w.table.ecs == t.ecs and w.table.rows.tolist() == t.rows.tolist() and w.table.n.tolist() == (2 * t.n).tolist()
    assert w.units.cls["split"] == w.units.cls["single"] == 0 and w.stats["exact_left_out"] == w.stats["rescued_left_out"] == 0


def test_pieces_sum_to_the_batch(calls_a):
    """the table is a sum over fragments: the definition over two halves merges to the definition over the batch"""
    c = calls_a
    nf = c.n // 2
    a, b = c.want(1, frags=range(0, 300)), c.want(1, frags=range(300, nf))
    m = merge_tables([a.table, b.table])
    assert (m.ecs, m.rows.tolist(), m.n.tolist()) == _tab(c.want(1))
    assert {k: a.stats[k] + b.stats[k] for k in STATS} == c.want(1).stats
