"""The index and the reads of tests/test_rescue_ec_shapes.py and tests/test_rescue_calls_shapes.py: the rescued reads in the equivalence
classes (kernels_rescue_ec.hpp) and in assigned coverage (kernels_rescue_acov.hpp) at the shapes tests/test_rescue_ec.py and
tests/test_rescue_calls_def.py do not reach.  CPU only.

Five graphs, eleven paths, path_words == 1.  The first four graphs, their seeds and the first reads of the batch are those of
tests/test_rescue_shapes.py (r0, r1 | gap, full | main, p11, p46 | l0, l1: tandem repeats of period 1, 3, 16 and 20, a text-less path, paths
of 11 and 46 bases, reads of up to 512 bases).  The fifth graph is the first once more under the path names r0b, r1b: every read in the
repeats has its set in two graphs, which GROOT_TEST_SHARED_SLOW (at most one graph per row) sends through the bitmaps and the placement
log.  Behind that batch come the reads it lacks for the classes of the pileup:

    many      48 bases of the A x 72 run with one or two substitutions, both strands: 25 kept placements on each of r0, r1, r0b, r1b, and
              every such read has the SAME 100 tuples (one new key claimed by many threads at once, one slot added to by all of them);
    textless  error-free reads of the nodes that `gap` and `full` share, and of the node that `gap` holds alone: S(r) = {gap, full} and
              {gap} come from the oracle's records, while a rescued read next to them has R(r) = {full} at most;
    full      error-free reads through the nodes of `full` alone, so that the EC {full} carries exact and rescued records on one path.

The expectation comes from rescue_sets_def.rescued_sets / ecs_plus, rescue_calls_def.rescued_records / exact_rows / table_of and the
oracle's records (test_rescue._has_record) only: every window of every text against every oriented read, no anchors, no tables.

Not covered: a path whose first node's Position is not 0 (a.path[p].z != 0 in rescue_acov_x).  A Position is the running length over the
path's own nodes, so every path a GFA file gives starts at 0 (tests/gap_shapes_case.py); the hand-worked cases of
tests/test_rescue_calls_def.py keep the definition's X = first Position + offset, and no index arrays are faked here."""
import numpy as np

from groot_amd import host
from rescue_def import A, Tables, _rc, path_texts
from test_counter_edges import _of_reads
from test_rescue import _has_record, _mut, _reads_of
from test_rescue_calls_def import CallsCase
from test_rescue_shapes import LONG, SHIFTED, _long_graph, _make_reads, _no_text_graph, _repeat_graph, _short_graph

PATHS = ("r0", "r1", "gap", "full", "main", "p11", "p46", "l0", "l1", "r0b", "r1b")
MANY = 16           # kept placements of one read on one path from which the claims of one key are called contended


class Sets(CallsCase):
    """CallsCase's expectations (the definition's ECs, records, table and stats, cached per M) over any batch of one index"""

    def __init__(self, index, batch, names=None, tables=None):
        self.index, self.batch, self.names = index, batch, names
        self.reads = _reads_of(batch)
        self.gpo = index.arrays["graph_path_off"].astype(np.int64)
        self._by_m, self._tables = {}, tables or Tables(index, 1)      # (the windows of the texts, shared by every M and every batch)
        self._rec, self._rows = {}, None

    def of(self, batch):
        """the same over another batch of this index"""
        return Sets(self.index, batch, tables=self._tables)

    def n_tuples(self, M):
        return len(self.table(M).n)


def _more_reads(rng, index, T, spans, gap, gap_at):
    """-> [(class name, read)] behind the batch of test_rescue_shapes"""
    out = []

    def put(name, r):
        out.append((name, _rc(r) if len(out) & 1 else r))

    (sa, ea, _), = [x for x in spans["homopolymer"] if x[1] - x[0] == 72]
    assert T["r0"][sa:ea] == b"A" * 72
    for k in range(40):                                          # the substitution anywhere, the first and the last base among them
        at = [(0, 47)[k & 1]] if k < 4 else rng.choice(48, 1 + (k % 4 == 3), replace=False)
        put("many", _mut(rng, T["r0"][sa:sa + 48], at))
    for k in range(12):                                          # M = 1: the path of 46 bases filled exactly
        put("fit46", _mut(rng, T["p46"], [int(rng.integers(1, 45))]))
    for k in range(64):                                          # the first and the last bases of the long paths, one substitution
        L, t = (100, 257, 300, 512)[k % 4], T[("l0", "l1")[k >> 2 & 1]]
        put("ends/" + ("first", "last")[k >> 3 & 1], _mut(rng, t[len(t) - L:] if k >> 3 & 1 else t[:L], [int(rng.integers(L))]))
    # error-free reads that the aligner takes (it seeds a read where a sketch of its windows meets one of the graph's, which not every
    # read does): drawn until the oracle has records for enough of each kind
    j13, s5, e5 = gap_at
    full = T["full"]
    pool = []
    for k in range(600):
        L = (64, 80, 100, 120)[k % 4]
        if k % 3 == 0:                                           # nodes 3 . 4, which both paths hold side by side
            name, t, lo, hi = "textless/shared", gap, j13, s5 - L
        elif k % 3 == 1:                                         # at least eight bases of the node `gap` holds alone
            name, t, lo, hi = "textless/alone", gap, s5 - L + 8, e5 - 8
        else:                                                    # at least eight bases of node 2, which `full` holds alone
            name, t, lo, hi = "full/alone", full, j13 - L + 8, j13 + 60 - 8
        x = int(rng.integers(max(lo, 0), min(hi, len(t) - L) + 1))
        pool.append((name, _rc(t[x:x + L]) if k & 4 else t[x:x + L]))
    has = _has_record(_of_reads("pool", [r for _, r in pool]), index)
    for name, n in (("textless/shared", 30), ("textless/alone", 24), ("full/alone", 24)):
        got = [(c, r) for (c, r), h in zip(pool, has) if c == name and h][:n]
        assert len(got) == n, (name, len(got))
        out += got
    return out


_CASE = {}


def build(tmp_path_factory):
    """-> (Sets of the batch of every class with its class names, {path name: global path}, {path name: text}): built once per session"""
    if not _CASE:
        tmp = tmp_path_factory.mktemp("rescue_sets_shapes")
        rng = np.random.default_rng(31)
        f0, spans = _repeat_graph(rng, tmp / "g0.gfa")
        f1, gap, gap_at = _no_text_graph(rng, tmp / "g1.gfa")
        files = [f0, f1, _short_graph(rng, tmp / "g2.gfa"), _long_graph(rng, tmp / "g3.gfa")]
        again = tmp / "g4.gfa"                                   # the repeat graph once more: the same nodes and edges under other path names
        again.write_text(open(f0).read().replace("P\tr0\t", "P\tr0b\t").replace("P\tr1\t", "P\tr1b\t"))
        index = host.Index.from_gfa_files(files + [str(again)], host.index_params(k=7, s=10, w=64))
        texts = path_texts(index)
        paths = dict(zip(PATHS, range(len(PATHS))))
        assert index.view.n_paths == len(PATHS) == 11 and index.view.path_words == 1 and index.view.n_graphs == 5
        assert [t is None for t in texts] == [n == "gap" for n in PATHS]
        assert all(t[1] == 0 and len(t[0]) == int(index.arrays["path_len"][p]) for p, t in enumerate(texts) if t is not None)
        assert texts[paths["r0b"]] == texts[paths["r0"]] and texts[paths["r1b"]] == texts[paths["r1"]]
        assert [len(texts[paths[n]][0]) for n in ("main", "p11", "p46", "l0", "l1")] == [340, 11, 46, 901, 901]
        T = {n: texts[p][0] for n, p in paths.items() if texts[p] is not None}
        named = _make_reads(np.random.default_rng(32), texts, spans, gap, gap_at)
        order = np.random.default_rng(33).permutation(len(named))
        named = [named[i] for i in order]                        # so far the batch of test_rescue_shapes, read by read
        more = _more_reads(np.random.default_rng(35), index, T, spans, gap, gap_at)
        named += [more[i] for i in np.random.default_rng(36).permutation(len(more))]
        batch = _of_reads("set shapes", [r for _, r in named])
        _CASE["case"] = (Sets(index, batch, [n for n, _ in named]), paths, T)
    return _CASE["case"]


def five_pieces(c):
    """the five pieces of test_rescue_shapes.test_pieces_in_flight: the long reads in a piece of their own, in the middle"""
    long = [r for r, n in zip(c.reads, c.names) if n.startswith("long")]
    rest = [r for r, n in zip(c.reads, c.names) if not n.startswith("long")]
    cuts = [0, len(rest) // 4, len(rest) // 2, 3 * len(rest) // 4, len(rest)]
    pieces = [_of_reads("piece %d" % i, rest[a:b]) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]
    pieces.insert(2, _of_reads("long", long))
    assert len(pieces) == 5 and min(len(r) for r in long) >= 159 and sum(p.n for p in pieces) == c.batch.n
    # (a read's records do not depend on its batch: the pieces' candidates are the batch's)
    want = dict(zip(c.reads, _has_record(c.batch, c.index)))
    assert all(want[r] == h for p in pieces for r, h in zip(_reads_of(p), _has_record(p, c.index)))
    return pieces


def redone_piece(c):
    """a sixth piece for GROOT_TEST_SMALL_BUFFERS, whose record buffers start with room for 64: every read of the batch that has a record
    and the batch's first 150 reads -> Sets of it.  A mapped read has a record at least, so the pass of this piece is redone for certain"""
    f = c.of(_of_reads("mapped and not", [c.reads[i] for i in sorted(c.exact())] + c.reads[:150]))
    assert len(f.exact()) == len(c.exact()) + sum(i in c.exact() for i in range(150)) > 2 * 64 and len(f.rescued(2)[0]) >= 20
    return f


def clean_blocks(text, rec, read):
    """per kept placement (a row of rescued_records) the blocks of A bases of the oriented read that equal the text under them"""
    out = []
    for p, x, last, strand in rec.tolist():
        o, w = (_rc(read) if strand else read), text[p][0][x - text[p][1]:last + 1 - text[p][1]]
        assert len(w) == len(o)
        out.append(sum(o[A * b:A * b + A] == w[A * b:A * b + A] for b in range(len(o) // A)))
    return out


def classes(case, paths, M):
    """the number of reads (of tuples, of records, where the name says so) of every input class under max mismatches M"""
    res, rec = case.rescued(M)[0], case.records(M)
    ex, rows = case.exact(), case.rows()
    plen = case.index.arrays["path_len"].astype(np.int64)
    names, reads = case.names, case.reads
    gap, full, p46 = paths["gap"], paths["full"], paths["p46"]

    def per(r, cols):                       # the most kept placements of one read over the values of the given columns
        return int(np.unique(r[:, cols], axis=0, return_counts=True)[1].max())

    many = {i for i, r in rec.items() if per(r, [0]) >= MANY}
    by_tuple = {}
    for i in many:
        for p, x, last in set(map(tuple, rec[i][:, :3].tolist())):
            by_tuple.setdefault((res[i].paths, p, x, last), set()).add(i)
    exact_sets, rescued_sets_ = set(ex.values()), set(r.paths for r in res.values())
    ex_on_full = set(ex[int(r)] for r, p in rows[:, :2].tolist() if p == full)
    out = {"shifted/" + c: sum(1 for i, r in rec.items() if names[i] == c and per(r, [0, 3]) >= 2) for c in SHIFTED}
    out.update({"many_on_one_path": len(many),
                "contended_tuples": sum(len(v) >= 2 for v in by_tuple.values()),
                "most_reads_on_one_tuple": max((len(v) for v in by_tuple.values()), default=0),
                "long": sum(len(reads[i]) > 256 for i in res),
                "fewest_of_a_long_length": min(sum(len(reads[i]) == L for i in res) for L in LONG),
                "exact_on_textless": sum(gap in s for s in ex.values()),
                "exact_on_textless_only": sum(s == (gap,) for s in ex.values()),
                "exact_on_both": sum(s == (gap, full) for s in ex.values()),
                "rescued_on_full_only": sum(r.paths == (full,) for r in res.values()),
                "exact_on_full_only": sum(s == (full,) for s in ex.values()),
                "rescued_on_textless": sum(gap in r.paths for r in res.values()),
                "ecs_with_exact_rows_on_full": len(ex_on_full),
                "fills_p46": sum(int(((r[:, 0] == p46) & (r[:, 1] == 0) & (r[:, 2] == plen[p46] - 1)).sum()) for r in rec.values()),
                "at_the_start_of_a_long_path": sum(bool(((r[:, 1] == 0) & (plen[r[:, 0]] > 256)).any()) for r in rec.values()),
                "at_the_end_of_a_long_path": sum(bool(((r[:, 2] == plen[r[:, 0]] - 1) & (plen[r[:, 0]] > 256)).any()) for r in rec.values()),
                "in_rescued_only_ecs": sum(r.paths not in exact_sets for r in res.values()),
                "in_ecs_with_exact_reads": sum(r.paths in exact_sets for r in res.values()),
                "rescued_only_ecs": len(rescued_sets_ - exact_sets),
                "ecs_of_both": len(rescued_sets_ & exact_sets),
                "two_graphs": sum(case.graphs_of(r.paths) == 2 for r in res.values()),
                "two_graphs_exact": sum(case.graphs_of(s) == 2 for s in ex.values())})
    return out
