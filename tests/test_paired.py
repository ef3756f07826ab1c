"""Paired-end counting (groot_hip_pairs_enable; kernels_shared.hpp shared_gather_paired_kernel and the kPaired kernels behind it).

The definition, quoted from include/groot_hip.h and DESIGN.md section 12:

    With pairing on, reads 2i and 2i+1 of a batch are the mates of fragment i.  The index is batch-relative: read_id - first_read_id;
    first_read_id may be odd.  Let A = S(r_2i) and B = S(r_2i+1), S(r) exactly as above.
      joined:  A and B intersect.  The fragment is one unit with the set A n B.
      split:   A and B are non-empty and do not intersect.  The fragment is two units, A and B, exactly as without pairing (mates on
               different genes are evidence for both).
      single:  exactly one of A, B is non-empty.  The fragment is one unit with that set.
      none:    both are empty.  There is no unit.
    Everywhere shared reads and equivalence classes say "read", paired mode says "unit": shared[a][b] is the number of units whose set
    holds both a and b (the diagonal: the units on a); an EC is a distinct unit set and its count the units with that set; the `reads`
    fields of the shared and EC stats count units; bootstrap replicates draw units.  Coverage, records, call counts, weights, the BAM and
    every groot_counts field do not depend on pairing.

units_of_alns restates it in plain Python over the CPU oracle's records of a batch; every expectation below comes from it, never from
device output, and every GPU test first asserts, from those records, that its input holds the case it was written for.

Case (a) is the seven-graph index of test_counter_edges.py with fragments placed on its named segments; case (b) is a two-graph index
on which the intersection empties the segment of a graph both mates have in common."""
import numpy as np
import pytest

import test_counter_edges as ce
from groot_amd import device, host, synth
from oracle import oracle_py as O
from test_abundance import _dev_ecs, ecs_of_alns
from test_counter_edges import L, NP, SEGS, THR, _Batch, _bad_batch, _feed, _feed_pipelined, _of_reads, _open
from test_coverage import STAGES, _stage, expand_coverage
from test_path_pass import _COMP, _gfa, _seq
from test_shared_reads import _dev_pairs, pairs_of_alns


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def units_of_alns(alns, n_reads, first=0):
    """-> (the unit sets of the batch, one sorted tuple of global path ids per unit, in fragment order; fragments per class)"""
    assert n_reads % 2 == 0
    sets = [set() for _ in range(n_reads)]
    for r, p in zip((alns["read_id"].astype(np.int64) - first).tolist(), alns["ref_id"].tolist()):
        sets[r].add(p)
    units, cls = [], {"joined": 0, "split": 0, "single": 0, "none": 0}
    for i in range(n_reads // 2):
        a, b = sets[2 * i], sets[2 * i + 1]
        if a & b:
            units.append(tuple(sorted(a & b)))
            cls["joined"] += 1
        elif a and b:
            units += [tuple(sorted(a)), tuple(sorted(b))]
            cls["split"] += 1
        elif a or b:
            units.append(tuple(sorted(a or b)))
            cls["single"] += 1
        else:
            cls["none"] += 1
    return units, cls


class _PWant:
    """what one batch adds in paired mode, from the oracle's records of it: the attributes test_counter_edges._Total / _check read
    (`graphs` is per unit here), plus the fragment classes"""

    def __init__(self, index, b):
        run = O.Run(index, THR)
        run.batch(b.seq, b.off)
        al = self.alns = run.alns().astype(device.ALN_DTYPE)
        self.n = b.n
        self.records, self.depth = expand_coverage(index, al, b.off)
        self.sets = [set() for _ in range(b.n)]
        for r, p in zip(al["read_id"].tolist(), al["ref_id"].tolist()):
            self.sets[r].add(p)
        self.units, self.cls = units_of_alns(al, b.n)
        gpo = index.arrays["graph_path_off"].astype(np.int64)
        self.graph_of = lambda p: int(np.searchsorted(gpo, p, side="right")) - 1
        self.unit_graphs = [tuple(sorted({self.graph_of(p) for p in u})) for u in self.units]
        self.graphs = np.array([len(g) for g in self.unit_graphs], dtype=np.int64)
        self.ecs = {}
        for u in self.units:
            self.ecs[u] = self.ecs.get(u, 0) + 1
        self.tri = ce._tri_of_ecs(self.ecs, index.view.n_paths)

    def fast_sets(self, max_segs):
        return {u for u, g in zip(self.units, self.unit_graphs) if len(g) <= max_segs}

    def read_graphs(self, r):
        return tuple(sorted({self.graph_of(p) for p in self.sets[r]}))


def _pwant(index, b):
    if getattr(b, "_pwant", None) is None:
        b._pwant = _PWant(index, b)
    return b._pwant


def _check(al, index, wants, max_segs=4, cov=True, sh=True, ec=True):
    """test_counter_edges._check on unit expectations, plus pairs_stats and its invariant"""
    t = ce._check(al, index, wants, max_segs, cov=cov, sh=sh, ec=ec)
    st = al.pairs_stats()
    print("pairs", st)
    want = {k: sum(w.cls[k] for w in wants) for k in ("joined", "split", "single")}
    assert st == want, (st, want)
    assert st["joined"] + 2 * st["split"] + st["single"] == t.reads
    if sh:
        assert al.shared_stats()["reads"] == t.reads
    if ec:
        assert al.ec_stats()["reads"] == t.reads
    return t


def _popen(index, batches, pairs=True, **kw):
    al = _open(index, batches, **kw)
    if pairs:
        al.pairs_enable()
    return al


# ---- case (a): fragments on the seven graphs of test_counter_edges.py -----------------------------------------------------------------

def _rc(s):
    return s.translate(_COMP)[::-1]


class _CaseA:
    def __init__(self, tmp):
        rng = np.random.default_rng(13)                      # test_counter_edges._build_case, keeping what it drops: the segments' texts
        self.shared = {name: _seq(rng, 45) for name, _ in SEGS}
        files = [ce._graph(rng, tmp / ("g%d.gfa" % g), g, self.shared)[0] for g in range(len(NP))]
        self.index = host.Index.from_gfa_files(files, host.index_params(k=7, s=10, w=30))
        cat, off, _ = synth.reference_sequences(self.index)
        gpo = self.index.arrays["graph_path_off"].astype(np.int64)
        self.text = lambda g, p: bytes(cat[off[gpo[g] + p]:off[gpo[g] + p + 1]])
        self.segs = {g: [name for name, members in SEGS if g in members] for g in range(len(NP))}
        self.chain = {g: 35 + 75 * len(self.segs[g]) for g in self.segs}

    # mates: L bases of a path text of graph g
    def in_seg(self, rng, name, g=None):
        """wholly inside shared segment `name`"""
        g = dict(SEGS)[name][0] if g is None else g
        at = 35 + 75 * self.segs[g].index(name) + int(rng.integers(0, 45 - L + 1))
        return self.text(g, 0)[at:at + L]

    def in_head(self, rng, g):
        at = int(rng.integers(0, 35 - L + 1))
        return self.text(g, 0)[at:at + L]

    def in_spacer(self, rng, g, k=0):
        """inside the unique spacer behind graph g's k-th shared segment"""
        at = 35 + 75 * k + 45 + int(rng.integers(0, 30 - L + 1))
        return self.text(g, 0)[at:at + L]

    def over_allele(self, rng, g, p):
        """across allele p of graph g: the end of the chain, the allele, the start of the tail"""
        t = self.text(g, p)
        at = self.chain[g] - 12 + int(rng.integers(0, 3))
        assert at + L <= len(t) and at + L >= len(t) - 35 + 4
        return t[at:at + L]

    def noise(self, rng):
        return "".join(rng.choice(list("ACGT"), L)).encode()

    @staticmethod
    def damaged(m):
        """a base in the middle that matches nowhere (alignment is exact)"""
        return m[:L // 2] + bytes([_COMP[m[L // 2]]]) + m[L // 2 + 1:]

    def fragments(self, seed, per=80):
        """-> a _Batch of `per` fragments of every class, shuffled; every second fragment has mate 2 on the other strand"""
        rng = np.random.default_rng(seed)
        fr = []
        for j in range(2 * per):      # (about half of the 28-base mates are seeded by k = 7, s = 10: the rarer classes are drawn twice per round)
            twice = j & 1
            for g, ps in ((2, (62, 63, 64)), (3, (63, 64, 127, 128))):               # proper subset of A, both sides of both word edges
                for p in ps:
                    if g == 3 or twice:
                        fr.append((self.in_head(rng, g), self.over_allele(rng, g, p)))
            g = int(rng.integers(0, 7))
            fr.append((self.in_seg(rng, "D"), self.in_spacer(rng, g, int(rng.integers(0, len(self.segs[g]))))))     # slow alone -> 1 graph
            fr.append((self.in_seg(rng, "D"), self.in_seg(rng, "E", 5)))             # -> graphs 5 and 6
            g1, g2 = rng.choice(7, 2, replace=False)
            fr.append((self.in_head(rng, int(g1)), self.in_head(rng, int(g2))))      # split: two graphs
            p1, p2 = rng.choice(NP[3], 2, replace=False)
            fr.append((self.over_allele(rng, 3, int(p1)), self.over_allele(rng, 3, int(p2))))     # split: one graph, AND zero
            fr.append((self.in_seg(rng, "D"), self.in_seg(rng, "D")))                # joined and slow: 7 graphs
            fr.append((self.in_seg(rng, "D"), self.in_seg(rng, "C")) if twice else (self.in_seg(rng, "C"), self.in_seg(rng, "D")))     # 7 + 5 graphs -> 5: slow
            if twice:
                continue
            fr.append((self.in_seg(rng, "A"), self.in_seg(rng, "B")))                # 4 + 4 graphs -> 3
            fr.append((self.damaged(self.in_seg(rng, "A")), self.in_seg(rng, "D")))  # single, the even mate unaligned
            fr.append((self.in_seg(rng, "F", 4), self.damaged(self.in_head(rng, 1))))  # single, the odd mate unaligned
            fr.append((self.noise(rng), self.noise(rng)))                           # none
        order = rng.permutation(len(fr))
        fr = [fr[i] for i in order]
        reads = []
        for i, (a, b) in enumerate(fr):
            reads += [a, _rc(b) if i & 1 else b]
        return _of_reads("fragments %d" % seed, reads)


def _assert_case_a(w):
    """the floors on the generator: every class of the issue at least 50 times per batch"""
    n = {}

    def count(k):
        n[k] = n.get(k, 0) + 1

    full = lambda gs: {p for g in gs for p in range(sum(NP[:g]), sum(NP[:g + 1]))}
    for i in range(w.n // 2):
        a, b = w.sets[2 * i], w.sets[2 * i + 1]
        ga, gb = w.read_graphs(2 * i), w.read_graphs(2 * i + 1)
        u = a & b
        gu = tuple(sorted({w.graph_of(p) for p in u}))
        if u and len(ga) == 1 and ga == gb and len(u) == 1 and u < a:
            g, p = ga[0], next(iter(u)) - sum(NP[:ga[0]])
            count(("subset", g, p))
        if ga == (0, 1, 2, 3) and gb == (0, 1, 2, 4) and gu == (0, 1, 2):
            count("4+4->3")
        if len(ga) == 7 and len(gb) == 1 and len(gu) == 1:
            count("slow+1->fast")
        if {len(ga), len(gb)} == {7, 5} and len(gu) == 5:
            count("slow unit")
        if len(ga) == 7 and gb == (5, 6) and gu == (5, 6):
            count("D+E")
        if len(ga) == 7 and len(gb) == 7 and len(gu) == 7:
            count("D+D")
        if a and b and not u:
            count("split, one graph" if ga == gb else "split, two graphs")
        if b and not a:
            count("single, even unaligned")
        if a and not b:
            count("single, odd unaligned")
        if not a and not b:
            count("none")
    print(sorted(n.items(), key=str), w.cls)
    for k in [("subset", 2, 62), ("subset", 2, 63), ("subset", 2, 64), ("subset", 3, 63), ("subset", 3, 64), ("subset", 3, 127), ("subset", 3, 128),
              "4+4->3", "slow+1->fast", "slow unit", "D+E", "D+D", "split, one graph", "split, two graphs", "single, even unaligned",
              "single, odd unaligned", "none"]:
        assert n.get(k, 0) >= 50, (k, n.get(k, 0))
    assert w.sets[0] & w.sets[1] and bool(w.sets[w.n - 2]) != bool(w.sets[w.n - 1])      # the first fragment joined, the last single-mated
    assert any(full((0, 1, 2)) == set(u) for u in w.units)
    assert (w.graphs > 4).sum() >= 100 and w.cls["joined"] > 500 and w.cls["split"] >= 100 and w.cls["single"] >= 100


def _ends_arranged(index, b):
    """b with a joined fragment moved to the front and a single-mated one to the end (which reads map is the oracle's word, so the
    two are picked from its records; the expectation is recomputed on the arranged batch)"""
    w = _PWant(index, b)
    frag = list(range(b.n // 2))
    first = next(i for i in frag if w.sets[2 * i] & w.sets[2 * i + 1])
    last = next(i for i in reversed(frag) if bool(w.sets[2 * i]) != bool(w.sets[2 * i + 1]))
    frag = [first] + [i for i in frag if i not in (first, last)] + [last]
    return b.take([r for i in frag for r in (2 * i, 2 * i + 1)], b.name)


@pytest.fixture(scope="module")
def case_a(tmp_path_factory, native_libs):
    c = _CaseA(tmp_path_factory.mktemp("paired_a"))
    return c.index, [_ends_arranged(c.index, c.fragments(seed)) for seed in (201, 202)], c


# ---- case (b): two graphs, a common graph whose AND is empty ----------------------------------------------------------------------------

class _CaseB:
    """T0 and T1: unique head, shared X, bubble {a|b}, shared Y, bubble {c|d}, shared Z, unique tail; T0 = (a,c), (b,d); T1 = (a,d), (b,c)"""

    def __init__(self, tmp):
        rng = np.random.default_rng(29)
        X, Y, Z = (_seq(rng, 40) for _ in range(3))
        a, b, c, d = "ACCA", "GTTG", "CAAC", "TGGT"
        files = []
        self.text = {}
        for g, ch in ((0, ((a, c), (b, d))), (1, ((a, d), (b, c)))):
            head, tail = _seq(rng, 40), _seq(rng, 40)
            nodes = {1: head, 2: X, 3: a, 4: b, 5: Y, 6: c, 7: d, 8: Z, 9: tail}
            edges = [(1, 2), (2, 3), (2, 4), (3, 5), (4, 5), (5, 6), (5, 7), (6, 8), (7, 8), (8, 9)]
            ids = {a: 3, b: 4, c: 6, d: 7}
            paths = [("t%dp%d" % (g, i), [1, 2, ids[x], 5, ids[y], 8, 9]) for i, (x, y) in enumerate(ch)]
            files.append(_gfa(tmp / ("t%d.gfa" % g), nodes, edges, paths))
            for i, (x, y) in enumerate(ch):
                self.text[(g, i)] = (head + X + x + Y + y + Z + tail).encode()
        self.index = host.Index.from_gfa_files(files, host.index_params(k=7, s=10, w=30))

    def over1(self, rng, g, i):         # across bubble 1 of path i of graph g
        at = 80 - 12 + int(rng.integers(-2, 3))
        return self.text[(g, i)][at:at + L]

    def over2(self, rng, g, i):         # across bubble 2
        at = 124 - 12 + int(rng.integers(-2, 3))
        return self.text[(g, i)][at:at + L]

    def in_x(self, rng):
        at = 40 + int(rng.integers(0, 40 - L + 1))
        return self.text[(0, 0)][at:at + L]

    def in_head(self, rng, g):
        at = int(rng.integers(0, 40 - L + 1))
        return self.text[(g, 0)][at:at + L]

    def fragments(self, seed, per=150):
        rng = np.random.default_rng(seed)
        fr = []
        for _ in range(per):
            fr.append((self.over1(rng, 1, 0), self.over2(rng, 1, 0)))      # a, d -> {T1:(a,d)}: T0 is common and its AND is empty
            fr.append((self.over1(rng, 0, 0), self.over2(rng, 0, 0)))      # a, c -> {T0:(a,c)}: the mirror
            fr.append((self.in_x(rng), self.in_x(rng)))                    # all four paths
            fr.append((self.in_head(rng, 1), self.over2(rng, 1, 0)))       # {T1:(a,d)} again, by a key that never held T0
            fr.append((self.over1(rng, 0, 1), self.over2(rng, 1, 0)))      # b, d -> {T0:(b,d)}
            fr.append((self.in_head(rng, 0), self.in_head(rng, 1)))        # split
            fr.append((self.in_x(rng), "".join(rng.choice(list("ACGT"), L)).encode()))
        fr = [fr[i] for i in rng.permutation(len(fr))]
        reads = []
        for i, (x, y) in enumerate(fr):
            reads += [x, _rc(y) if i & 1 else y]
        return _of_reads("two graphs %d" % seed, reads)


def _assert_case_b(w):
    n = {}
    for i in range(w.n // 2):
        a, b = w.sets[2 * i], w.sets[2 * i + 1]
        key = (tuple(sorted(a)), tuple(sorted(b)))
        n[key] = n.get(key, 0) + 1
    print(sorted(n.items()), w.cls)
    # global paths: 0 = T0:(a,c), 1 = T0:(b,d), 2 = T1:(a,d), 3 = T1:(b,c)
    assert n.get(((0, 2), (1, 2)), 0) >= 50          # A = {T0:(a,c), T1:(a,d)}, B = {T0:(b,d), T1:(a,d)}: both in T0, unit in T1 alone
    assert n.get(((0, 2), (0, 3)), 0) >= 50          # the mirror: unit in T0 alone
    assert n.get(((0, 1, 2, 3), (0, 1, 2, 3)), 0) >= 50
    assert n.get(((2, 3), (1, 2)), 0) >= 50          # {T1:(a,d)} from mates that share T1 only: the same key must come out
    assert {(2,), (0,), (0, 1, 2, 3)} <= set(w.ecs)
    assert w.ecs[(2,)] == n[((0, 2), (1, 2))] + n[((2, 3), (1, 2))]


@pytest.fixture(scope="module")
def case_b(tmp_path_factory, native_libs):
    c = _CaseB(tmp_path_factory.mktemp("paired_b"))
    return c.index, [c.fragments(301), c.fragments(302)], c


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_generators_reach_every_class(case_a, case_b):
    index, batches, _ = case_a
    assert index.view.path_words == 3 and index.view.n_paths == sum(NP)
    for b in batches:
        assert b.n % 2 == 0 and 2000 <= b.n <= 6000
        _assert_case_a(_pwant(index, b))
    index, batches, _ = case_b
    assert index.view.n_graphs == 2 and index.view.n_paths == 4
    for b in batches:
        _assert_case_b(_pwant(index, b))


def test_units_of_doubled_reads_are_the_reads(case):
    """every read followed by a copy of itself: A = B, so the units are exactly the per-read sets of the original batch"""
    index, batches = case
    sub = batches[0].take(np.arange(1500), "slice")
    w = sub.want(index)
    dbl = sub.take(np.repeat(np.arange(sub.n), 2), "doubled")
    run = O.Run(index, THR)
    run.batch(dbl.seq, dbl.off)
    al = run.alns().astype(device.ALN_DTYPE)
    units, cls = units_of_alns(al, dbl.n)
    ecs = {}
    for u in units:
        ecs[u] = ecs.get(u, 0) + 1
    assert ecs == dict(ecs_of_alns(w.alns)) and cls["split"] == cls["single"] == 0 and cls["joined"] == int((w.graphs > 0).sum())
    a, b = np.nonzero(ce._tri_of_ecs(ecs, index.view.n_paths))
    tri = ce._tri_of_ecs(ecs, index.view.n_paths)
    assert {(int(x), int(y)): int(tri[x, y]) for x, y in zip(a, b)} == pairs_of_alns(w.alns)


case = ce.case


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_class_at_once(case_a, case_b, hip_lib, monkeypatch, which, stage, rod):
    """two batches of every class through one ctx, all three counters on: pairs, ECs and all stats are the restatement's, coverage the
    unpaired expectation"""
    index, batches, _ = case_a if which == "a" else case_b
    wants = [_pwant(index, b) for b in batches]
    for w in wants:
        (_assert_case_a if which == "a" else _assert_case_b)(w)
    _stage(monkeypatch, stage)
    al = _popen(index, batches, results_on_device=rod)
    try:
        _feed(al, batches)
        t = _check(al, index, wants)
        assert (t.slow > 0) == (which == "a")
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["a", "b"])
def test_forced_slow_mode(case_a, case_b, hip_lib, monkeypatch, which):
    """GROOT_TEST_SHARED_SLOW (max_segs = 1): every multi-graph intersection is a slow unit, single-graph intersections of
    multi-graph mates stay fast"""
    index, batches, _ = case_a if which == "a" else case_b
    wants = [_pwant(index, b) for b in batches]
    for w in wants:
        multi = [i for i in range(w.n // 2) if w.sets[2 * i] & w.sets[2 * i + 1] and len(w.read_graphs(2 * i)) > 1 and len(w.read_graphs(2 * i + 1)) > 1
                 and len({w.graph_of(p) for p in w.sets[2 * i] & w.sets[2 * i + 1]}) == 1]
        assert (w.graphs > 1).sum() >= 100 and (len(multi) >= 50 or which == "a")
        assert which == "b" or sum(1 for i in range(w.n // 2) if len(w.read_graphs(2 * i)) == 7 and len(w.read_graphs(2 * i + 1)) == 1) >= 50
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    al = _popen(index, batches)
    try:
        _feed(al, batches)
        t = _check(al, index, wants, max_segs=1)
        assert t.slow == sum(int((w.graphs > 1).sum()) for w in wants)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("on", ["ec_only", "shared_only"])
def test_one_of_shared_and_ec_in_either_order(case_a, hip_lib, monkeypatch, on):
    """pairing switched on before the counter it acts on, and only one of the two counters on"""
    index, batches, _ = case_a
    wants = [_pwant(index, b) for b in batches]
    assert all((w.graphs > 4).sum() > 32 for w in wants)
    _stage(monkeypatch, "path_first")
    al = _open(index, batches, sh=False, ec=False)
    try:
        al.pairs_enable()
        al.shared_enable() if on == "shared_only" else al.ec_enable()
        _feed(al, batches)
        _check(al, index, wants, sh=on == "shared_only", ec=on == "ec_only")
    finally:
        al.close()


@pytest.mark.gpu
def test_odd_first_read_id_and_the_largest_ids(case_a, hip_lib, monkeypatch):
    """the fragment index is batch-relative: an odd first_read_id, and ids that end at 2^32 - 1"""
    index, batches, _ = case_a
    wants = [_pwant(index, b) for b in batches]
    _stage(monkeypatch, "path_first")
    al = _popen(index, batches)
    try:
        first = (1 << 32) - sum(b.n for b in batches)
        al.submit(batches[0].seq, batches[0].off, first_read_id=7)
        assert al.wait()["received"] == batches[0].n
        _check(al, index, wants[:1])
        al.shared_reset(), al.ec_reset(), al.coverage_reset()
        assert al.pairs_stats() == {"joined": 0, "split": 0, "single": 0}
        assert _feed(al, batches, first) == 1 << 32
        _check(al, index, wants)
        t, _ = al.travs()
        assert int(t["read_id"].max()) > (1 << 32) - 64 and int(t["read_id"].min()) >= first + batches[0].n
    finally:
        al.close()


@pytest.mark.gpu
def test_pipeline_with_empty_and_two_read_batches(case_a, hip_lib, monkeypatch):
    """depth 3, batches of 0 and 2 reads between full ones; a second ctx fed one batch at a time has the same totals"""
    index, (b0, b1), _ = case_a
    w0 = _pwant(index, b0)
    slow = next(i for i in range(b0.n // 2) if len({w0.graph_of(p) for p in w0.sets[2 * i] & w0.sets[2 * i + 1]}) > 4)
    split = next(i for i in range(b0.n // 2) if w0.sets[2 * i] and w0.sets[2 * i + 1] and not w0.sets[2 * i] & w0.sets[2 * i + 1])
    empty = _Batch("empty", np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    seq = [b0, empty, b0.take([2 * slow, 2 * slow + 1], "one slow fragment"), b1, b0.take([2 * split, 2 * split + 1], "one split fragment"), empty, b1]
    wants = [_pwant(index, b) for b in seq]
    assert wants[2].cls["joined"] == 1 and wants[2].graphs.tolist() in ([5], [7])
    assert wants[4].cls["split"] == 1 and len(wants[4].units) == 2
    _stage(monkeypatch, "path_first")
    out = []
    for pipelined in (True, False):
        al = _popen(index, seq, pipeline_depth=3 if pipelined else 0)
        try:
            if pipelined:
                assert _feed_pipelined(al, seq) == [0] * len(seq)
            else:
                _feed(al, seq)
            _check(al, index, wants)
            out.append((_dev_pairs(al), _dev_ecs(al), al.pairs_stats(), al.shared_stats(), al.ec_stats()["reads"]))
        finally:
            al.close()
    assert out[0] == out[1]


@pytest.mark.gpu
def test_redone_batch_counts_once(case_a, hip_lib, monkeypatch):
    """GROOT_TEST_SMALL_BUFFERS: the first pass of each batch overflows and is redone at collect; only the redo counts"""
    index, batches, _ = case_a
    wants = [_pwant(index, b) for b in batches]
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    al = _popen(index, batches)
    try:
        _feed(al, batches)
        _check(al, index, wants)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(ce._CODE))
def test_failing_batch(case_a, hip_lib, monkeypatch, kind):
    """a GROOT_E_NOSPACE batch is not counted at all; GROOT_E_SHORT_READ and GROOT_E_REVCOMP batches are counted whole, and the bad
    read's mate counts as single"""
    index, (b0, b1), _ = case_a
    w1 = _pwant(index, b1)
    # the bad read lands in the middle of the batch (_bad_batch): make sure a joined fragment sits there
    half = b1.n // 2
    mid = next(i for i in range(half // 2, half) if w1.sets[2 * i] & w1.sets[2 * i + 1])
    order = np.arange(b1.n)
    k = (b1.n // 2) & ~1
    order[[k, k + 1, 2 * mid, 2 * mid + 1]] = order[[2 * mid, 2 * mid + 1, k, k + 1]]
    src = b1.take(order, "bad source")
    bad, bad_wants = _bad_batch(index, src, kind)
    bi = src.n // 2               # (where _bad_batch puts the bad read: the even mate of that joined fragment)
    assert bi == k and _pwant(index, src).sets[bi] & _pwant(index, src).sets[bi + 1]
    pw = []
    if bad_wants:
        if kind == "short":       # the oracle refuses the batch: the bad read replaced by one without records stands for it
            reads = [bytes(src.seq[i * L:(i + 1) * L]) for i in range(src.n)]
            reads[bi] = _CaseA.damaged(reads[bi])
            pw = [_pwant(index, _of_reads("short, stand-in", reads))]
        else:
            pw = [_pwant(index, bad)]
        assert not pw[0].sets[bi] and pw[0].sets[bi + 1] and pw[0].cls["single"] == _pwant(index, src).cls["single"] + 1     # was joined, now single
    _stage(monkeypatch, "path_first")
    al = _popen(index, [b0, bad], max_read_len=64)
    try:
        first = _feed(al, [b0])
        al.submit(bad.seq, bad.off, first_read_id=first)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == ce._CODE[kind]
        _check(al, index, [_pwant(index, b0)] + pw)
        _feed(al, [b0], first + bad.n)
        _check(al, index, [_pwant(index, b0)] + pw + [_pwant(index, b0)])
    finally:
        al.close()


@pytest.mark.gpu
def test_table_growth_with_slow_units_in_flight(case_a, hip_lib, monkeypatch):
    """GROOT_TEST_EC_SLOTS=8, three batches in flight: the run-wide table grows while batches with slow units are between merge and collect"""
    index, (b0, b1), _ = case_a
    seq = [b0.take(np.arange(400), "400"), b1.take(np.arange(1000), "1000"), b0, b1, b0.take(np.arange(1000, 2600), "1600")]
    wants = [_pwant(index, b) for b in seq]
    assert all((w.graphs > 4).sum() > 0 for w in wants)
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_EC_SLOTS", "8")
    al = _popen(index, seq, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, seq) == [0] * len(seq)
        _check(al, index, wants)
        assert al.ec_stats()["grows"] >= 2
    finally:
        al.close()


@pytest.mark.gpu
def test_odd_batch_is_refused_by_every_submit(case_a, hip_lib, monkeypatch):
    """GROOT_E_INVALID, nothing enqueued, every counter unchanged, and the next even batch counts"""
    index, (b0, b1), _ = case_a
    odd = b1.take(np.arange(999), "odd")
    _stage(monkeypatch, "path_first")
    al = _popen(index, [b0])
    try:
        _feed(al, [b0])
        before = (_dev_pairs(al), _dev_ecs(al), al.pairs_stats(), al.shared_stats(), al.ec_stats(), [x.copy() for x in al.coverage()])
        with pytest.raises(host.GrootError) as e:
            al.submit(odd.seq, odd.off, first_read_id=b0.n)
        assert e.value.code == -1
        import torch
        pk, ep, eb = host.pack_reads(odd.seq)
        lens = np.full(odd.n, L, dtype=np.uint16)
        dev = torch.device("cuda", 0)
        d_seq = torch.zeros(len(odd.seq) + 64, dtype=torch.uint8, device=dev)
        d_seq[: len(odd.seq)] = torch.from_numpy(odd.seq).to(dev)
        d_off = torch.from_numpy(odd.off.astype(np.int64)).to(dev)
        torch.cuda.synchronize()
        b = al.acquire()
        b["packed"][: len(pk)] = pk
        b["seq_len"][: odd.n] = lens
        for call in (lambda: al.submit_packed(pk, odd.off, ep, eb, first_read_id=b0.n),
                     lambda: al.submit_packed16(pk, lens, ep, eb, first_read_id=b0.n),
                     lambda: al.submit_acquired(b["ticket"], odd.n, 0, first_read_id=b0.n),
                     lambda: al.submit_device(d_seq.data_ptr(), d_off.data_ptr(), odd.n, first_read_id=b0.n, max_len=L)):
            with pytest.raises(host.GrootError) as e:
                call()
            assert e.value.code == -1
        al.submit_acquired(b["ticket"], 0, 0, first_read_id=b0.n)       # the batch stayed acquired: handed back empty
        al.wait()
        assert al.in_flight()[0] == 0
        after = (_dev_pairs(al), _dev_ecs(al), al.pairs_stats(), al.shared_stats(), al.ec_stats(), al.coverage())
        assert before[:5] == after[:5] and all(np.array_equal(x, y) for x, y in zip(before[5], after[5]))
        al.submit(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), first_read_id=b0.n)       # 0 reads is fine
        al.wait()
        _feed(al, [b1], b0.n)
        _check(al, index, [_pwant(index, b0), _pwant(index, b1)])
    finally:
        al.close()


@pytest.mark.gpu
def test_enable_in_flight_is_refused_and_off_counts_reads_again(case_a, hip_lib, monkeypatch):
    """GROOT_E_STATE while a batch is in flight; after switching off (and a reset) the counts are per read, as test_counter_edges has them"""
    index, (b0, b1), _ = case_a
    _stage(monkeypatch, "path_first")
    al = _popen(index, [b0, b1], pairs=False, pipeline_depth=2)
    try:
        with pytest.raises(host.GrootError) as e:
            al.pairs_stats()
        assert e.value.code == -9
        al.submit(b0.seq, b0.off, first_read_id=0)
        with pytest.raises(host.GrootError) as e:
            al.pairs_enable()
        assert e.value.code == -9
        r = al.collect(check=False)
        al.release(r["ticket"])
        ce._check(al, index, [b0.want(index)])                  # unpaired: that batch counted per read
        al.shared_reset(), al.ec_reset(), al.coverage_reset()
        al.pairs_enable()
        _feed(al, [b1], b0.n)
        _check(al, index, [_pwant(index, b1)])
        al.pairs_enable(False)
        al.shared_reset(), al.ec_reset(), al.coverage_reset()
        _feed(al, [b1], b0.n + b1.n)
        ce._check(al, index, [b1.want(index)])
        with pytest.raises(host.GrootError):
            al.pairs_stats()
    finally:
        al.close()


@pytest.mark.gpu
def test_pairing_without_counters_changes_nothing(case_a, hip_lib, monkeypatch):
    """pairing on with shared reads and ECs both off: counts, records and coverage equal a ctx without it"""
    index, (b0, b1), _ = case_a
    _stage(monkeypatch, "path_first")
    out = []
    for pairs in (False, True):
        al = _popen(index, [b0], pairs=pairs, sh=False, ec=False)
        try:
            al.submit(b0.seq, b0.off)
            c = al.wait()
            out.append((c, al.alns(), al.coverage()))
            if pairs:
                assert al.pairs_stats() == {"joined": 0, "split": 0, "single": 0}
        finally:
            al.close()
    assert out[0][0] == out[1][0]
    assert all(np.array_equal(out[0][1][f], out[1][1][f]) for f in device.ALN_DTYPE.names)
    assert all(np.array_equal(x, y) for x, y in zip(out[0][2], out[1][2]))


@pytest.mark.gpu
def test_doubled_reads_on_argannot(argannot_index, hip_lib, monkeypatch):
    """(r, r) fragments on the arg-annot index (path sets of three words): a paired run equals the unpaired run of the originals"""
    index = argannot_index
    assert index.view.path_words == 3
    seq, off, _ = synth.reads_np(*synth.reference_sequences(index), 3000, 100)        # error-free reads: nearly all of them map
    reads = [bytes(seq[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
    dseq, doff = O.pack_reads([r for r in reads for _ in (0, 1)])
    _stage(monkeypatch, "path_first")
    out = []
    for pairs, (s, o) in ((False, (seq, off)), (True, (dseq, doff))):
        al = device.Aligner(index, max_batch_reads=8192)
        try:
            al.shared_enable(), al.ec_enable()
            if pairs:
                al.pairs_enable()
            al.submit(s, o)
            al.wait()
            out.append((_dev_pairs(al), _dev_ecs(al), al.shared_stats(), al.ec_stats()["reads"]))
            if pairs:
                st = al.pairs_stats()
                assert st["split"] == st["single"] == 0 and st["joined"] == out[0][3] > 1000
        finally:
            al.close()
    assert out[0] == out[1]
