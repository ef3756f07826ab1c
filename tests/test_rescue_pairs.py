"""Rescued mates in paired-end units (groot_hip_rescue_pairs_*, kernels_rescue_pairs.hpp) against the rule in plain Python
(tests/rescue_pairs_def.py): the device's ECs and every stat == test_paired.units_of_alns over S+(r), integers throughout.

Case (a) is the nine-graph index of test_rescue_ec.py and stretches of its batch -- plus error-free stretches of segment D, which have
records in all seven graphs, and reads below 32 bases, which are too short for M = 1 -- arranged as fragments, every class of the rule at
least FLOOR times in ONE batch (test_inputs_hold_every_class asserts that from the definition alone).  Case (b) is the two-graph index of
test_paired.py's case (b) with 36-base mates, one of them with a substitution: a graph both mates have in common whose AND is empty.
Every expectation comes from the CPU oracle's records and the brute force of rescue_sets_def.py, never from device output."""
import numpy as np
import pytest

from groot_amd import device, host
from rescue_def import Tables, _rc
from rescue_pairs_def import KINDS, Want, expect
from rescue_sets_def import rescued_sets
from test_abundance import _dev_ecs, ecs_of_alns
from test_counter_edges import THR, _feed, _feed_pipelined, _first_diff, _of_reads
from test_coverage import STAGES, _stage
from test_paired import _CaseB
from test_rescue import _has_record, _mut, _plain
from test_rescue_ec import _Case

FLOOR = 20
PER = 22                # fragments per class


class _Frags:
    """a batch of mates (reads 2i, 2i+1 = fragment i) on an index, and per M the definition over it"""

    def __init__(self, index, name, reads, tables=None):
        assert len(reads) % 2 == 0
        self.index, self.reads, self.batch = index, list(reads), _of_reads(name, reads)
        self.n = len(reads)
        self.gpo = index.arrays["graph_path_off"].astype(np.int64)
        self._tables, self._exact, self._res = tables, None, {}

    def exact(self):
        if self._exact is None:
            w = self.batch.want(self.index)
            r, p = w.read_ref >> 10, w.read_ref & 1023
            starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]]) if len(r) else np.zeros(0, dtype=np.int64)
            self._exact = {int(r[s]): tuple(int(v) for v in p[s:e]) for s, e in zip(starts, np.r_[starts[1:], len(r)])}
        return self._exact

    def rescued(self, M):
        """{read: R(r)}: the brute force once per distinct sequence (R(r) depends on the read's bases and the index alone)"""
        if M not in self._res:
            ex = self.exact()
            uniq = sorted({r for i, r in enumerate(self.reads) if i not in ex})
            self._tables = self._tables or Tables(self.index, 1)
            res = rescued_sets(self.index, M, uniq, np.zeros(len(uniq), dtype=bool), self._tables)[0]
            by_seq = {uniq[i]: v.paths for i, v in res.items()}
            self._res[M] = {i: by_seq[r] for i, r in enumerate(self.reads) if i not in ex and r in by_seq}
        return self._res[M]

    def want(self, M=1, max_segs=4, frags=None, on=True):
        return expect(self.gpo, self.exact(), self.rescued(M) if on else {}, self.n, max_segs, frags)

    def piece(self, a, b):
        """fragments [a, b) as a batch of their own"""
        return _of_reads("frags %d..%d" % (a, b), self.reads[2 * a:2 * b])


def _total(wants):
    ecs, cls, kinds = {}, dict(joined=0, split=0, single=0, none=0), dict.fromkeys(KINDS, 0)
    for w in wants:
        for k, v in w.ecs.items():
            ecs[k] = ecs.get(k, 0) + v
        for k in cls:
            cls[k] += w.cls[k]
        for k in KINDS:
            kinds[k] += w.kinds[k]
    s = lambda f: sum(getattr(w, f) for w in wants)
    return Want(ecs, cls, kinds, s("rescued_mates"), s("bitmap_rows"), s("bitmap_units"), s("bitmap_mates"), s("exact_slow"), sum((w.units for w in wants), []))


# ---- case (a) ---------------------------------------------------------------------------------------------------------------------------

POOL = ("clean", "len48", "len64", "len100", "x0", "xend", "segA", "segB", "segC", "segD", "segE", "segF", "repeat", "read N", "random", "blocks32/0")


class _CaseA:
    def __init__(self, tmp):
        src = _Case(tmp)
        self.index, self.tables = src.index, src._tables
        gpo = src.gpo
        graphs_of = lambda s: tuple(sorted(set((np.searchsorted(gpo, np.array(s), side="right") - 1).tolist())))
        # the pool: at most 40 reads of each of the batch's classes named above, the error-free stretches of segment D (in every graph
        # that holds it), and reads of 25 bases (too short for M = 1)
        pool, seen = [], {}
        for i, n in enumerate(src.names):
            if n in POOL and seen.get(n, 0) < 40:
                seen[n] = seen.get(n, 0) + 1
                pool.append(src.reads[i])
        d = src.shared["D"].encode()
        pool += [s for L, x in ((42, 2), (43, 1), (43, 2), (44, 0), (44, 1), (45, 0)) for s in (d[x:x + L], _rc(d[x:x + L]))]
        short = list(range(len(pool), len(pool) + 12))
        pool += [r[:25] for r in pool[:12]]
        p = _Frags(self.index, "pool", pool + [b"A" * 10] * (len(pool) & 1), self.tables)
        ex, res = p.exact(), p.rescued(1)
        E, R = sorted(ex), sorted(res)
        has_n = [i for i, r in enumerate(pool) if b"N" in r]
        left = [i for i, r in enumerate(pool) if i not in ex and i not in res and b"N" not in r and len(r) >= 32]
        assert len(E) >= 40 and len(R) >= 200 and len(has_n) >= 10 and len(left) >= 10 and len(short) >= 10
        S = lambda i: set(ex.get(i) or res.get(i))
        frs, self.classes = [], {}

        def add(name, xs, ys, cond, both=True):
            """PER fragments (x, y), x of xs and y of ys, with cond(x, y); both: as many again with the mates swapped"""
            got, n = 0, 2 * PER if both else PER
            for k in range(10 * n):
                if got == n:
                    break
                x = xs[(7 * k) % len(xs)]
                for j in range(len(ys)):
                    y = ys[(11 * k + j) % len(ys)]
                    if cond(x, y):
                        frs.append((pool[y], pool[x]) if both and got & 1 else (pool[x], pool[y]))
                        got += 1
                        break
            assert got == n, (name, got)
            self.classes[name] = (len(frs) - n, len(frs))

        multi = lambda i: len(graphs_of(sorted(S(i))))
        add("ER equal", E, R, lambda x, y: S(x) == S(y))
        add("ER subset", E, R, lambda x, y: S(x) & S(y) and not S(x) <= S(y) and not S(y) <= S(x))
        add("ER split", E, R, lambda x, y: not S(x) & S(y))
        add("RR equal", R, R, lambda x, y: x != y and S(x) == S(y), both=False)
        add("RR subset", R, R, lambda x, y: S(x) & S(y) and not S(x) <= S(y) and not S(y) <= S(x), both=False)
        add("RR split", R, R, lambda x, y: not S(x) & S(y), both=False)
        for kind, empties in (("short", short), ("N", has_n), ("unplaced", left)):
            add("E alone, " + kind, E, empties, lambda x, y: True)
            add("R alone, " + kind, R, empties, lambda x, y: True)
        add("none", has_n + left, left + has_n, lambda x, y: True)
        add("EE joined", E, E, lambda x, y: S(x) & S(y), both=False)
        add("EE split", E, E, lambda x, y: not S(x) & S(y), both=False)
        add("E7 R5", [i for i in E if multi(i) == 7], [i for i in R if multi(i) == 5], lambda x, y: True)
        add("E7 R1", [i for i in E if multi(i) == 7], [i for i in R if multi(i) == 1], lambda x, y: S(x) & S(y))
        add("R7 R2", [i for i in R if multi(i) == 7], [i for i in R if multi(i) == 2], lambda x, y: True)
        add("repeat", [i for i in R if S(i) == {self.index.view.n_paths - 1}], [i for i in R if S(i) == {self.index.view.n_paths - 1}], lambda x, y: True, both=False)
        order = np.random.default_rng(41).permutation(len(frs))
        self.where = {int(f): k for k, f in enumerate(order)}       # fragment of the list above -> its place in the batch
        self.frags = _Frags(self.index, "fragments", [m for f in order for m in frs[f]], self.tables)
        self.n = self.frags.n

    def of_class(self, name):
        a, b = self.classes[name]
        return [self.where[f] for f in range(a, b)]


@pytest.fixture(scope="module")
def case_a(tmp_path_factory, native_libs):
    return _CaseA(tmp_path_factory.mktemp("rescue_pairs"))


class _CaseBR(_CaseB):
    """test_paired's two graphs; an exact mate has test_paired's 28 bases, a mate with one substitution (`mut`) the 36 bases from four bases
    ahead of it (M = 1 takes 32)"""

    def mate(self, g, i, at, mut, rng):
        t = self.text[(g, i)]
        return _mut(rng, t[at:at + 36], [int(rng.integers(8, 28))]) if mut else t[at + 4:at + 32]

    def build(self):
        rng, fr = np.random.default_rng(43), []
        for k in range(90):
            j = int(rng.integers(-2, 3))
            mut = k % 3 != 0                                       # a third of them exact + exact: the unchanged path reaches the same sets
            fr.append((self.mate(1, 0, 64 + j, False, rng), self.mate(1, 0, 108 + j, mut, rng)))      # a, d -> {T1:(a,d)}: T0 is common, its AND empty
            fr.append((self.mate(0, 0, 64 + j, False, rng), self.mate(0, 0, 108 + j, mut, rng)))      # a, c -> {T0:(a,c)}: the mirror
            fr.append((self.mate(1, 0, 2 + j, False, rng), self.mate(1, 0, 108 + j, mut, rng)))       # {T1:(a,d)} by mates that share T1 only
            fr.append((self.mate(1, 0, 64 + j, mut, rng), self.mate(1, 0, 108 + j, not mut, rng)))    # the rescued mate on the other side
        fr = [fr[i] for i in rng.permutation(len(fr))]
        reads = []
        for i, (x, y) in enumerate(fr):
            reads += [x, _rc(y) if i & 1 else y]
        return _Frags(self.index, "two graphs", reads)


@pytest.fixture(scope="module")
def case_b(tmp_path_factory, native_libs):
    return _CaseBR(tmp_path_factory.mktemp("rescue_pairs_b")).build()


# ---- CPU: the definition alone puts every class at its floor --------------------------------------------------------------------------------

def test_inputs_hold_every_class(case_a, case_b):
    f = case_a.frags
    ex, res, w = f.exact(), f.rescued(1), f.want(1)
    gpo = f.gpo
    graphs = lambda s: len(set((np.searchsorted(gpo, np.array(sorted(s)), side="right") - 1).tolist())) if s else 0
    S = lambda r: set(ex.get(r) or res.get(r) or ())
    n = {}

    def count(name, cond, frags=None):
        n[name] = sum(1 for i in (range(f.n // 2) if frags is None else frags) if cond(2 * i, 2 * i + 1))
        assert n[name] >= FLOOR, (name, n[name])

    kind = lambda r: "E" if r in ex else "R" if r in res else "0"
    strict = lambda x, y: S(x) & S(y) and S(x) & S(y) != S(x) and S(x) & S(y) != S(y)
    for even, odd in (("E", "R"), ("R", "E")):                       # the rescued mate odd, and even
        tag = even + odd
        count(tag + " equal", lambda x, y: (kind(x), kind(y)) == (even, odd) and S(x) == S(y))
        count(tag + " subset", lambda x, y: (kind(x), kind(y)) == (even, odd) and strict(x, y))
        count(tag + " split", lambda x, y: (kind(x), kind(y)) == (even, odd) and not S(x) & S(y))
    count("RR equal", lambda x, y: kind(x) == kind(y) == "R" and S(x) == S(y))
    count("RR subset", lambda x, y: kind(x) == kind(y) == "R" and strict(x, y))
    count("RR split", lambda x, y: kind(x) == kind(y) == "R" and not S(x) & S(y))
    count("EE joined", lambda x, y: kind(x) == kind(y) == "E" and S(x) & S(y))
    count("EE split", lambda x, y: kind(x) == kind(y) == "E" and not S(x) & S(y))
    empty = {"short": lambda r: len(f.reads[r]) < 32, "N": lambda r: b"N" in f.reads[r],
             "unplaced": lambda r: kind(r) == "0" and len(f.reads[r]) >= 32 and b"N" not in f.reads[r]}
    for what, is_empty in empty.items():
        for k in "ER":
            count("%s alone, %s, even" % (k, what), lambda x, y: kind(x) == k and kind(y) == "0" and is_empty(y))
            count("%s alone, %s, odd" % (k, what), lambda x, y: kind(y) == k and kind(x) == "0" and is_empty(x))
    count("none", lambda x, y: kind(x) == kind(y) == "0")
    # a graph with more than 64 paths, the unit's bits on both sides of the 63 / 64 word edge, one mate rescued
    def edge(x, y):
        u = np.array(sorted(S(x) & S(y)))
        g = np.searchsorted(gpo, u, side="right") - 1
        return {kind(x), kind(y)} == {"E", "R"} and any({63, 64} <= set((u[g == k] - gpo[k]).tolist()) for k in set(g.tolist()))
    count("word edge", edge)
    count("E7 R5: joined in more than 4 graphs", lambda x, y: {kind(x), kind(y)} == {"E", "R"} and max(graphs(S(x)), graphs(S(y))) == 7 and graphs(S(x) & S(y)) == 5)
    count("E7 R1", lambda x, y: {kind(x), kind(y)} == {"E", "R"} and max(graphs(S(x)), graphs(S(y))) == 7 and graphs(S(x) & S(y)) == 1)
    count("R7 R2", lambda x, y: kind(x) == kind(y) == "R" and graphs(S(x)) == 7 and graphs(S(x) & S(y)) == 2)
    last = f.index.view.n_paths - 1
    count("repeat", lambda x, y: kind(x) == kind(y) == "R" and S(x) == S(y) == {last})
    print(n, w.cls, w.kinds, "bitmaps", w.bitmap_rows, w.bitmap_units, "M=2,3 rescued mates", f.want(2).rescued_mates, f.want(3).rescued_mates)
    assert w.cls["joined"] + 2 * w.cls["split"] + w.cls["single"] == sum(w.ecs.values()) == len(w.units)
    assert w.bitmap_rows >= 3 * FLOOR and f.want(1, max_segs=1).bitmap_rows >= 6 * FLOOR
    for M in (2, 3):
        assert f.want(M).rescued_mates >= 5 * FLOOR and f.want(M).ecs != w.ecs
    # case (b): both mates in T0 and T1, the AND empty in one of them, with a rescued mate and without: one set, one EC
    ex, res, wb = case_b.exact(), case_b.rescued(1), case_b.want(1)
    nb = {}
    for i in range(case_b.n // 2):
        x, y = 2 * i, 2 * i + 1
        key = (tuple(ex.get(x) or res.get(x) or ()), tuple(ex.get(y) or res.get(y) or ()), (x in res) + (y in res))
        nb[key] = nb.get(key, 0) + 1
    print(sorted(nb.items()), wb.cls, wb.kinds)
    for resc in (0, 1):                    # global paths: 0 = T0:(a,c), 1 = T0:(b,d), 2 = T1:(a,d), 3 = T1:(b,c)
        assert nb.get(((0, 2), (1, 2), resc), 0) >= FLOOR and nb.get(((0, 2), (0, 3), resc), 0) >= FLOOR and nb.get(((2, 3), (1, 2), resc), 0) >= FLOOR, nb
    assert wb.ecs[(2,)] == sum(v for k, v in nb.items() if set(k[0]) & set(k[1]) == {2})


def test_doubled_reads_are_the_unpaired_rescued_run(case_a):
    """fragments (r, r): A = B = S+(r), so the units are the classes of the unpaired run with the rescued reads in the classes"""
    f = case_a.frags
    dbl = _Frags(f.index, "doubled", [r for r in f.reads[:600] for _ in (0, 1)], f._tables)
    ex, res = f.exact(), f.rescued(1)
    unpaired = {}
    for r in range(600):
        s = ex.get(r) or res.get(r)
        if s:
            unpaired[s] = unpaired.get(s, 0) + 1
    w = dbl.want(1)
    assert w.ecs == unpaired and w.cls["split"] == w.cls["single"] == 0


# ---- the device side -----------------------------------------------------------------------------------------------------------------------

def _open(f, M=1, on=True, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    kw.setdefault("max_batch_reads", max(1024, f.n))
    al = device.Aligner(f.index, threshold=THR, **kw)
    if M:
        al.rescue_enable(M)
    if on:
        al.rescue_pairs_enable()
    return al


def _assert_device(al, w, passes=None):
    got = dict(_dev_ecs(al))
    assert got == w.ecs, _first_diff(got, w.ecs)
    ps, es, rs, st = al.pairs_stats(), al.ec_stats(), al.rescue_ec_stats(), al.rescue_pairs_stats()
    print("pairs", ps, "ec", es, "rescue_ec", rs, "rescue_pairs", st)
    assert ps == {k: w.cls[k] for k in ("joined", "split", "single")}, (ps, w.cls)
    assert ps["joined"] + 2 * ps["split"] + ps["single"] == es["reads"] == sum(w.ecs.values())
    assert (es["distinct"], es["slow_reads"]) == (len(w.ecs), w.exact_slow), (es, len(w.ecs), w.exact_slow)
    assert {k: st[k] for k in KINDS} == w.kinds, (st, w.kinds)
    assert (st["rescued_mates"], st["bitmap_units"]) == (w.rescued_mates, w.bitmap_units), (st, w.rescued_mates, w.bitmap_units)
    assert (rs["reads"], rs["slow_reads"]) == (w.rescued_mates, w.bitmap_mates), (rs, w.rescued_mates, w.bitmap_mates)
    # three kernels per pass (a pass that collect redoes launches them again; they return at once in the pass that is not counted)
    assert st["launches"] % 3 == 0 and (passes is None or st["launches"] >= 3 * passes), (st, passes)
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 3])
def test_every_class_at_once(case_a, hip_lib, monkeypatch, M):
    _stage(monkeypatch, "path_first")
    f = case_a.frags
    al = _open(f, M)
    try:
        _feed(al, [f.batch])
        _assert_device(al, f.want(M), passes=1)
        assert al.rescue_ec_stats()["rows"] == max(1024, f.n)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case_a, case_b, hip_lib, monkeypatch, stage, rod):
    _stage(monkeypatch, stage)
    for f in (case_a.frags, case_b):
        al = _open(f, results_on_device=rod)
        try:
            _feed(al, [f.batch])
            _assert_device(al, f.want(1), passes=1)
        finally:
            al.close()


@pytest.mark.gpu
def test_forced_slow_mode(case_a, case_b, hip_lib, monkeypatch):
    """GROOT_TEST_SHARED_SLOW: every fragment with a mate in more than one graph goes through the bitmaps"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    for f in (case_a.frags, case_b):
        w = f.want(1, max_segs=1)
        assert w.bitmap_units >= 2 * FLOOR
        al = _open(f)
        try:
            _feed(al, [f.batch])
            _assert_device(al, w, passes=1)
        finally:
            al.close()


@pytest.mark.gpu
def test_too_few_bitmaps_fail_the_batch(case_a, hip_lib, monkeypatch):
    """one bitmap fewer than a batch's fragments need: GROOT_E_NOSPACE that names the knob, and NOTHING of the batch counted -- the classes
    and every stat are those of the batch before it, and a batch behind it counts whole; exactly as many: every unit counted"""
    _stage(monkeypatch, "path_first")
    f = case_a.frags
    nf = f.n // 2
    w, first, rest = f.want(1), f.want(1, frags=range(100)), f.want(1, frags=range(100, nf))
    need = rest.bitmap_rows
    small, w_small = f.piece(100, 260), f.want(1, frags=range(100, 260))
    ee = rest.cls["joined"] + rest.cls["split"] - sum(rest.kinds[k] for k in KINDS[:4])
    assert 0 < first.bitmap_rows < need and 0 < w_small.bitmap_rows < need and ee >= FLOOR      # (the failing batch has exact + exact fragments too)
    monkeypatch.setenv("GROOT_TEST_RESCUE_EC_ROWS", str(need - 1))
    al = _open(f)
    try:
        assert al.rescue_ec_stats()["rows"] == need - 1
        n0 = _feed(al, [f.piece(0, 100)])
        before = _assert_device(al, first, passes=1)
        b = f.piece(100, nf)
        al.submit(b.seq, b.off, first_read_id=n0)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == -6 and "GROOT_TEST_RESCUE_EC_ROWS" in str(e.value) and "paired-end units" in str(e.value), e.value      # GROOT_E_NOSPACE
        after = _assert_device(al, first)                      # the ECs, ec_stats, pairs_stats, rescue_ec_stats and rescue_pairs_stats: unchanged
        assert {k: after[k] for k in after if k != "launches"} == {k: before[k] for k in before if k != "launches"}
        _feed(al, [small], first=n0)                            # and the ctx goes on
        _assert_device(al, _total([first, w_small]))
    finally:
        al.close()
    monkeypatch.setenv("GROOT_TEST_RESCUE_EC_ROWS", str(w.bitmap_rows))
    al = _open(f)
    try:
        _feed(al, [f.batch])
        _assert_device(al, w, passes=1)
        assert al.rescue_ec_stats()["rows"] == w.bitmap_rows
    finally:
        al.close()


def _pieces(f, cuts):
    """the batch cut at the fragments `cuts` -> [(batch, its fragments)]"""
    return [(f.piece(a, b), range(a, b)) for a, b in zip(cuts, cuts[1:])]


@pytest.mark.gpu
def test_table_growth_with_batches_in_flight(case_a, hip_lib, monkeypatch):
    """GROOT_TEST_EC_SLOTS small and three batches in flight, the later ones holding other fragments: the rows and the state of a batch are
    the ctx's, and the table of classes grows between merges"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_EC_SLOTS", "2")
    f = case_a.frags
    nf = f.n // 2
    pieces = _pieces(f, [0, nf // 4, nf // 2, 3 * nf // 4, nf])
    al = _open(f, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, [p for p, _ in pieces]) == [0] * len(pieces)
        _assert_device(al, f.want(1), passes=len(pieces))
        assert al.ec_stats()["grows"] >= 1
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pipelined_pieces_sum_to_the_batch(case_a, hip_lib, monkeypatch, small):
    """the batch cut into pieces, one empty and one of a single fragment, three in flight, from an odd first_read_id -- and the same with
    GROOT_TEST_SMALL_BUFFERS, where a piece with many records is redone at collect and counts once"""
    f = case_a.frags
    nf = f.n // 2
    pieces = _pieces(f, [0, 150, 150, 151, 300, nf])
    assert [p.n for p, _ in pieces][1:3] == [0, 2]
    wants = [f.want(1)]
    batches = [p for p, _ in pieces]
    if small:       # a piece of its own with more records than the small buffers hold: redone for certain
        ex = f.exact()
        clean = [f.reads[r] for r in sorted(ex) if len(ex[r]) > 60][:80]
        extra = _Frags(f.index, "mapped and not", (clean * 8)[:600] + f.reads[:200], f._tables)
        assert len(extra.batch.want(f.index).alns) > 20000
        wants.append(extra.want(1))
        batches.insert(4, extra.batch)
        monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    _stage(monkeypatch, "path_first")
    al = _open(f, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, batches, first=1) == [0] * len(batches)
        st = _assert_device(al, _total(wants))
        n = sum(1 for b in batches if b.n)
        assert st["launches"] > 3 * n if small else st["launches"] >= 3 * n, st
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["long", "short", "lower"])
def test_failing_batch(case_a, hip_lib, monkeypatch, kind):
    """a batch that fails with GROOT_E_NOSPACE adds nothing; one that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP counts whole, the bad
    read as an empty mate"""
    f = case_a.frags
    cut = 300                                                    # fragments in the good batch
    reads, ex = list(f.reads[2 * cut:]), f.exact()
    mid = next(i for i in range(100, len(reads)) if len(reads[i]) >= 48 and 2 * cut + i in ex)
    reads[mid] = {"long": reads[mid] * 6, "short": reads[mid][:5], "lower": reads[mid].lower()}[kind]
    code = {"long": -6, "short": -7, "lower": -8}[kind]
    _stage(monkeypatch, "path_first")
    al = _open(f)
    try:
        first = _feed(al, [f.piece(0, cut)])
        b = _of_reads(kind, reads)
        al.submit(b.seq, b.off, first_read_id=first)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == code
        if kind == "long":
            want = f.want(1, frags=range(cut))
        else:
            bad = _Frags(f.index, kind, f.reads[:2 * cut] + reads[:mid] + [b"N" * 40] + reads[mid + 1:], f._tables)      # (an empty mate in its place)
            want = bad.want(1)
        _assert_device(al, want)
    finally:
        al.close()


@pytest.mark.gpu
def test_odd_batch_is_refused_by_every_submit(case_a, hip_lib, monkeypatch):
    _stage(monkeypatch, "path_first")
    f = case_a.frags
    odd = _of_reads("odd", f.reads[:301])
    al = _open(f)
    try:
        with pytest.raises(host.GrootError) as e:
            al.submit(odd.seq, odd.off, first_read_id=0)
        assert e.value.code == -1 and "whole fragments" in str(e.value), e.value
        _feed(al, [f.batch])
        _assert_device(al, f.want(1), passes=1)
    finally:
        al.close()


def _sum(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = out.get(k, 0) + v
    return out


@pytest.mark.gpu
def test_two_ctxs_off_on_and_reset(case_a, hip_lib, monkeypatch):
    f = case_a.frags
    nf = f.n // 2
    (a, ra), (b, rb) = _pieces(f, [0, 400, nf])
    wa, wb, whole = f.want(1, frags=ra), f.want(1, frags=rb), f.want(1)
    _stage(monkeypatch, "path_first")
    al, al2 = _open(f), _open(f)
    try:
        _feed(al, [b])
        al.ec_reset()                                           # the classes, the pairing counts and the stats start over; the rule stays on
        assert _dev_ecs(al) == [] and al.rescue_pairs_stats()["rescued_mates"] == 0 and al.pairs_stats() == dict(joined=0, split=0, single=0)
        _feed(al, [a])
        s1 = _assert_device(al, wa, passes=2)
        _feed(al2, [b])
        _assert_device(al2, wb, passes=1)
        assert _sum(dict(_dev_ecs(al)), dict(_dev_ecs(al2))) == whole.ecs      # the merge of two ctxs is a sum by set
        al.rescue_enable(2); al.rescue_enable(1)                # another M and back: the classes stay
        _assert_device(al, wa, passes=2)
        al.rescue_pairs_enable(False)                           # off: the rule and the rescued classes go, the classes and pairing stay
        assert al.rescue_ec_stats()["rows"] == 0 and al.rescue_pairs_stats() == dict(dict.fromkeys(KINDS, 0), rescued_mates=0, bitmap_units=0, launches=s1["launches"])
        _feed(al, [b])
        off = f.want(1, frags=rb, on=False)                     # == pairing and the classes alone
        assert dict(_dev_ecs(al)) == _sum(wa.ecs, off.ecs)
        al.rescue_pairs_enable()                                # on again: the classes stay, the counts of the rule start from zero
        _feed(al, [b])
        assert dict(_dev_ecs(al)) == _sum(_sum(wa.ecs, off.ecs), wb.ecs)
        st = al.rescue_pairs_stats()
        assert {k: st[k] for k in KINDS} == wb.kinds and st["launches"] == s1["launches"] + 3, st
        al.ec_reset()
        al.rescue_enable(3)                                     # another M
        _feed(al, [f.batch])
        _assert_device(al, f.want(3))
        al.pairs_enable(False)                                  # pairing off takes the rule and the rescued classes with it
        assert al.rescue_ec_stats()["rows"] == 0
        al.ec_reset()
        _feed(al, [a])
        assert dict(_dev_ecs(al)) == dict(ecs_of_alns(a.want(f.index).alns))
    finally:
        al.close()
        al2.close()


@pytest.mark.gpu
def test_consequences_of_the_rule(case_a, hip_lib, monkeypatch):
    """(r, r) fragments == the unpaired run with the rescued reads in the classes; a batch without candidates == pairing and the classes alone;
    the rule off == pairing and the classes alone, and nothing launched for it"""
    _stage(monkeypatch, "path_first")
    f = case_a.frags
    orig = _of_reads("originals", f.reads[:600])
    dbl = _Frags(f.index, "doubled", [r for r in f.reads[:600] for _ in (0, 1)], f._tables)
    al = _open(f, on=False)
    try:
        al.ec_enable(); al.rescue_ec_enable()
        _feed(al, [orig])
        unpaired = dict(_dev_ecs(al))
    finally:
        al.close()
    al = _open(f)
    try:
        _feed(al, [dbl.batch])
        assert dict(_dev_ecs(al)) == unpaired == dbl.want(1).ecs
        ps = al.pairs_stats()
        assert ps["split"] == ps["single"] == 0 and ps["joined"] == sum(unpaired.values())
    finally:
        al.close()
    ex = f.exact()
    mapped = [f.reads[r] for r in sorted(ex)]
    plain = _Frags(f.index, "no candidates", mapped[:len(mapped) & ~1], f._tables)
    got = []
    for rule in (True, False):
        al = _open(f, on=rule)
        try:
            if not rule:
                al.ec_enable(); al.pairs_enable()
            _feed(al, [plain.batch])
            got.append((dict(_dev_ecs(al)), al.pairs_stats(), al.ec_stats()))
            if not rule:
                assert al.rescue_pairs_stats()["launches"] == 0 and al.rescue_ec_stats()["launches"] == 0
        finally:
            al.close()
    assert got[0] == got[1] and got[0][0] == plain.want(1).ecs
    al = _open(f, on=False)                                     # the rule off, the batch of every class: the records' fragments alone
    try:
        al.ec_enable(); al.pairs_enable()
        _feed(al, [f.batch])
        w = f.want(1, on=False)
        assert dict(_dev_ecs(al)) == w.ecs and al.pairs_stats() == {k: w.cls[k] for k in ("joined", "split", "single")}
    finally:
        al.close()


@pytest.mark.gpu
def test_everything_else_is_unchanged(case_a, hip_lib, monkeypatch):
    """records, coverage, the rescue and gap tables, their stats and the rescued records with the rule on == without it"""
    _stage(monkeypatch, "path_first")
    f = case_a.frags
    got = []
    for on in (False, True):
        al = _open(f, M=2, on=False)
        try:
            al.coverage_enable(); al.gap_enable(3); al.rescue_rec_enable(1 << 16)
            if on:
                al.rescue_pairs_enable()
            al.submit(f.batch.seq, f.batch.off, first_read_id=0)
            counts = al.wait()
            alns = al.alns()
            order = np.lexsort([alns[x] for x in reversed(alns.dtype.names)])
            got.append((counts, alns[order].tolist(), al.coverage(), al.rescue(), al.rescue_stats(), al.gap()[0], al.gap()[1].tolist(), al.gap_stats(),
                        al.rescue_records().tolist()))
            if on:
                _assert_device(al, f.want(2), passes=1)
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)
