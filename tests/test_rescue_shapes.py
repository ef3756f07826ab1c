"""Mismatch rescue (kernels_rescue.hpp) at the shapes tests/test_rescue.py does not reach, against the same brute force (tests/rescue_def.py):

    repeats         tandem repeats of period 1, 3, 16 and 20: the blocks of a read share one key, a key has many occurrences in one path,
                    and shifted copies of a read are placements of their own (the count-once rule of rescue_count_kernel); keys 0 (poly-A:
                    also what a free table slot holds), 0xAAAAAAAA (poly-T), 0xFFFFFFFF (poly-G);
    a text-less path  it owns path_len + 1 slots of the dense tables and of the export's prefix sums, and takes no placement;
    short paths     one of 11 bases (below the anchor: no table entry), one of 46 (shorter than every candidate at M >= 2: every occurrence in
                    it hangs over its end; at M = 1 a read of 46 bases fills it exactly);
    long reads      159 .. 512 bases (5 .. 16 words, 9 .. 32 blocks), substitutions on both sides of every word edge from 128 upwards;
    a full buffer   exactly max_batch_reads candidates of exactly max_batch_bases bases.

Four small graphs, built here.  The expectation comes from rescue_def.Tables and from the oracle's records (test_rescue._has_record) only.

One addition to the repeat graph: an "A" * 72 run next to the "A" * 40 one.  A candidate has at least 48 bases, so none lies inside a run of
40; a read that hangs out of the run into unique sequence has no shifted copy within M <= 3 (the shift moves every unique base onto another
one).  Only a run longer than the read holds shifted placements of one read under one key, and the key that matters is 0."""
import numpy as np
import pytest

from groot_amd import device, host
from rescue_def import A, _rc, path_texts
from test_counter_edges import THR, _feed, _feed_pipelined, _of_reads
from test_coverage import STAGES, _stage
from test_path_pass import _gfa, _seq
from test_rescue import _assert_device, _expect, _has_record, _mut, _reads_of

REP_LENGTHS = (48, 64, 80, 100)
LONG = (159, 160, 161, 191, 192, 193, 255, 256, 257, 300, 511, 512)
SHIFTED = ("period16/keep0", "period16/keep1", "period16/keep2", "period20", "period3", "homopolymer")
_SWAP = bytes.maketrans(b"ACGT", b"CATG")                       # every base to another one


# ---- the index -----------------------------------------------------------------------------------------------------------------------

def _repeat_graph(rng, path):
    """60 unique . A*40 . 40 u . ACG*20 . 40 u . W16*4 . 40 u . W20*4 . 60 u . (A | C) . 20 u . T*40 . 20 u . G*40 . 20 u . A*72 . 20 u
    -> (file, {class: [(first base, behind the last, period)]})"""
    w16, w20 = _seq(rng, 16), _seq(rng, 20)
    head = [(None, _seq(rng, 60)), ("homopolymer", "A" * 40), (None, _seq(rng, 40, "A")), ("period3", "ACG" * 20), (None, _seq(rng, 40, "A")),
            ("period16", w16 * 4), (None, _seq(rng, 40, w16[0])), ("period20", w20 * 4), (None, _seq(rng, 60, w20[0]))]
    tail = [(None, _seq(rng, 20)), ("homopolymer", "T" * 40), (None, _seq(rng, 20, "T")), ("homopolymer", "G" * 40), (None, _seq(rng, 20, "G")),
            ("homopolymer", "A" * 72), (None, _seq(rng, 20, "A"))]
    spans, at = {}, 0
    for part in (head, [(None, "A")], tail):
        for name, s in part:
            if name:
                spans.setdefault(name, []).append((at, at + len(s), {"homopolymer": 1, "period3": 3, "period16": 16, "period20": 20}[name]))
            at += len(s)
    nodes = {1: "".join(s for _, s in head), 2: "A", 3: "C", 4: "".join(s for _, s in tail)}
    return _gfa(path, nodes, [(1, 2), (1, 3), (2, 4), (3, 4)], [("r0", [1, 2, 4]), ("r1", [1, 3, 4])]), spans


def _no_text_graph(rng, path):
    """the no_text case of test_path_pass.py with nodes of 60 .. 70 bases: `gap` goes 1 -> 3 with no L edge, node 5 lies on it alone
    -> (file, the spelling of gap, (the 1 | 3 junction, first base of node 5, behind its last))"""
    nodes = {1: _seq(rng, 64), 2: _seq(rng, 60), 3: _seq(rng, 66), 4: _seq(rng, 62), 5: "A" + _seq(rng, 60), 6: "C" + _seq(rng, 59), 7: _seq(rng, 70)}
    edges = [(1, 2), (2, 3), (3, 4), (4, 5), (4, 6), (5, 7), (6, 7)]
    f = _gfa(path, nodes, edges, [("gap", [1, 3, 4, 5, 7]), ("full", [1, 2, 3, 4, 6, 7])])
    at5 = len(nodes[1] + nodes[3] + nodes[4])
    return f, "".join(nodes[i] for i in (1, 3, 4, 5, 7)).encode(), (len(nodes[1]), at5, at5 + len(nodes[5]))


def _short_graph(rng, path):
    """main = 10 + 30 + 300 bases, p11 = the 10 and a one-base sink, p46 = 10 + 30 + 6 (the 6 differ from main's next 6 in every base)"""
    c = _seq(rng, 300)
    b = _seq(rng, 30)
    nodes = {1: _seq(rng, 10), 2: b, 3: c, 4: _seq(rng, 1, b[0]), 5: c[:6].encode().translate(_SWAP).decode()}
    return _gfa(path, nodes, [(1, 2), (2, 3), (1, 4), (2, 5)], [("main", [1, 2, 3]), ("p11", [1, 4]), ("p46", [1, 2, 5])])


def _long_graph(rng, path):
    nodes = {1: _seq(rng, 400), 2: "A", 3: "C", 4: _seq(rng, 500)}
    return _gfa(path, nodes, [(1, 2), (1, 3), (2, 4), (3, 4)], [("l0", [1, 2, 4]), ("l1", [1, 3, 4])])


# ---- the reads -----------------------------------------------------------------------------------------------------------------------

def _make_reads(rng, texts, spans, gap, gap_at, M=2):
    """-> [(class name, read)]"""
    out = []
    r0, full, main, p11, p46, l0, l1 = (texts[p][0] for p in (0, 3, 4, 5, 6, 7, 8))

    def add(name, t, x, L, at, strand=None):
        assert 0 <= x and x + L <= len(t), (name, x, L, len(t))
        s = _mut(rng, t[x:x + L], at)
        out.append((name, _rc(s) if (len(out) & 1 if strand is None else strand) else s))

    subs = lambda L, n: rng.choice(L, n, replace=False)
    for name, where in sorted(spans.items()):
        for s, e, per in where:
            for L in REP_LENGTHS:                                # inside the repeat or over one or both of its edges, at least 32 bases in it
                for nm in range(M + 1):
                    for k in range(4):
                        add(name, r0, int(rng.integers(max(0, s - (L - 32)), min(e - 32, len(r0) - L) + 1)), L, subs(L, nm))
            fit = [L for L in REP_LENGTHS if L + per <= e - s]   # inside it with room for a copy one period to the left or to the right
            for k in range(45 if fit and name != "period16" else 0):
                L = fit[k % len(fit)]
                x = int(rng.integers(s, e - L + 1))
                while x + per > e - L and x - per < s:
                    x = int(rng.integers(s, e - L + 1))
                add(name, r0, x, L, subs(L, k % (M + 1)))
    # period 16: a substitution in every block before `keep`, so that block `keep` is the first clean one and the later blocks are clean
    # with its key; 48 bases at either end of the 64 (the other end is the shifted copy), the whole 64, and 80 / 100 over the edges
    (s16, e16, _), = spans["period16"]
    for keep in range(4):
        for k in range(44):
            L, x = ((48, s16 + 16 * (k & 1)), (64, s16), (80, s16 - 16 * (k & 1)), (100, s16 - 16))[0 if k < 30 else 1 + k % 3]
            if keep < L // A:
                at = [A * b + int(rng.integers(A)) for b in range(keep)] or [L - 1 - int(rng.integers(A))]      # (keep 0: one in the last block, or the read is error-free and aligned)
                add("period16/keep%d" % keep, r0, x, L, at, strand=k >> 1 & 1)
    # the text-less path's own spelling over the missing junction and through the node it alone holds; its neighbour's text
    j13, s5, e5 = gap_at
    for k in range(90):
        L = (48, 64, 100)[k % 3]
        x = int(rng.integers(max(0, j13 - L + 16), j13 - 15)) if k < 45 else int(rng.integers(max(s5 + 16 - L, j13), min(e5 - 16, len(gap) - L) + 1))
        add("gap", gap, x, L, subs(L, 1))
    for k in range(45):
        L = (48, 64, 100)[k % 3]
        add("full", full, int(rng.integers(0, len(full) - L + 1)), L, subs(L, 1))
    # the short paths: windows of main that begin inside its first 46 bases; p46 and p11 run on into main (6 bases off, one base off);
    # for M = 1, p46 filled exactly and its last 32 bases
    assert main[:40] == p46[:40] and main[:10] == p11[:10] and len(p46) == 46 and len(p11) == 11
    for x in range(46):
        for L in (48, 64):
            add("short", main, x, L, subs(L, 1))
    for k in range(30):
        L = (48, 64)[k & 1]
        add("short/p46", p46 + main[46:], 0, L, subs(L, 1))
        add("short/p11", p11 + main[11:], 0, L, [11 + int(rng.integers(L - 11))])
        add("short/fit", p46, *((14, 32) if k & 1 else (0, 46)), [int(rng.integers(1, 31))])
    # long reads
    for L in LONG:
        for nm in range(M + 2):
            for k in range(5):
                add("long", (l0, l1)[k & 1], int(rng.integers(0, len(l0) - L + 1)), L, subs(L, nm))
    for L in (256, 257, 512):
        edges = [[e - 1] for e in range(128, L, 32)] + [[e] for e in range(128, L, 32)] + [[e - 1, e] for e in range(128, L, 32)] + [[L - 1, 40]]
        for k, at in enumerate(edges * 2):
            add("long/pos", (l0, l1)[k & 1], int(rng.integers(0, len(l0) - L + 1)), L, at, strand=k >= len(edges))
    for k in range(44):                                          # over the bubble base (400) with one substitution: d = 1 on one path, 2 on the other
        L = (257, 300, 511, 512)[k % 4]
        x = int(rng.integers(max(0, 401 - L + 8), min(400 - 8, len(l0) - L) + 1))
        at = int(rng.integers(L))
        add("long/bubble", (l0, l1)[k >> 2 & 1], x, L, [at if x + at != 400 else at - 1])
    # controls
    for k in range(60):
        out.append(("random", _seq(rng, (48, 64, 100, 160, 300, 512)[k % 6]).encode()))
    for k in range(30):
        L = (100, 300)[k & 1]
        r = bytearray(_mut(rng, l0[k:k + L], [L // 2]))
        r[int(rng.integers(L))] = ord("N")
        out.append(("read N", bytes(r)))
    return out


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    """(index of the four graphs, the batch of every class, its class names, {M: Tables}, the global path ids by name)"""
    tmp = tmp_path_factory.mktemp("rescue_shapes")
    rng = np.random.default_rng(31)
    f0, spans = _repeat_graph(rng, tmp / "g0.gfa")
    f1, gap, gap_at = _no_text_graph(rng, tmp / "g1.gfa")
    files = [f0, f1, _short_graph(rng, tmp / "g2.gfa"), _long_graph(rng, tmp / "g3.gfa")]
    index = host.Index.from_gfa_files(files, host.index_params(k=7, s=10, w=64))
    texts = path_texts(index)
    paths = dict(zip(("r0", "r1", "gap", "full", "main", "p11", "p46", "l0", "l1"), range(9)))
    assert index.view.n_paths == 9 and [t is None for t in texts] == [p == paths["gap"] for p in range(9)]
    assert sum(t is not None and len(t[0]) < A for t in texts) == 1 and sum(t is not None and A <= len(t[0]) < 48 for t in texts) == 1     # 11 and 46 bases
    assert [len(texts[paths[n]][0]) for n in ("main", "p11", "p46", "l0", "l1")] == [340, 11, 46, 901, 901]
    assert all(texts[p][1] == 0 and len(texts[p][0]) == int(index.arrays["path_len"][p]) for p in range(9) if p != paths["gap"])
    named = _make_reads(np.random.default_rng(32), texts, spans, gap, gap_at)
    order = np.random.default_rng(33).permutation(len(named))
    named = [named[i] for i in order]
    batch = _of_reads("shapes", [r for _, r in named])
    return index, batch, [n for n, _ in named], {M: _expect(index, M, [batch]) for M in (1, 2, 3)}, paths


def _rows(t, p):
    return slice(int(t.base[p]), int(t.base[p + 1]))


def _most_in_one_path_and_strand(texts, read, d):
    """the largest number of windows at Hamming distance d from the read over (path, strand)"""
    most = 0
    for t in texts:
        if t is None or len(t[0]) < len(read):
            continue
        w = np.lib.stride_tricks.sliding_window_view(np.frombuffer(t[0], dtype=np.uint8), len(read))
        for o in (read, _rc(read)):
            most = max(most, int(((w != np.frombuffer(o, dtype=np.uint8)).sum(axis=1) == d).sum()))
    return most


# ---- CPU: the batch holds every class --------------------------------------------------------------------------------------------------

def test_inputs_hold_every_class(case):
    index, batch, names, ts, paths = case
    t = ts[2]
    has = _has_record(batch, index)
    reads = _reads_of(batch)
    cand = {i: (d, kept) for i, d, kept in t.d_star}
    floor = 20
    count = lambda f: sum(1 for i in range(batch.n) if f(i))
    rescued = lambda i: i in cand and cand[i][0] is not None
    cls = lambda i, c: names[i] == c or names[i].startswith(c + "/")
    print({M: x.stats for M, x in ts.items()}, "reads", batch.n, "with a record", int(has.sum()))
    assert batch.n < 4000
    # shifted copies: two or more kept placements in one path and strand
    shifted = {i for i in cand if rescued(i) and names[i].split("/")[0] in ("period16", "period20", "period3", "homopolymer")
               and _most_in_one_path_and_strand(t.texts, reads[i], cand[i][0]) >= 2}
    for c in SHIFTED:
        assert count(lambda i: names[i] == c and i in shifted) >= floor, (c, count(lambda i: names[i] == c and i in shifted))
    assert count(lambda i: i in shifted and cand[i][1] >= 16) >= floor                         # many copies: the long runs
    t3 = {i: d for i, d, kept in ts[3].d_star}
    assert count(lambda i: names[i] == "period16/keep3" and t3.get(i) == 3) >= 10 and count(lambda i: names[i] == "period16/keep3" and rescued(i)) == 0
    assert count(lambda i: names[i] == "period16" and rescued(i)) >= floor                      # over the repeat's edges
    # the text-less path and its neighbour
    assert count(lambda i: names[i] == "gap" and i in cand and not rescued(i)) >= floor
    assert count(lambda i: names[i] == "full" and rescued(i)) >= floor
    for x in ts.values():
        assert not x.depth()[_rows(x, paths["gap"])].any() and not x.alt[_rows(x, paths["gap"])].any()
        assert x.depth()[_rows(x, paths["full"])].any() and x.alt[_rows(x, paths["full"])].any()
    # the short paths: rescued on main only
    assert count(lambda i: names[i] == "short" and rescued(i)) >= floor
    assert count(lambda i: names[i] == "short/p46" and i in cand and not rescued(i)) >= floor
    assert count(lambda i: names[i] == "short/p11" and rescued(i) and cand[i][0] == 2) >= floor
    for p in ("p11", "p46"):
        assert not t.depth()[_rows(t, paths[p])].any() and not t.alt[_rows(t, paths[p])].any()
    assert t.depth()[_rows(t, paths["main"])][:46].all() and t.alt[_rows(t, paths["main"])][:46].any()
    t1 = {i: d for i, d, kept in ts[1].d_star}
    assert count(lambda i: names[i] == "short/fit" and t1.get(i) == 1) >= floor                 # M = 1: the 46-base path filled exactly, and its last 32
    assert ts[1].depth()[_rows(t, paths["p46"])].all() and t.stats["too_short"] >= floor
    # long reads
    for L in LONG:
        assert count(lambda i: len(reads[i]) == L and rescued(i)) >= 8, L
    assert count(lambda i: names[i] == "long" and rescued(i)) >= floor and count(lambda i: names[i] == "long" and i in cand and not rescued(i)) >= floor
    assert count(lambda i: names[i] == "long/pos" and rescued(i)) >= 5 * floor
    assert count(lambda i: names[i] == "long/bubble" and cand.get(i) == (1, 1)) >= floor        # d = 2 on the other path: dropped
    assert count(lambda i: i in cand and len(reads[i]) > 256) >= floor and count(lambda i: rescued(i) and len(reads[i]) > 256) >= floor
    # controls, distances, candidates without a placement
    assert count(lambda i: names[i] == "random" and i in cand and not rescued(i)) >= floor
    assert t.stats["non_acgt"] >= floor and count(lambda i: names[i] == "read N" and not has[i]) >= floor
    for d in (0, 1, 2):
        assert count(lambda i: rescued(i) and cand[i][0] == d) >= floor, d
    for c in ("gap", "short", "random"):
        assert count(lambda i: cls(i, c) and i in cand and not rescued(i)) >= 1, c
    for M, x in ts.items():
        assert 0 < x.stats["rescued"] < x.stats["candidates"] and x.stats["placements"] > x.stats["rescued"], (M, x.stats)


# ---- the device side -------------------------------------------------------------------------------------------------------------------

def _open(index, n_reads, M=2, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 512)
    kw.setdefault("max_batch_reads", max(1024, n_reads))
    al = device.Aligner(index, threshold=THR, **kw)
    al.rescue_enable(M)
    return al


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 3])
def test_every_shape_at_once(case, hip_lib, monkeypatch, M):
    index, batch, names, ts, paths = case
    _stage(monkeypatch, "path_first")
    al = _open(index, batch.n, M)
    try:
        _feed(al, [batch])
        _assert_device(al, ts[M])
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case, hip_lib, monkeypatch, stage):
    index, batch, names, ts, paths = case
    _stage(monkeypatch, stage)
    al = _open(index, batch.n)
    try:
        _feed(al, [batch])
        _assert_device(al, ts[2])
    finally:
        al.close()


@pytest.mark.gpu
def test_pieces_in_flight(case, hip_lib, monkeypatch):
    """five pieces, one of long reads only, three in flight: the tables of the whole batch"""
    index, batch, names, ts, paths = case
    reads = _reads_of(batch)
    long = [r for r, n in zip(reads, names) if n.startswith("long")]
    rest = [r for r, n in zip(reads, names) if not n.startswith("long")]
    cuts = [0, len(rest) // 4, len(rest) // 2, 3 * len(rest) // 4, len(rest)]
    pieces = [_of_reads("piece %d" % i, rest[a:b]) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]
    pieces.insert(2, _of_reads("long", long))
    assert len(pieces) == 5 and min(len(r) for r in long) >= 159 and sum(p.n for p in pieces) == batch.n
    # (a read's records do not depend on its batch: the pieces' candidates are the batch's)
    want = dict(zip(reads, _has_record(batch, index)))
    assert all(want[r] == h for p in pieces for r, h in zip(_reads_of(p), _has_record(p, index)))
    _stage(monkeypatch, "path_first")
    al = _open(index, batch.n, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, pieces) == [0] * 5
        _assert_device(al, ts[2])
    finally:
        al.close()


def _candidates_only(index, l0, n):
    """n reads without a record, of mixed lengths: stretches of a long path with 1 .. 3 substitutions and random reads -> (batch, Tables for M = 2)"""
    rng, pool = np.random.default_rng(34), []
    for k in range(2 * n):
        L = (48, 63, 65, 512, 100, 161, 257, 64)[k % 8]
        x = int(rng.integers(0, len(l0) - L + 1))
        r = _mut(rng, l0[x:x + L], rng.choice(L, 1 + k % 3, replace=False)) if k % 16 < 12 else _seq(rng, L).encode()
        pool.append(_rc(r) if k & 8 else r)
    keep = np.flatnonzero(~_has_record(_of_reads("pool", pool), index))[:n]
    full = _of_reads("full", [pool[i] for i in keep])
    lens = np.diff(full.off.astype(np.int64))
    assert full.n == n and {48, 63, 65, 512} <= set(lens.tolist()) and not _has_record(full, index).any()
    t = _expect(index, 2, [full])
    assert t.stats["candidates"] == n and 100 <= t.stats["rescued"] < n - 100, t.stats
    return full, t


@pytest.mark.gpu
def test_batch_that_fills_the_buffer(case, hip_lib, monkeypatch):
    """max_batch_reads candidates of exactly max_batch_bases bases: every read takes its words of the 2-bit buffer, the last one ends on the
    last base, and none is left out for want of room (the export would fail with GROOT_E_DEVICE)"""
    index, batch, names, ts, paths = case
    n = 1024
    full, t = _candidates_only(index, ts[2].texts[paths["l0"]][0], n)
    lens = np.diff(full.off.astype(np.int64))
    _stage(monkeypatch, "path_first")
    al = _open(index, n, max_batch_reads=n, max_batch_bases=int(full.off[-1]))
    try:
        assert al.params.max_batch_reads == n and al.params.max_batch_bases == int(lens.sum())
        _feed(al, [full])
        assert _assert_device(al, t)["candidates"] == n
    finally:
        al.close()


@pytest.mark.gpu
def test_two_ctxs_sum_over_a_textless_path(case, hip_lib, monkeypatch):
    index, batch, names, ts, paths = case
    t = ts[2]
    reads = _reads_of(batch)
    a, b = _of_reads("a", reads[:batch.n // 2]), _of_reads("b", reads[batch.n // 2:])
    ta, tb = _expect(index, 2, [a]), _expect(index, 2, [b])
    _stage(monkeypatch, "path_first")
    al, al2 = _open(index, batch.n), _open(index, batch.n)
    try:
        _feed(al, [a])
        _feed(al2, [b])
        _assert_device(al, ta)
        _assert_device(al2, tb)
        (d1, a1), (d2, a2) = al.rescue(), al2.rescue()
        assert np.array_equal(d1 + d2, t.depth()) and np.array_equal(a1 + a2, t.alt.astype(np.uint64))
        gap = _rows(t, paths["gap"])
        assert gap.stop - gap.start > 300
        for d, x in ((d1, a1), (d2, a2)):
            assert not d[gap].any() and not x[gap].any() and d[_rows(t, paths["full"])].any()
        s1, s2 = al.rescue_stats(), al2.rescue_stats()
        assert all(s1[k] + s2[k] == t.stats[k] for k in t.stats)
    finally:
        al.close()
        al2.close()
