"""Mismatch rescue of unaligned reads (groot_hip_rescue_*, kernels_rescue.hpp) against a brute force of its definition.

The definition (include/groot_hip.h, "mismatch rescue"), restated:

    M = max mismatches, 1 <= M <= 3.   A = 16 (anchor length in bases).
    Text of path p: the concatenation of its nodes' sequences in Position order, for the paths build_path_tables gives a text
    (non-empty nodes, no gap or overlap, joined by OutEdges); path coordinate x = Position of the path's first node + offset in the text.
    A read r of a batch is a CANDIDATE when: the batch pass is counted (the kCovSkipFlags rule of the other counters), r has NO traversal
    record, every base of r is A/C/G/T (nothing of it on the exception list), and len(r) >= A * (M + 1).
    A PLACEMENT of r is (p, strand, x): the oriented read (r, or its reverse complement for strand = 1) laid ungapped on
    text_p[x .. x + len), entirely inside the text (0 <= x, x + len <= path_len(p)), with no 'N' of the path in the window, and
    Hamming distance d <= M.
    d*(r) = the smallest d over r's placements.  r is RESCUED when it has a placement; its KEPT placements are all those with d = d*
    (every path, both strands, every x).  A placement is counted once, however many blocks anchor it.
    Per kept placement:   rdepth[p][x .. x + len - 1] += 1;   for every mismatching base at path coordinate y:  alt[p][y][b] += 1, b = the
    base the oriented read has there (path strand).
    Stats: candidates, rescued, rescued with d* = 0, kept placements, reads left out as too short / non-ACGT (non-ACGT first).

`Tables` (tests/rescue_def.py) computes that over ALL (path, strand, x) with no anchor, no table and no knowledge of the kernels: every window of every
text is compared with every oriented candidate (the comparison of one window with one read is a sum over one-hot columns, exact in
float32 since no count reaches 2^24).  "Has a record" comes from the CPU oracle's records of the batch.  The index is the seven graphs of
test_counter_edges.py (its builders) plus an eighth with what they lack: a node that starts with an 'N', an 'N' inside a node, a 64-base
reverse-complement palindrome (a tie over both strands) and a one-base bubble A / C (two alleles one substitution apart: placements at
distance 1 and 2 for one read)."""
import numpy as np
import pytest

from groot_amd import device, host
from oracle import oracle_py as O
from test_abundance import _dev_ecs
from test_counter_edges import NP, SEGS, THR, _Batch, _check, _feed, _feed_pipelined, _graph, _of_reads
from test_coverage import STAGES, _stage
from test_path_pass import _gfa, _seq
from rescue_def import A, Tables, _rc, path_texts

LENGTHS = (47, 48, 63, 64, 65, 100, 129, 150)


def _has_record(batch, index):
    return np.bincount(batch.want(index).alns["read_id"].astype(np.int64), minlength=batch.n) > 0


def _expect(index, M, batches):
    t = Tables(index, M)
    for b in batches:
        t.add(_reads_of(b), _has_record(b, index))
    return t


def _reads_of(b):
    s, o = b.seq.tobytes(), b.off.astype(np.int64)
    return [s[o[i]:o[i + 1]] for i in range(b.n)]


def _assert_device(al, t):
    depth, alt = al.rescue()
    want = t.depth()
    assert np.array_equal(depth, want), (np.flatnonzero(depth != want)[:10], depth[depth != want][:10], want[depth != want][:10])
    assert np.array_equal(alt, t.alt.astype(np.uint64)), np.argwhere(alt != t.alt.astype(np.uint64))[:10]
    st = al.rescue_stats()
    print("rescue", st)
    assert {k: st[k] for k in t.stats} == {k: int(x) for k, x in t.stats.items()}, (st, t.stats)
    assert st["text_paths"] == sum(x is not None for x in t.texts)
    assert st["launches"] >= 2 and st["launches"] % 2 == 0, st      # two kernels per pass (a pass that is redone launches them again and returns at once)
    return st


# ---- the index and the reads ------------------------------------------------------------------------------------------------------

def _mut(rng, s, at):
    s = bytearray(s)
    for p in at:
        s[p] = int(rng.choice([c for c in b"ACGT" if c != s[p]]))
    return bytes(s)


def _extra_graph(rng, path):
    """graph 7: U1 . N+U2 . U3 with an 'N' inside . a 64-base palindrome . U5 . (A | C) . U8; its two paths differ in the one bubble base"""
    half = _seq(rng, 32).encode()
    u3 = _seq(rng, 50)
    nodes = {1: _seq(rng, 60), 2: "N" + _seq(rng, 39), 3: u3[:20] + "N" + u3[21:], 4: (half + _rc(half)).decode(), 5: _seq(rng, 60), 6: "A", 7: "C", 8: _seq(rng, 80)}
    edges = [(1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (5, 7), (6, 8), (7, 8)]
    return _gfa(path, nodes, edges, [("q0", [1, 2, 3, 4, 5, 6, 8]), ("q1", [1, 2, 3, 4, 5, 7, 8])])


def _make_reads(rng, texts, M=2):
    """-> [(class name, read)]: stretches of the path texts with 0 .. M + 1 substitutions, and what must be left out"""
    out = []
    seven = [(p, t[0]) for p, t in enumerate(texts[:sum(NP)]) if p in (0, 1, 70, 134, 199, 328, 329, 457)]     # paths of every one of the seven graphs
    q0 = texts[sum(NP)][0]
    draw = lambda t, L: int(rng.integers(1, len(t) - L))

    def stretch(t, x, L, at, strand=None):
        s = _mut(rng, t[x:x + L].replace(b"N", bytes([b"ACGT"[int(rng.integers(4))]])), at)
        return _rc(s) if (len(out) & 1 if strand is None else strand) else s

    for L in LENGTHS:
        for nm in range(M + 2):                                  # 0 .. M + 1 substitutions anywhere: below, at and above the threshold
            for k in range(28):
                p, t = seven[(k + nm) % len(seven)]
                out.append(("len%d" % L if nm else "clean", stretch(t, draw(t, L), L, rng.choice(L, nm, replace=False))))
        for k in range(24):                                      # at both ends of a path, and hanging over its end (one substitution each)
            p, t = seven[k % len(seven)]
            out.append(("x0", stretch(t, 0, L, [L // 2])))
            out.append(("xend", stretch(t, len(t) - L, L, [L // 2])))
            r = stretch(t + _seq(rng, 10).encode(), len(t) - L + 10, L, [L // 2], strand=0)
            out.append(("overhang", r if k & 1 else _rc(r)))
    for L in (100, 129, 150):                                    # a substitution at the first / last base (with one inside: alone it would be clipped
        for k in range(10):                                      # away and aligned), and on both sides of every word and block edge
            p, t = seven[k % len(seven)]
            for at in ([0, 40], [L - 1, 40], [15], [16], [31], [32], [63], [64], [15, 16], [63, 64]):
                out.append(("pos%s" % "/".join(map(str, at)), stretch(t, draw(t, L), L, at, strand=k & 1)))
    for L in (32, 48, 64):                                       # a substitution in every block but one, for every choice of the surviving block:
        for keep in range(L // A):                               # M = 1, 2, 3 substitutions in the shortest read that M admits
            for k in range(30):
                p, t = seven[k % len(seven)]
                at = [A * b + int(rng.integers(A)) for b in range(L // A) if b != keep]
                out.append(("blocks%d/%d" % (L, keep), stretch(t, draw(t, L), L, at)))
    assert q0[150:214] == _rc(q0[150:214])
    for k in range(30):                                          # the palindrome with one substitution: distance 1 on both strands, on q0 and q1
        out.append(("palindrome", _mut(rng, q0[150:214], [int(rng.integers(64))])))
    for k in range(30):                                          # across the bubble base of q0 with one substitution: distance 1 on q0, 2 on q1
        x = 274 - int(rng.integers(20, 60))
        out.append(("two distances", stretch(q0, x, 100 if x + 100 <= len(q0) else 80, [5 + int(rng.integers(10))], strand=k & 1)))
    for k in range(30):                                          # a window with an 'N' of the path (bases 60 and 120 of graph 7's texts), one substitution
        x = (60, 120)[k & 1] - int(rng.integers(1, 47))
        out.append(("path N", stretch(q0, x, 48, [int(rng.integers(48))], strand=k >> 1 & 1)))
    for k in range(30):                                          # a read with an 'N'
        p, t = seven[k % len(seven)]
        r = bytearray(stretch(t, draw(t, 100), 100, [50]))
        r[int(rng.integers(100))] = ord("N")
        out.append(("read N", bytes(r)))
    for k in range(60):                                          # no seed, no anchor
        out.append(("random", _seq(rng, LENGTHS[k % len(LENGTHS)]).encode()))
    return out


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    """(index of the eight graphs, the batch of every class, its class names, Tables for M = 2)"""
    tmp = tmp_path_factory.mktemp("rescue")
    rng = np.random.default_rng(13)
    shared = {name: _seq(rng, 45) for name, _ in SEGS}
    files = [_graph(rng, tmp / ("g%d.gfa" % g), g, shared)[0] for g in range(len(NP))] + [_extra_graph(rng, tmp / "g7.gfa")]
    # (windows of 64 bases: the aligner takes error-free reads of 48 .. 65 bases, so that the batch holds reads it is the record that excludes)
    index = host.Index.from_gfa_files(files, host.index_params(k=7, s=10, w=64))
    texts = path_texts(index)
    assert index.view.n_paths == sum(NP) + 2 and all(t is not None for t in texts)
    named = _make_reads(np.random.default_rng(14), texts)
    order = np.random.default_rng(15).permutation(len(named))
    named = [named[i] for i in order]
    batch = _of_reads("classes", [r for _, r in named])
    return index, batch, [n for n, _ in named], _expect(index, 2, [batch])


# ---- CPU: the batch holds every class, and the brute force is the definition -----------------------------------------------------------

def test_brute_force_on_a_hand_made_case(case):
    """two texts by hand: placements at the ends, a tie, only d* kept, the read's base on the path strand"""
    index = case[0]
    t = Tables(index, 1)
    a = b"ACGTTGCAAGGCTTAACCGGATCAGGTTACAGTCATGCAA"                # 40 bases
    t.texts = [(a, 0), (a[:36] + b"T" + a[37:], 0)] + [None] * (len(t.texts) - 2)     # path 1: one substitution away (a[36] = 'G')
    assert a[36:37] == b"G" and a[19:20] == b"G" and int(t.plen[0]) >= 40 and int(t.plen[1]) >= 40
    t.plen[:2] = 40
    r0 = a[:32]                                                      # exact on both paths at x = 0: a tie, both kept
    r1 = _rc(a[8:19] + b"C" + a[20:40])                              # strand 1, x = 8: 'C' for a[19]: d = 1 on path 0, 2 on path 1 (above M, and above d*)
    t.add([r0, r1, a[:31], a[:16] + b"N" + a[17:33]], [False] * 4)
    assert t.stats == dict(candidates=2, rescued=2, exact=1, placements=3, too_short=1, non_acgt=1)
    d = t.depth()
    b1 = int(t.base[1])
    assert d[:40].tolist() == [1] * 8 + [2] * 24 + [1] * 8 and d[b1:b1 + 40].tolist() == [1] * 32 + [0] * 8
    assert t.alt.sum() == 1 and t.alt[19].tolist() == [0, 1, 0, 0]


def test_inputs_hold_every_class(case):
    index, batch, names, t = case
    has = _has_record(batch, index)
    reads = _reads_of(batch)
    cand = {i: (d, kept) for i, d, kept in t.d_star}
    floor = 20
    count = lambda f: sum(1 for i in range(batch.n) if f(i))
    rescued = lambda i: i in cand and cand[i][0] is not None
    print(t.stats, "reads", batch.n, "with a record", int(has.sum()))
    assert batch.n < 6000
    for L in LENGTHS:
        n = count(lambda i: len(reads[i]) == L and i in cand and not has[i])
        assert (n == 0) if L == 47 else (count(lambda i: len(reads[i]) == L and rescued(i)) >= floor), (L, n)
    assert t.stats["too_short"] >= floor and t.stats["non_acgt"] >= floor
    assert count(lambda i: names[i] == "clean" and has[i] and len(reads[i]) >= 48) >= floor      # error-free reads the aligner took: long enough, and no candidates
    assert count(lambda i: names[i] == "read N" and not has[i]) >= floor
    for cls in ("x0", "xend", "palindrome", "two distances", "blocks48/0", "blocks48/1", "blocks48/2") + tuple(n for n in set(names) if n.startswith("pos")):
        assert count(lambda i: names[i] == cls and rescued(i)) >= (floor if not cls.startswith("pos") else 8), cls
    assert count(lambda i: names[i].startswith("pos") and rescued(i)) >= 10 * floor
    for cls in ("overhang", "path N", "random"):
        assert count(lambda i: names[i] == cls and i in cand and not rescued(i)) >= floor, cls
    for d in (0, 1, 2):                                                                             # below and at the threshold; above it: not rescued
        assert count(lambda i: rescued(i) and cand[i][0] == d) >= floor, d
    assert count(lambda i: names[i].startswith("len") and i in cand and not rescued(i)) >= floor
    assert count(lambda i: rescued(i) and cand[i][1] > 64) >= floor                              # ties over many alleles
    assert count(lambda i: names[i] == "palindrome" and rescued(i) and cand[i][1] == 4) >= floor     # both strands of q0 and q1
    assert count(lambda i: names[i] == "two distances" and rescued(i) and cand[i] == (1, 1)) >= floor


@pytest.mark.parametrize("M", [1, 3])
def test_surviving_blocks_under_the_other_thresholds(case, M):
    """M substitutions, one in every 16-base block but one, in a read of 16 (M + 1) bases: rescued under M, for every choice of the block"""
    index, batch, names, _ = case
    t = _expect(index, M, [batch])
    rescued = {i for i, d, kept in t.d_star if d is not None}
    L = A * (M + 1)
    for keep in range(M + 1):
        n = sum(1 for i in rescued if names[i] == "blocks%d/%d" % (L, keep))
        assert n >= 20, (M, keep, n)
    assert sum(1 for i, d, kept in t.d_star if d == M) >= 20 and t.stats["rescued"] < t.stats["candidates"]


# ---- the device side ---------------------------------------------------------------------------------------------------------------------

def _open(index, batches, M=2, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    al = device.Aligner(index, threshold=THR, max_batch_reads=max(1024, max(b.n for b in batches)), **kw)
    if M:
        al.rescue_enable(M)
    return al


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 3])
def test_every_class_at_once(case, hip_lib, monkeypatch, M):
    index, batch, names, t2 = case
    t = t2 if M == 2 else _expect(index, M, [batch])
    _stage(monkeypatch, "path_first")
    al = _open(index, [batch], M)
    try:
        _feed(al, [batch])
        _assert_device(al, t)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case, hip_lib, monkeypatch, stage, rod):
    index, batch, names, t = case
    _stage(monkeypatch, stage)
    al = _open(index, [batch], results_on_device=rod)
    try:
        _feed(al, [batch])
        _assert_device(al, t)
    finally:
        al.close()


def _plain(x):
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, dict):
        return sorted((_plain(k), _plain(v)) for k, v in x.items())
    return [_plain(v) for v in x] if isinstance(x, (tuple, list)) else x


def _pieces(batch, cuts):
    reads = _reads_of(batch)
    return [_of_reads("piece %d" % i, reads[a:b]) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pipelined_pieces_sum_to_the_batch(case, hip_lib, monkeypatch, small):
    """the batch cut into seven, one piece empty and one of a single read, three in flight -- and the same with GROOT_TEST_SMALL_BUFFERS,
    where every piece is redone at collect and counts once"""
    index, batch, names, t = case
    pieces = _pieces(batch, [0, 700, 700, 701, 1100, 1500, 1900, batch.n])
    assert [p.n for p in pieces][1:3] == [0, 1]
    if small:       # a piece of its own with more records than the small buffers hold (the batch's reads mostly have none): redone for certain
        texts, rng = path_texts(index), np.random.default_rng(16)
        clean = [texts[p][0][x:x + 64] for p, x in zip(rng.choice([0, 70, 134, 199, 329, 457], 300), rng.integers(1, 200, 300))]
        extra = _of_reads("mapped and not", clean + _reads_of(batch)[:150])
        assert int(_has_record(extra, index).sum()) >= 280 and len(extra.want(index).alns) > 1000
        pieces.insert(4, extra)
        t = _expect(index, 2, [batch, extra])
    # (a read's records do not depend on its batch: the pieces' candidates are the batch's)
    assert np.array_equal(np.concatenate([_has_record(p, index) for p in pieces if p.n and p.name != "mapped and not"]), _has_record(batch, index))
    _stage(monkeypatch, "path_first")
    if small:
        monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    al = _open(index, [batch], pipeline_depth=3)
    try:
        assert _feed_pipelined(al, pieces) == [0] * len(pieces)
        st = _assert_device(al, t)
        if small:
            assert st["launches"] > 2 * sum(1 for p in pieces if p.n), st      # (a pass was redone: its kernels ran again, and counted once)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["long", "short", "lower"])
def test_failing_batch(case, hip_lib, monkeypatch, kind):
    """a batch that fails with GROOT_E_NOSPACE is not counted; one that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP is counted
    whole (the bad read has no record: too short, or not A/C/G/T)"""
    index, batch, names, t = case
    good, bad = _pieces(batch, [0, 1100, batch.n])
    reads = _reads_of(bad)
    mid = next(i for i in range(300, bad.n) if len(reads[i]) >= 48 and _has_record(bad, index)[i])
    if kind == "long":
        reads[mid] = reads[mid] * 6                              # (288 bases and more: above the ctx's max_read_len of 256)
        code, counted = -6, []
    elif kind == "short":            # (the oracle refuses a batch with a read below k: the other reads' records stand for it)
        has = np.insert(np.delete(_has_record(bad, index), mid), mid, False)
        reads[mid] = reads[mid][:5]
        code, counted = -7, [(reads, has)]
    else:
        reads[mid] = reads[mid].lower()
        b = _of_reads("lower", reads)
        code, counted = -8, [(reads, _has_record(b, index))]
        assert not counted[0][1][mid]
    want = Tables(index, 2)
    want.add(_reads_of(good), _has_record(good, index))
    for r, h in counted:
        want.add(r, h)
    _stage(monkeypatch, "path_first")
    al = _open(index, [batch])
    try:
        first = _feed(al, [good])
        b = _of_reads(kind, reads)
        al.submit(b.seq, b.off, first_read_id=first)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == code
        _assert_device(al, want)
    finally:
        al.close()


@pytest.mark.gpu
def test_reset_off_and_two_ctxs(case, hip_lib, monkeypatch):
    index, batch, names, t = case
    a, b = _pieces(batch, [0, 2000, batch.n])
    ta, tb = _expect(index, 2, [a]), _expect(index, 2, [b])
    _stage(monkeypatch, "path_first")
    al, al2 = _open(index, [batch]), _open(index, [batch])
    try:
        _feed(al, [b])
        al.rescue_reset()
        _feed(al, [a])
        _assert_device(al, ta)
        _feed(al2, [b])
        _assert_device(al2, tb)
        (d1, a1), (d2, a2) = al.rescue(), al2.rescue()           # the merge of two ctxs is a sum
        assert np.array_equal(d1 + d2, t.depth()) and np.array_equal(a1 + a2, t.alt.astype(np.uint64))
        s1, s2 = al.rescue_stats(), al2.rescue_stats()
        assert all(s1[k] + s2[k] == t.stats[k] for k in t.stats)
        al.rescue_enable(0)                                      # off: nothing is launched, the stats are zero but for the launches so far
        _feed(al, [b])
        st = al.rescue_stats()
        assert st["launches"] == s1["launches"] and all(st[k] == 0 for k in t.stats) and st["text_paths"] == 0, (st, s1)
        with pytest.raises(host.GrootError) as e:
            al.rescue()
        assert e.value.code == -9                                # GROOT_E_STATE
        al.rescue_enable(2)                                      # on again: from zero
        _feed(al, [b])
        assert _assert_device(al, tb)["launches"] >= s1["launches"] + 2
        with pytest.raises(host.GrootError):
            al.rescue_enable(4)
    finally:
        al.close()
        al2.close()


@pytest.mark.gpu
def test_refused_with_assignment_in_either_order(case, hip_lib, monkeypatch):
    index, batch, names, t = case
    _stage(monkeypatch, "path_first")
    alpha = np.full(index.view.n_paths, 1.0 / index.view.n_paths)
    al = _open(index, [batch], M=0)
    try:
        al.assign_enable(alpha)
        with pytest.raises(host.GrootError) as e:
            al.rescue_enable(2)
        assert e.value.code == -10 and "assignment" in str(e.value), e.value      # GROOT_E_UNSUPPORTED
        al.assign_enable(None)
        al.rescue_enable(2)
        with pytest.raises(host.GrootError) as e:
            al.assign_enable(alpha)
        assert e.value.code == -10 and "rescue" in str(e.value), e.value
        _feed(al, [batch])
        _assert_device(al, t)
    finally:
        al.close()


@pytest.mark.gpu
def test_beside_the_other_counters_and_pairing(case, hip_lib, monkeypatch):
    """coverage, shared reads, equivalence classes and assigned coverage on beside it: theirs as without it, and as the oracle's records say;
    with pairing on the mates are rescued one by one"""
    index, batch, names, t = case
    even = _pieces(batch, [0, batch.n & ~1])[0]
    te = _expect(index, 2, [even])
    _stage(monkeypatch, "path_first")
    got = []
    for M in (0, 2):
        al = _open(index, [batch], M)
        try:
            al.coverage_enable(); al.shared_enable(); al.ec_enable(); al.acov_enable()
            _feed(al, [even])
            _check(al, index, [even.want(index)])
            got.append((al.coverage(), al.shared(), _dev_ecs(al), al.acov()))
            if M:
                _assert_device(al, te)
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)
    al = _open(index, [batch])
    try:
        al.ec_enable()
        al.pairs_enable()
        _feed(al, [even])
        _assert_device(al, te)
    finally:
        al.close()
