"""Gapped rescue (kernels_gap.hpp) at the shapes tests/test_gap_rescue.py does not reach, against the same brute force (tests/gap_def.py):

    repeats         W16 x 8 and W20 x 7, longer than the read: every block in front of the gap has one key with 6 to 8 occurrences in one
                    path, and the copies of the read one period to the left and to the right are kept placements of their own (the count-once
                    rule of sweep 2); (ACG) x 30 and A x 72 with a gap of one whole period, where k* left-aligns onto the repeat's start
                    or onto A; poly-A, poly-T and poly-G blocks (keys 0, 0xAAAAAAAA, 0xFFFFFFFF) as the only clean block of a read;
    short paths     one of 72 bases and one of 81 that an INS read of more bases, or a DEL read of fewer, fills exactly, and that a read
                    one base longer does not lie on; the paths of 11 and 46 bases of tests/test_rescue_shapes.py;
    a text-less path  in the middle of the index: it owns path_len + 1 slots of the device tables, and the export turns slots back into
                    (path, pos) behind it;
    long reads      159 .. 512 bases (5 .. 16 words): the cut on and beside word edges, in the last word, at kmax and at A; INS with len - g
                    a multiple of 32 (one word fewer than the read has); inserted bases over a word edge of the read;
    M = 3           96 bases, six blocks, of which the inserted bases spoil two and the substitutions three;
    a full hand-over list   exactly max_batch_reads reads, every one a gap candidate.

The index and the reads are in tests/gap_shapes_case.py.  The expectation comes from gap_def.Brute / gap_def.GapTables (m_max = 3),
rescue_def.Tables and the oracle's records (test_rescue._has_record) only.  Every comparison is exact."""
import numpy as np
import pytest

import gap_shapes_case
from gap_def import DEL, INS, GapTables
from gap_shapes_case import INS_WORDS, PATHS
from groot_amd import device
from rescue_def import A, _rc, path_texts
from test_abundance import _dev_ecs
from test_counter_edges import THR, _feed, _feed_pipelined, _of_reads
from test_coverage import STAGES, _stage
from test_gap_rescue import _assert_device, _open, _pieces
from test_rescue import _has_record, _reads_of
from test_rescue_shapes import LONG

MG = [(1, 1), (1, 8), (2, 3), (2, 8), (3, 3), (3, 8)]
POLY = {"polyA": 0, "polyT": 0xAAAAAAAA, "polyG": 0xFFFFFFFF}        # the 2-bit code of the kernels: A C T G = 0 1 2 3
_CODE = {c: i for i, c in enumerate(b"ACTG")}


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    """(index, batch, class names, has_record, expect(M, G[, parts]) -> GapTables, {path name: global path})"""
    index, batch, names, has, brute, paths = gap_shapes_case.case(tmp_path_factory)
    memo = {}

    def expect(M, G, parts=None):
        if parts is not None:
            t = GapTables(index, M, G, brute)
            for r, h in parts:
                t.add(r, h)
            return t
        if (M, G) not in memo:
            memo[M, G] = expect(M, G, [(_reads_of(batch), has)])
        return memo[M, G]

    return index, batch, names, has, expect, paths


def _rows(t, p):
    return slice(int(t.base[p]), int(t.base[p + 1]))


def _reaching(text, read, placement):
    """the (block, hypothesis, key) that reach the placement by the definition's anchor argument: the block of the oriented read equals the
    text on the diagonal in front of the gap (0) or behind it (1), and lies in the window"""
    p, strand, x, typ, g, d, k = placement
    R = read if strand == 0 else _rc(read)
    wlen = len(R) + g if typ == DEL else len(R) - g
    out = []
    for i in range(len(R) // A):
        for h, at in ((0, x + A * i), (1, x + A * i + (g if typ == DEL else -g))):
            if at >= x and at + A <= x + wlen and text[at:at + A] == R[A * i:A * i + A]:
                out.append((i, h, sum(_CODE[c] << (2 * j) for j, c in enumerate(R[A * i:A * i + A]))))
    return out


# ---- CPU: the index is what the module says, the batch holds every class ---------------------------------------------------------------

def test_inputs_hold_every_class(case):
    index, batch, names, has, expect, paths = case
    texts = path_texts(index)
    plen = index.arrays["path_len"].astype(np.int64)
    assert [t is None for t in texts] == [n == "gap" for n in PATHS] and 0 < paths["gap"] < len(PATHS) - 1
    assert all(t[1] == 0 and len(t[0]) == int(plen[p]) for p, t in enumerate(texts) if t is not None)
    assert [int(plen[paths[n]]) for n in ("m300", "p72", "p81", "p46", "p11")] == [300, 72, 81, 46, 11]
    m300, p72, p81 = (texts[paths[n]][0] for n in ("m300", "p72", "p81"))
    assert m300[:40] == p72[:40] == p81[:40] and all(a != b for a, b in zip(p72[40:], m300[40:])) and all(a != b for a, b in zip(p81[40:], m300[40:]))
    assert sum(len(t[0]) for t in texts if t is not None) <= 6000 and batch.n <= 900
    reads = _reads_of(batch)
    ts = {mg: expect(*mg) for mg in MG}
    cand = {mg: {i: (e, kept) for i, e, kept in t.per_read} for mg, t in ts.items()}
    print({mg: t.stats for mg, t in ts.items()}, "reads", batch.n, "with a record", int(has.sum()), "events", {mg: len(t.events) for mg, t in ts.items()})
    count = lambda f: sum(1 for i in range(batch.n) if f(i))
    cls = lambda i, c: names[i] == c or names[i].startswith(c + "/")

    def rescued(i, mg=(2, 8)):
        return i in cand[mg] and cand[mg][i][0] is not None

    def kept(i, mg=(2, 8)):
        return cand[mg][i][1] if rescued(i, mg) else []

    def copies(i, mg):
        """the most kept placements in one (path, strand, type, g)"""
        n = {}
        for x in kept(i, mg):
            n[x[0], x[1], x[3], x[4]] = n.get((x[0], x[1], x[3], x[4]), 0) + 1
        return max(n.values(), default=0)

    both = lambda f: count(lambda i: f(i) and any(x[1] == 0 for x in kept(i, (3, 8)))) >= 1 and count(lambda i: f(i) and any(x[1] == 1 for x in kept(i, (3, 8)))) >= 1
    # repeats longer than the read: shifted copies, and every `keep`
    for mg in MG:                                                # (four copies need a window of at most 80 bases: an INS read of 80, which M = 3 leaves out as too short)
        n2, n4 = (count(lambda i: (cls(i, "rep16") or cls(i, "rep20")) and copies(i, mg) >= n) for n in (2, 4))
        print("shifted copies", mg, n2, n4)
        assert n2 >= 20 and (n4 >= 10 or mg[0] == 3 or mg[1] < 3), (mg, n2, n4)
    for name in ("rep16", "rep20"):
        for k in range(4):
            mg = (max(k, 1), 8 if k < 2 else 3)
            assert count(lambda i: names[i] == "%s/keep%d" % (name, k) and rescued(i, mg) and copies(i, mg) >= 2) >= 3, (name, k)
            if k > 1:
                assert count(lambda i: names[i] == "%s/keep%d" % (name, k) and rescued(i, (k - 1, 8))) == 0, (name, k)
    assert both(lambda i: cls(i, "rep16")) and both(lambda i: cls(i, "rep20"))
    # a gap of one whole period: k* on the repeat's start, or clamped to A
    for c in ("whole period/ACG", "whole period/A"):
        assert count(lambda i: names[i] == c and rescued(i, (2, 3))) >= 10, c
        assert count(lambda i: names[i] == c and any(x[6] == A and x[5] == 0 for x in kept(i, (2, 3)))) >= 3, c
        assert count(lambda i: names[i] == c and any(x[6] > A and x[5] == 0 for x in kept(i, (2, 3)))) >= 3, c
    # one clean block, and its key is a homopolymer's
    for c, key in POLY.items():
        n = count(lambda i: names[i] == c and rescued(i, (2, 3)) and all({b[2] for b in _reaching(texts[x[0]][0], reads[i], x)} == {key} for x in kept(i, (2, 3))))
        print(c, n)
        assert n >= 5, (c, n)
        assert count(lambda i: names[i] == c and rescued(i, (1, 8))) == 0
    # the short paths
    short = [paths[n] for n in ("p72", "p81", "p46", "p11")]
    for typ in (DEL, INS):
        c = "DI"[typ]
        fills = lambda i, mg: any(x[0] in short and x[2] == 0 and (len(reads[i]) + x[4] if x[3] == DEL else len(reads[i]) - x[4]) == plen[x[0]] for x in kept(i, mg))
        assert count(lambda i: names[i] == "fit/" + c and fills(i, (1, 8))) >= 10, c
        assert count(lambda i: names[i] == "fit/" + c and fills(i, (2, 8))) >= 1, c
        over = [i for i in range(batch.n) if names[i] == "over/" + c]
        assert len(over) >= 10 and all(i in cand[1, 8] for i in over)
        assert not any(x[0] in short for i in over for x in ts[1, 8].brute.placements(reads[i]))
    assert count(lambda i: names[i] == "short/main" and rescued(i, (1, 8))) >= 20
    assert not any(x[0] in short for i in range(batch.n) if names[i] == "short/main" for mg in MG for x in kept(i, mg))
    assert ts[1, 8].gdepth[_rows(ts[1, 8], paths["p72"])].all() and ts[1, 8].gdepth[_rows(ts[1, 8], paths["p81"])].all()
    for n in ("p46", "p11"):
        assert not any(t.gdepth[_rows(t, paths[n])].any() for t in ts.values())
    # the text-less path and the one behind it
    assert count(lambda i: names[i] == "gap" and i in cand[3, 8] and not rescued(i, (3, 8))) >= 10
    assert count(lambda i: names[i] == "full" and rescued(i, (2, 8)) and all(x[0] == paths["full"] for x in kept(i))) >= 20
    for t in ts.values():
        assert not t.gdepth[_rows(t, paths["gap"])].any() and all(e[0] != paths["gap"] for e in t.events)
        assert t.gdepth[_rows(t, paths["full"])].any() and any(e[0] == paths["full"] for e in t.events)
    # long reads
    lens = np.array([len(r) for r in reads])
    for L in LONG:
        assert count(lambda i: cls(i, "long") and lens[i] == L and rescued(i)) >= 4, L
        assert count(lambda i: names[i] == "random" and lens[i] == L and i in cand[3, 8] and not rescued(i, (3, 8))) >= 1, L
    last_word = lambda i, x: x[6] >= 32 * (((lens[i] if x[3] == DEL else lens[i] - x[4]) + 31) // 32 - 1)
    n = count(lambda i: cls(i, "long") and any(last_word(i, x) for x in kept(i)))
    print("k* in the last word", n)
    assert n >= 20
    assert count(lambda i: cls(i, "long") and any(x[6] == (lens[i] if x[3] == DEL else lens[i] - x[4]) - A for x in kept(i))) >= 10          # k* = kmax
    assert count(lambda i: cls(i, "long") and any(x[6] == A for x in kept(i))) >= 10
    assert count(lambda i: cls(i, "long") and any(x[6] % 32 == 0 for x in kept(i))) >= 20 and count(lambda i: cls(i, "long") and any(x[6] % 32 == 31 for x in kept(i))) >= 10
    for L, g in INS_WORDS:
        assert count(lambda i: names[i] == "long/ins words" and lens[i] == L and any(x[3] == INS and x[4] == g and (L - g) % 32 == 0 for x in kept(i))) >= 1 + (g <= 3), (L, g)
    assert count(lambda i: names[i] == "long/ins straddle" and any(x[3] == INS and x[6] // 32 < (x[6] + x[4] - 1) // 32 for x in kept(i))) >= 8
    assert count(lambda i: cls(i, "long") and any(x[5] == 2 for x in kept(i))) >= 20 and count(lambda i: cls(i, "long") and any(x[5] == 0 for x in kept(i))) >= 20
    # M = 3
    for c in ("m3/ins", "m3/del"):
        assert count(lambda i: names[i] == c and rescued(i, (3, 3)) and cand[3, 3][i][0] == 3 + kept(i, (3, 3))[0][4]) >= 10, c
        assert count(lambda i: names[i] == c and rescued(i, (2, 8))) == 0, c
    assert count(lambda i: names[i] == "m3/ins" and rescued(i, (3, 3)) and all(len({b[0] for b in _reaching(texts[x[0]][0], reads[i], x)}) == 1 for x in kept(i, (3, 3)))) >= 10      # one clean block
    assert count(lambda i: names[i] == "m3/len95" and i in cand[2, 8] and i not in cand[3, 8]) >= 10 and ts[3, 8].stats["too_short"] >= 10
    assert count(lambda i: names[i] == "m3/len95" and rescued(i, (2, 3))) >= 5
    assert count(lambda i: names[i] == "m3/d4" and i in cand[3, 8] and not rescued(i, (3, 8))) >= 10
    # flush with the start of the first path and with the end of the last
    first, last = 0, len(PATHS) - 1
    assert count(lambda i: names[i] == "flush first" and any(x[:5] == (first, x[1], 0, DEL, 8) for x in kept(i))) >= 5
    assert count(lambda i: names[i] == "flush last" and any(x[0] == last and x[3] == DEL and x[4] == 8 and x[2] + lens[i] + 8 == plen[last] for x in kept(i))) >= 5
    # controls
    assert count(lambda i: names[i] == "clean" and has[i]) >= 10
    assert count(lambda i: names[i] == "ungapped" and not has[i] and not any(i in c for c in cand.values())) >= 10
    for mg, t in ts.items():
        assert 0 < t.stats["rescued"] < t.stats["candidates"] and t.stats["placements"] > t.stats["rescued"], (mg, t.stats)
        assert t.stats["del_placements"] >= 50 and t.stats["ins_placements"] >= 50, (mg, t.stats)
    assert ts[1, 8].stats["too_short"] == 0 < ts[2, 8].stats["too_short"] < ts[3, 8].stats["too_short"]


# ---- the device side -------------------------------------------------------------------------------------------------------------------

def _slots(t):
    """1 << 13, or the next power of two above the events"""
    return max(1 << 13, 1 << len(t.events).bit_length())


@pytest.mark.gpu
@pytest.mark.parametrize("M,G", MG)
def test_every_shape_at_once(case, hip_lib, monkeypatch, M, G):
    index, batch, names, has, expect, paths = case
    t = expect(M, G)
    _stage(monkeypatch, "path_first")
    al = _open(index, batch.n, M, G, slots=_slots(t), max_read_len=512)
    try:
        _feed(al, [batch])
        _assert_device(al, t)
        gdepth, ev = al.gap()
        assert not gdepth[_rows(t, paths["gap"])].any() and all(int(e["path"]) != paths["gap"] for e in ev)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case, hip_lib, monkeypatch, stage, rod):
    index, batch, names, has, expect, paths = case
    t = expect(3, 8)
    _stage(monkeypatch, stage)
    al = _open(index, batch.n, 3, 8, slots=_slots(t), max_read_len=512, results_on_device=rod)
    try:
        _feed(al, [batch])
        _assert_device(al, t)
    finally:
        al.close()


@pytest.mark.gpu
def test_pipelined_pieces_sum_to_the_batch(case, hip_lib, monkeypatch):
    """the batch in seven pieces, three in flight: one empty, one of a single 512-base read, one of the reads of one repeat only"""
    index, batch, names, has, expect, paths = case
    reads = _reads_of(batch)
    one = next(i for i in range(batch.n) if len(reads[i]) == 512 and names[i] == "long")
    rep = [i for i in range(batch.n) if names[i].startswith("rep16/")]
    rest = [i for i in range(batch.n) if i != one and not names[i].startswith("rep16/")]
    q = len(rest) // 4
    order = rest[:q] + [one] + rest[q:2 * q] + rep + rest[2 * q:]
    cuts = [0, q, q, q + 1, 2 * q + 1, 2 * q + 1 + len(rep), 3 * q + 1 + len(rep), batch.n]
    pieces = _pieces(_of_reads("reordered", [reads[i] for i in order]), has[order], cuts)
    assert [p.n for p, _ in pieces][1:3] == [0, 1] and len(rep) >= 60 and sum(p.n for p, _ in pieces) == batch.n and len(pieces) == 7
    assert len(_reads_of(pieces[2][0])[0]) == 512 and _reads_of(pieces[4][0]) == [reads[i] for i in rep]
    # (a read's records do not depend on its batch: the pieces' candidates are the batch's)
    assert all(np.array_equal(_has_record(p, index), h) for p, h in pieces if p.n)
    t = expect(2, 8)
    _stage(monkeypatch, "path_first")
    al = _open(index, batch.n, 2, 8, slots=_slots(t), max_read_len=512, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, [p for p, _ in pieces]) == [0] * len(pieces)
        _assert_device(al, t)
    finally:
        al.close()


@pytest.mark.gpu
def test_full_hand_over_list(case, hip_lib, monkeypatch):
    """a batch of exactly max_batch_reads reads, every one a gap candidate with a block in the table: the hand-over list is full to its last
    entry; and the same batch again in a ctx whose max_batch_bases are exactly its bases"""
    index, batch, names, has, expect, paths = case
    M, G = 2, 8
    whole = expect(M, G)
    reads = _reads_of(batch)
    ids = [i for i, e, kept in whole.per_read if names[i] != "random"]
    full = _of_reads("gap candidates", [reads[i] for i in ids])
    n = full.n
    t = expect(M, G, [(_reads_of(full), has[ids])])
    assert t.stats["candidates"] == n >= 500 and 100 <= t.stats["rescued"] <= n - 100 and t.stats["too_short"] == 0, t.stats
    assert np.array_equal(_has_record(full, index), has[ids])
    _stage(monkeypatch, "path_first")
    for kw in ({}, {"max_batch_bases": int(full.off[-1])}):
        al = device.Aligner(index, threshold=THR, max_batch_reads=n, max_read_len=512, memo_budget_mb=device.MEMO_OFF, **kw)
        try:
            assert al.params.max_batch_reads == n and (not kw or al.params.max_batch_bases == int(full.off[-1]))
            al.rescue_enable(M)
            al.gap_enable(G, _slots(t))
            _feed(al, [full])
            assert _assert_device(al, t)["candidates"] == n
        finally:
            al.close()


@pytest.mark.gpu
def test_beside_rescued_reads_in_the_classes(case, hip_lib, monkeypatch):
    """with ec_enable and rescue_ec_enable the hand-over is rescue_count_ec_kernel<true>'s: the gap tables are the brute force's, and the
    classes are those of a run with gapped rescue off"""
    index, batch, names, has, expect, paths = case
    t = expect(2, 8)
    _stage(monkeypatch, "path_first")
    got = []
    for G in (0, 8):
        al = _open(index, batch.n, 2, 0, max_read_len=512)
        try:
            al.ec_enable()
            al.rescue_ec_enable()
            if G:
                al.gap_enable(G, _slots(t))
            _feed(al, [batch])
            got.append((_dev_ecs(al), al.rescue_ec_stats()["reads"], al.rescue_stats()))
            if G:
                _assert_device(al, t)
            else:
                assert al.gap_stats()["launches"] == 0
        finally:
            al.close()
    assert got[0] == got[1] and got[0][1] > 0 and len(got[0][0]) > 1


@pytest.mark.gpu
def test_event_table_nearly_full(case, hip_lib, monkeypatch):
    """the smallest power of two that holds the events: the load is above 1/2, probe runs are long and wrap, and everything is there"""
    index, batch, names, has, expect, paths = case
    t = expect(3, 8)
    slots = 1 << (len(t.events) - 1).bit_length()
    assert len(t.events) * 2 > slots >= len(t.events)
    _stage(monkeypatch, "path_first")
    al = _open(index, batch.n, 3, 8, slots=slots, max_read_len=512)
    try:
        _feed(al, [batch])
        st = _assert_device(al, t)
        assert st["event_slots"] == slots and st["dropped"] == 0 and st["events"] == len(t.events)
    finally:
        al.close()
