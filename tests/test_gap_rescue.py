"""Gapped rescue on the device (groot_hip_gap_*, kernels_gap.hpp) against the brute force of its definition (tests/gap_def.py, which
knows nothing of the kernel: no anchors, no table).  The definition (include/groot_hip.h, "gapped rescue") is restated in
tests/test_gap_def.py, which also checks that the inputs used here (tests/gap_case.py) hold every class.  Comparisons are exact: gdepth
as an integer array, events as sorted tuples, stats as integers."""
import ctypes as C

import numpy as np
import pytest

import gap_case
from gap_def import STATS, GapTables
from groot_amd import device, host
from rescue_def import Tables
from test_abundance import _dev_ecs
from test_counter_edges import THR, _check, _feed, _feed_pipelined, _of_reads
from test_coverage import STAGES, _stage
from test_rescue import _has_record, _plain, _reads_of


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    """(index, the batch of every class, its class names, has_record per read, the brute force) and the expectations per (M, G), made once"""
    index, batch, names, has, brute = gap_case.case(tmp_path_factory)
    memo = {}

    def expect(M, G, parts=None):
        """GapTables over [(reads, has_record)]; default: the batch"""
        if parts is not None:
            t = GapTables(index, M, G, brute)
            for r, h in parts:
                t.add(r, h)
            return t
        if (M, G) not in memo:
            memo[M, G] = expect(M, G, [(_reads_of(batch), has)])
        return memo[M, G]

    return index, batch, has, expect


def _events(ev):
    return [tuple(int(e[f]) for f in ("path", "pos", "type", "len", "seq", "reads")) for e in ev]


def _assert_device(al, t):
    gdepth, ev = al.gap()
    assert np.array_equal(gdepth.astype(np.int64), t.gdepth), np.flatnonzero(gdepth.astype(np.int64) != t.gdepth)[:10]
    got, want = _events(ev), t.sorted_events()
    assert got == want, (sorted(set(got) - set(want))[:5], sorted(set(want) - set(got))[:5])
    assert all(int(e["reserved"]) == 0 for e in ev)
    st = al.gap_stats()
    print("gap", st)
    assert {k: st[k] for k in STATS} == t.stats, (st, t.stats)
    assert st["events"] == len(t.events) and st["dropped"] == 0
    return st


def _open(index, n, M=2, G=3, slots=1 << 12, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    al = device.Aligner(index, threshold=THR, max_batch_reads=max(1024, n), **kw)
    if M:
        al.rescue_enable(M)
    if M and G:
        al.gap_enable(G, slots)
    return al


def _pieces(batch, has, cuts):
    reads = _reads_of(batch)
    return [(_of_reads("piece %d" % i, reads[a:b]), has[a:b]) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]


@pytest.mark.gpu
@pytest.mark.parametrize("M,G", [(2, 1), (2, 3), (2, 8), (1, 3), (1, 8)])
def test_every_class_at_once(case, hip_lib, monkeypatch, M, G):
    index, batch, has, expect = case
    _stage(monkeypatch, "path_first")
    al = _open(index, batch.n, M, G)
    try:
        _feed(al, [batch])
        st = _assert_device(al, expect(M, G))
        assert st["launches"] >= 1 and st["event_slots"] == 1 << 12  # (a pass that is redone launches its kernels again, and they return at once)
        assert al.rescue_stats()["launches"] == 2 * st["launches"]   # (the gap kernel's launches are not among rescue's two per pass)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case, hip_lib, monkeypatch, stage, rod):
    index, batch, has, expect = case
    _stage(monkeypatch, stage)
    al = _open(index, batch.n, results_on_device=rod)
    try:
        _feed(al, [batch])
        _assert_device(al, expect(2, 3))
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pipelined_pieces_sum_to_the_batch(case, hip_lib, monkeypatch, small):
    """the batch cut into six, one piece empty and one of a single read, three in flight -- and the same with GROOT_TEST_SMALL_BUFFERS and a
    piece with more records than the small buffers hold, which is redone at collect and counts once"""
    index, batch, has, expect = case
    pieces = _pieces(batch, has, [0, 120, 120, 121, 250, 380, batch.n])
    assert [p.n for p, _ in pieces][1:3] == [0, 1]
    t = expect(2, 3)
    if small:
        from rescue_def import path_texts
        texts, rng = path_texts(index), np.random.default_rng(24)
        clean = [texts[p][0][x:x + 100] for p, x in zip(rng.choice([2, 3, 4, 5], 300), rng.integers(1, 140, 300))]
        extra = _of_reads("mapped and not", clean + _reads_of(batch)[:100])
        eh = _has_record(extra, index)
        assert int(eh.sum()) >= 280 and len(extra.want(index).alns) > 64          # (the small buffers hold 64 records)
        pieces.insert(4, (extra, eh))
        t = expect(2, 3, [(_reads_of(batch), has), (_reads_of(extra), eh)])
    _stage(monkeypatch, "path_first")
    if small:
        monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    al = _open(index, batch.n, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, [p for p, _ in pieces]) == [0] * len(pieces)
        st = _assert_device(al, t)
        if small:
            assert st["launches"] > sum(1 for p, _ in pieces if p.n), st      # (a pass was redone: its kernel ran again, and counted once)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["long", "short", "lower"])
def test_failing_batch(case, hip_lib, monkeypatch, kind):
    """a batch that fails with GROOT_E_NOSPACE is not counted; one that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP is counted whole"""
    index, batch, has, expect = case
    (good, gh), (bad, bh) = _pieces(batch, has, [0, 250, batch.n])
    reads = _reads_of(bad)
    mid = next(i for i in range(50, bad.n) if bh[i])
    parts = [(_reads_of(good), gh)]
    if kind == "long":
        reads[mid] = reads[mid] * 3                              # (288 bases and more: above the ctx's max_read_len of 256)
        code = -6
    elif kind == "short":            # (the oracle refuses a batch with a read below k: the other reads' records stand for it)
        h = bh.copy()
        h[mid] = False
        reads[mid] = reads[mid][:5]
        code = -7
        parts.append((reads, h))
    else:
        reads[mid] = reads[mid].lower()
        code = -8
        h = _has_record(_of_reads("lower", reads), index)
        assert not h[mid]
        parts.append((reads, h))
    want = expect(2, 3, parts)
    _stage(monkeypatch, "path_first")
    al = _open(index, batch.n)
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
def test_event_table_full_and_nearly_full(case, hip_lib, monkeypatch):
    """8 slots: events are dropped, the stats say how many and the export refuses with GROOT_E_NOSPACE, naming event_slots.  The smallest
    power of two that holds the events (load above 1/2, so that probe runs are long and wrap): everything is there"""
    index, batch, has, expect = case
    t = expect(2, 3)
    _stage(monkeypatch, "path_first")
    al = _open(index, batch.n, slots=8)
    try:
        _feed(al, [batch])
        st = al.gap_stats()
        assert st["events"] == 8 and st["dropped"] > 0 and st["event_slots"] == 8, st
        assert st["dropped"] >= len(t.events) - 8 and {k: st[k] for k in STATS} == t.stats
        with pytest.raises(host.GrootError) as e:
            al.gap()
        assert e.value.code == -6 and "event_slots" in str(e.value), e.value
        slots = 1 << (len(t.events) - 1).bit_length()
        assert len(t.events) * 2 > slots
        al.gap_enable(3, slots)                                  # another table: from zero
        _feed(al, [batch])
        assert _assert_device(al, t)["event_slots"] == slots
    finally:
        al.close()


@pytest.mark.gpu
def test_reset_off_on_and_two_ctxs(case, hip_lib, monkeypatch):
    index, batch, has, expect = case
    (a, ah), (b, bh) = _pieces(batch, has, [0, 200, batch.n])
    ta, tb, t = expect(2, 3, [(_reads_of(a), ah)]), expect(2, 3, [(_reads_of(b), bh)]), expect(2, 3)
    _stage(monkeypatch, "path_first")
    al, al2 = _open(index, batch.n), _open(index, batch.n)
    try:
        _feed(al, [b])
        al.gap_reset()
        _feed(al, [a])
        s1 = _assert_device(al, ta)
        assert al.rescue_stats()["candidates"] == batch.n - int(has.sum())      # (gap_reset leaves rescue's tables alone)
        _feed(al2, [b])
        s2 = _assert_device(al2, tb)
        (d1, e1), (d2, e2) = al.gap(), al2.gap()                 # the merge of two ctxs is a sum: gdepth elementwise, events by key
        assert np.array_equal((d1 + d2).astype(np.int64), t.gdepth)
        merged = {}
        for ev in _events(e1) + _events(e2):
            merged[ev[:5]] = merged.get(ev[:5], 0) + ev[5]
        assert merged == t.events
        assert all(s1[k] + s2[k] == t.stats[k] for k in STATS)
        al.rescue_reset()                                        # rescue's reset zeroes the gap tables too: the same reads
        assert all(v == 0 for k, v in al.gap_stats().items() if k not in ("launches", "event_slots"))
        _feed(al, [a])
        _assert_device(al, ta)
        before = al.gap_stats()["launches"]
        al.gap_enable(0)                                         # off: nothing is launched, the stats are zero but for the launches so far
        _feed(al, [b])
        st = al.gap_stats()
        assert st["launches"] == before and all(v == 0 for k, v in st.items() if k != "launches"), st
        with pytest.raises(host.GrootError) as e:
            al.gap()
        assert e.value.code == -9                                # GROOT_E_STATE
        al.gap_enable(3, 1 << 12)                                # on again: from zero
        _feed(al, [b])
        assert _assert_device(al, tb)["launches"] >= before + 1
        al.gap_enable(8, 1 << 12)                                # another G: from zero
        _feed(al, [b])
        _assert_device(al, expect(2, 8, [(_reads_of(b), bh)]))
        al.rescue_enable(1)                                      # another M: rescue's and the gap tables from zero
        _feed(al, [b])
        _assert_device(al, expect(1, 8, [(_reads_of(b), bh)]))
        al.rescue_enable(0)                                      # rescue off: gapped rescue off with it
        assert al.gap_stats()["event_slots"] == 0
        with pytest.raises(host.GrootError) as e:
            al.gap_enable(3)
        assert e.value.code == -9 and "rescue" in str(e.value), e.value
    finally:
        al.close()
        al2.close()


@pytest.mark.gpu
def test_refusals_through_the_abi(case, hip_lib, monkeypatch):
    index, batch, has, expect = case
    _stage(monkeypatch, "path_first")
    al = _open(index, batch.n)
    try:
        for args in ((9, 0), (3, 12), (3, 3)):
            with pytest.raises(host.GrootError) as e:
                al.gap_enable(*args)
            assert e.value.code == -1, (args, e.value)
        _feed(al, [batch])
        t = expect(2, 3)
        L = device.lib()
        gdepth, n = np.zeros(len(t.gdepth), dtype=np.uint64), C.c_uint64(0)
        ev = np.zeros(len(t.events), dtype=device.GAP_EVENT_DTYPE)
        rc = L.groot_hip_gap_export(al._h, gdepth.ctypes.data_as(C.c_void_p), ev.ctypes.data_as(C.c_void_p), C.c_uint64(len(ev) - 1), C.byref(n))
        assert rc == -1 and n.value == len(t.events)             # cap below the number of distinct events: GROOT_E_INVALID, with n set
        al.submit(batch.seq, batch.off, first_read_id=batch.n)
        with pytest.raises(host.GrootError) as e:                # something is in flight
            al.gap_enable(2)
        assert e.value.code == -9
        al.wait()
    finally:
        al.close()


@pytest.mark.gpu
def test_beside_rescue_and_the_other_counters(case, hip_lib, monkeypatch):
    """rescue, coverage, shared reads, equivalence classes and assigned coverage beside it: theirs as in a run without gapped rescue"""
    index, batch, has, expect = case
    _stage(monkeypatch, "path_first")
    got = []
    for G in (0, 3):
        al = _open(index, batch.n, 2, G)
        try:
            al.coverage_enable(); al.shared_enable(); al.ec_enable(); al.acov_enable()
            _feed(al, [batch])
            _check(al, index, [batch.want(index)])
            got.append((al.rescue(), al.rescue_stats(), al.coverage(), al.shared(), _dev_ecs(al), al.acov()))
            if G:
                _assert_device(al, expect(2, 3))
            else:
                assert al.gap_stats()["launches"] == 0
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)
    r = Tables(index, 2)                                         # ... and rescue's are the brute force's
    r.add(_reads_of(batch), has)
    assert np.array_equal(got[1][0][0], r.depth()) and np.array_equal(got[1][0][1], r.alt.astype(np.uint64))
