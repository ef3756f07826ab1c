"""Gapped records on the device (groot_hip_gap_rec_*, kernels_gap_rec.hpp) against the brute force of their definition
(tests/gap_records_def.py; include/groot_hip.h, "gapped records"): the list a batch hands out equals the definition's record for record,
order included.  The case is that of tests/test_gap_records_def.py, which also holds the floor of every class of record."""
import numpy as np
import pytest

from gap_records_case import the_case
from gap_records_def import RECORD_DTYPE, plain
from groot_amd import device, host
from test_abundance import _dev_ecs
from test_counter_edges import THR, _feed, _of_reads
from test_coverage import STAGES, _stage
from test_rescue import _has_record, _plain

PARTS = ["classes", "shapes", "pal"]
SLOTS = 1 << 14


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return the_case(tmp_path_factory)


def _open(part, M=2, G=3, slots=SLOTS, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", part.max_read_len)
    al = device.Aligner(part.index, threshold=THR, max_batch_reads=max(1024, part.batch.n), **kw)
    if M:
        al.rescue_enable(M)
    if M and G:
        al.gap_enable(G, 1 << 13)
    if M and G and slots:
        al.gap_rec_enable(slots)
    return al


def _same(got, want):
    assert got.dtype == RECORD_DTYPE == device.GAP_RECORD_DTYPE and got.dtype.itemsize == 24
    if not np.array_equal(got, want):
        n = min(len(got), len(want))
        bad = np.flatnonzero(got[:n] != want[:n])[:5]
        raise AssertionError("device %d records, definition %d; first differences (device, definition): %s"
                             % (len(got), len(want), [(plain(got[i:i + 1]), plain(want[i:i + 1])) for i in bad]))


def _one_batch(al, b, first=0):
    al.submit(b.seq, b.off, first_read_id=first)
    c = al.wait()
    assert c["received"] == b.n
    return al.gap_records()


@pytest.mark.gpu
@pytest.mark.parametrize("M,G", [(2, 1), (2, 3), (2, 8), (1, 3), (3, 8)])
@pytest.mark.parametrize("name", PARTS)
def test_every_class_at_once(case, hip_lib, monkeypatch, name, M, G):
    part = case[name]
    _stage(monkeypatch, "path_first")
    al = _open(part, M, G)
    try:
        want = part.records(M, G)
        _same(_one_batch(al, part.batch), want)
        st = al.gap_rec_stats()
        print("gapped records", name, M, G, st)
        launches = st.pop("launches")
        assert st == dict(records=len(want), reads=len(np.unique(want["read"])), failed=0, slots=SLOTS), st
        assert launches >= 2 and launches % 2 == 0      # the scan and the emit kernel per pass (a pass that is redone launches them again: they return at once)
        gs = al.gap_stats()
        assert gs["placements"] == len(want) and gs["rescued"] == st["reads"]
        assert gs["del_placements"] == int((want["type"] == 0).sum()) and gs["ins_placements"] == int((want["type"] == 1).sum())
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case, hip_lib, monkeypatch, stage, rod):
    part = case["classes"]
    _stage(monkeypatch, stage)
    al = _open(part, 2, 8, results_on_device=rod)
    try:
        _same(_one_batch(al, part.batch), part.records(2, 8))
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("beside", ["records", "classes", "both"])
def test_beside_the_rescued_records_and_the_classes(case, hip_lib, monkeypatch, beside):
    """rescue_gap_rec_kernel behind every instance of the count kernel that hands gap candidates on: the list is the same, and the rescued
    records, the classes, rescue's tables and gapped rescue's gdepth / events / stats are what they are without the gapped records"""
    part = case["classes"]
    _stage(monkeypatch, "path_first")
    got = []
    for slots in (0, SLOTS):
        al = _open(part, 2, 3, slots=slots)
        try:
            if beside != "records":
                al.ec_enable()
                al.rescue_ec_enable()
            if beside != "classes":
                al.rescue_rec_enable(1 << 16)
            if slots:
                _same(_one_batch(al, part.batch), part.records(2, 3))
            else:
                _feed(al, [part.batch])
            rr = al.rescue_records() if beside != "classes" and slots else None
            gs = {k: v for k, v in al.gap_stats().items()}
            got.append((al.rescue(), al.rescue_stats(), _dev_ecs(al) if beside != "records" else None, al.rescue_ec_stats()["reads"] if beside != "records" else None,
                        al.gap(), gs))
            if rr is not None:
                assert len(rr) == al.rescue_stats()["placements"] > 0
                assert not set(rr["read"].tolist()) & set(part.records(2, 3)["read"].tolist())      # a read has records of one kind
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)


def _pieces_pipelined(al, pieces, depth=3):
    """`depth` batches in flight, collected oldest first -> (status, records) of every batch"""
    out, pending, first = [], 0, 0

    def collect():
        r = al.collect(check=False)
        out.append((r["status"], al.gap_records(r["ticket"])))
        al.release(r["ticket"])

    for b in pieces:
        if pending == depth:
            collect()
            pending -= 1
        al.submit(b.seq, b.off, first_read_id=first)
        pending += 1
        first += b.n
    for _ in range(pending):
        collect()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pipelined_pieces_concatenate_to_the_batch(case, hip_lib, monkeypatch, small):
    """the batch cut into six, one piece empty and one of a single read, three in flight: every piece hands out the batch's records of its
    reads with batch-relative `read` -- and the same with GROOT_TEST_SMALL_BUFFERS and a piece that is redone at collect for certain, which
    yields the records of its redo, once"""
    part = case["classes"]
    cuts = [0, 150, 150, 151, 300, 450, part.batch.n]
    pieces = [part.piece(a, b) for a, b in zip(cuts, cuts[1:])]
    want = [part.records_of(2, 3, a, b) for a, b in zip(cuts, cuts[1:])]
    assert [p.n for p in pieces][1:3] == [0, 1] and len(want[1]) == 0 and sum(len(w) for w in want) == len(part.records(2, 3))
    if small:       # error-free reads with more records than the small buffers hold, and reads of the batch behind them
        from rescue_def import path_texts
        texts, rng = path_texts(part.index), np.random.default_rng(24)
        clean = [texts[p][0][x:x + 100] for p, x in zip(rng.choice([2, 3, 4, 5], 300), rng.integers(1, 140, 300))]
        extra = _of_reads("mapped and not", clean + part.reads[:120])
        assert int(_has_record(extra, part.index).sum()) >= 280 and len(extra.want(part.index).alns) > 64
        w = part.records_of(2, 3, 0, 120)
        w["read"] += 300
        assert len(w) >= 20
        pieces.insert(4, extra)
        want.insert(4, w)
        monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    _stage(monkeypatch, "path_first")
    al = _open(part, pipeline_depth=3)
    try:
        got = _pieces_pipelined(al, pieces)
        assert [s for s, _ in got] == [0] * len(pieces)
        for (_, g), w in zip(got, want):
            _same(g, w)
        st = al.gap_rec_stats()
        assert st["records"] == sum(len(w) for w in want) and st["failed"] == 0, st
        if small:
            assert st["launches"] > 2 * sum(1 for p in pieces if p.n), st      # (a pass was redone: its kernels ran again, and it counted once)
        else:
            assert st["launches"] >= 2 * sum(1 for p in pieces if p.n) and st["launches"] % 2 == 0, st
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["long", "short", "lower"])
def test_failing_batch(case, hip_lib, monkeypatch, kind):
    """a batch that fails with GROOT_E_NOSPACE yields no record; one that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP yields all of
    them (the bad read has no record and is no candidate: too short, or not A/C/G/T), and the batch behind either is clean"""
    part = case["classes"]
    lo = 300
    reads = list(part.reads[lo:])
    has = part.has[lo:]
    mid = next(i for i in range(100, len(reads)) if has[i])
    want = part.records_of(2, 3, lo, part.batch.n)
    if kind == "long":
        reads[mid] = reads[mid] * 3                              # (288 bases and more: above the ctx's max_read_len of 256)
        code, want = -6, want[:0]
    elif kind == "short":
        reads[mid] = reads[mid][:5]
        code = -7
    else:
        reads[mid] = reads[mid].lower()
        code = -8
    _stage(monkeypatch, "path_first")
    al = _open(part)
    try:
        b = _of_reads(kind, reads)
        al.submit(b.seq, b.off)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == code
        _same(al.gap_records(), want)
        _same(_one_batch(al, part.piece(0, lo)), part.records_of(2, 3, 0, lo))
        assert al.gap_rec_stats()["records"] == len(want) + len(part.records_of(2, 3, 0, lo))
    finally:
        al.close()


@pytest.mark.gpu
def test_room(case, hip_lib, monkeypatch):
    """slots_per_batch exactly the batch's total passes; one less fails the batch with GROOT_E_NOSPACE and a message that names the
    capacity, its other results stay readable, the rescued records included, the stats count it, and the next batch is clean"""
    part = case["classes"]
    want = part.records(2, 3)
    small = part.piece(0, 300)
    _stage(monkeypatch, "path_first")
    al = _open(part, slots=len(want))
    try:
        al.rescue_rec_enable(1 << 16)
        _same(_one_batch(al, part.batch), want)
        rr = al.rescue_records()
        n_travs, launches = len(al.travs()[0]), al.gap_rec_stats()["launches"]
        assert len(rr) > 0
        al.gap_rec_enable(len(want) - 1)
        assert al.gap_rec_stats() == dict(records=0, reads=0, failed=0, slots=len(want) - 1, launches=launches)      # another capacity: from zero
        al.submit(part.batch.seq, part.batch.off)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == -6 and "slots_per_batch" in str(e.value) and "groot_hip_gap_rec_enable" in str(e.value), e.value
        assert str(len(want) - 1) in str(e.value) and str(len(want)) in str(e.value), e.value
        assert len(al.gap_records()) == 0
        assert len(al.travs()[0]) == n_travs > 0 and np.array_equal(al.rescue_records(), rr)
        st = al.gap_rec_stats()
        assert st["failed"] == 1 and st["records"] == 0, st
        _same(_one_batch(al, small, first=part.batch.n), part.records_of(2, 3, 0, 300))
        st = al.gap_rec_stats()
        assert st["failed"] == 1 and st["records"] == len(part.records_of(2, 3, 0, 300)), st
    finally:
        al.close()


@pytest.mark.gpu
def test_off_on_and_the_enable_rules(case, hip_lib, monkeypatch):
    part = case["classes"]
    want = part.records_of(2, 3, 0, 300)
    small = part.piece(0, 300)
    _stage(monkeypatch, "path_first")
    al = _open(part, M=2, G=0, slots=0)
    try:
        with pytest.raises(host.GrootError) as e:                # needs gapped rescue
            al.gap_rec_enable(1000)
        assert e.value.code == -9 and "gapped rescue" in str(e.value), e.value
        al.gap_enable(3, 1 << 13)
        with pytest.raises(host.GrootError) as e:                # beyond 2^40 bytes
            al.gap_rec_enable((1 << 40) // 24 + 1)
        assert e.value.code == -1 and "2^40" in str(e.value), e.value
        assert al.gap_rec_stats() == dict(records=0, reads=0, failed=0, slots=0, launches=0)
        _feed(al, [small])                                       # off: nothing is launched, nothing is handed out
        assert al.gap_rec_stats()["launches"] == 0
        with pytest.raises(host.GrootError) as e:
            al.gap_records()
        assert e.value.code == -9
        al.gap_rec_enable(1 << 12)
        _same(_one_batch(al, small), want)
        on = al.gap_rec_stats()
        assert on["launches"] >= 2
        al.gap_enable(8, 1 << 13)                                # another G, another M, a reset: it stays on
        _same(_one_batch(al, small), part.records_of(2, 8, 0, 300))
        al.rescue_enable(1)
        _same(_one_batch(al, small), part.records_of(1, 8, 0, 300))
        al.rescue_enable(2); al.gap_enable(3, 1 << 13); al.gap_reset(); al.rescue_reset()
        _same(_one_batch(al, small), want)
        assert al.gap_rec_stats()["slots"] == 1 << 12
        al.gap_rec_enable(0)                                     # off again
        on = al.gap_rec_stats()["launches"]
        _feed(al, [small])
        assert al.gap_rec_stats() == dict(records=0, reads=0, failed=0, slots=0, launches=on)
        al.gap_rec_enable(1 << 12)
        al.gap_enable(0)                                         # gapped rescue off switches it off too
        assert al.gap_rec_stats()["slots"] == 0
        al.gap_enable(3, 1 << 13)
        _feed(al, [small])
        assert al.gap_rec_stats()["launches"] == on
        al.gap_rec_enable(1 << 12)
        al.rescue_enable(0)                                      # ... and so does rescue off
        assert al.gap_rec_stats()["slots"] == 0
        al.rescue_enable(2); al.gap_enable(3, 1 << 13)
        al.submit(small.seq, small.off)                          # only while nothing is in flight
        with pytest.raises(host.GrootError) as e:
            al.gap_rec_enable(1000)
        assert e.value.code == -9
        al.wait()
    finally:
        al.close()
