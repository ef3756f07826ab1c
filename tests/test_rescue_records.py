"""Rescued records on the device (groot_hip_rescue_rec_*, kernels_rescue_rec.hpp) against the brute force of their definition
(tests/rescue_records_def.py; include/groot_hip.h, "rescued records"): the list a batch hands out equals the definition's record for
record, order included.  The case is that of tests/test_rescue_records_def.py, which also holds the floor of every class of record."""
import numpy as np
import pytest

from groot_amd import device, host
from rescue_records_case import the_case
from rescue_records_def import RECORD_DTYPE, plain
from test_abundance import _dev_ecs
from test_counter_edges import THR, _feed, _of_reads
from test_coverage import STAGES, _stage
from test_rescue import _has_record, _plain

CUTS = [0, 700, 700, 701, 1100, 1500, 1900]      # + the batch's end: seven pieces, one empty and one of a single read


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return the_case(tmp_path_factory)


def _open(case, M=2, slots=1 << 17, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    al = device.Aligner(case.index, threshold=THR, max_batch_reads=max(1024, case.batch.n), **kw)
    if M:
        al.rescue_enable(M)
    if slots:
        al.rescue_rec_enable(slots)
    return al


def _same(got, want):
    assert got.dtype == RECORD_DTYPE == device.RESCUE_RECORD_DTYPE
    if not np.array_equal(got, want):
        n = min(len(got), len(want))
        bad = np.flatnonzero(got[:n] != want[:n])[:5]
        raise AssertionError("device %d records, definition %d; first differences (device, definition): %s"
                             % (len(got), len(want), [(plain(got[i:i + 1]), plain(want[i:i + 1])) for i in bad]))


def _one_batch(al, b, first=0):
    al.submit(b.seq, b.off, first_read_id=first)
    c = al.wait()
    assert c["received"] == b.n
    return al.rescue_records()


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 3])
def test_every_class_at_once(case, hip_lib, monkeypatch, M):
    _stage(monkeypatch, "path_first")
    al = _open(case, M)
    try:
        want = case.records(M)
        _same(_one_batch(al, case.batch), want)
        st = al.rescue_rec_stats()
        print("rescued records", st)
        launches = st.pop("launches")
        assert st == dict(records=len(want), reads=len(np.unique(want["read"])), failed=0, slots=1 << 17), st
        assert launches >= 2 and launches % 2 == 0      # the scan and the emit kernel per pass (a pass that is redone launches them again: they return at once)
        assert al.rescue_stats()["placements"] == len(want)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case, hip_lib, monkeypatch, stage, rod):
    _stage(monkeypatch, stage)
    al = _open(case, results_on_device=rod)
    try:
        _same(_one_batch(al, case.batch), case.records(2))
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("beside", ["classes", "gap", "both"])
def test_beside_the_other_count_kernels(case, hip_lib, monkeypatch, beside):
    """rescue_count_rec_kernel<kGap, kEc> in its three other instances: the list is the same, and what the classes and the gap tables
    hold is what they hold without the records"""
    _stage(monkeypatch, "path_first")
    got = []
    for slots in (0, 1 << 17):
        al = _open(case, slots=slots)
        try:
            if beside != "gap":
                al.ec_enable()
                al.rescue_ec_enable()
            if beside != "classes":
                al.gap_enable(3, 1 << 12)
            if slots:
                _same(_one_batch(al, case.batch), case.records(2))
            else:
                _feed(al, [case.batch])
            got.append((al.rescue(), al.rescue_stats(), _dev_ecs(al) if beside != "gap" else None, al.rescue_ec_stats()["reads"] if beside != "gap" else None,
                        al.gap() if beside != "classes" else None))
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)


def _pieces_pipelined(al, pieces, depth=3):
    """`depth` batches in flight, collected oldest first -> (status, records) of every batch"""
    out, pending, first = [], 0, 0

    def collect():
        r = al.collect(check=False)
        out.append((r["status"], al.rescue_records(r["ticket"])))
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
    """the batch cut into seven, one piece empty and one of a single read, three in flight: every piece hands out the batch's records of
    its reads with batch-relative `read` -- and the same with GROOT_TEST_SMALL_BUFFERS and a piece that is redone at collect for certain,
    which yields the records of its redo, once"""
    cuts = CUTS + [case.batch.n]
    pieces = [case.piece(a, b) for a, b in zip(cuts, cuts[1:])]
    want = [case.records_of(2, a, b) for a, b in zip(cuts, cuts[1:])]
    assert [p.n for p in pieces][1:3] == [0, 1] and len(want[1]) == 0 and sum(len(w) for w in want) == len(case.records(2))
    if small:       # error-free reads with more records than the small buffers hold, and reads of the batch behind them
        rng = np.random.default_rng(16)
        clean = [case.texts[p][0][x:x + 64] for p, x in zip(rng.choice([0, 70, 134, 199, 329, 457], 300), rng.integers(1, 200, 300))]
        extra = _of_reads("mapped and not", clean + case.reads[:150])
        assert int(_has_record(extra, case.index).sum()) >= 280
        w = case.records_of(2, 0, 150)
        w["read"] += 300
        pieces.insert(4, extra)
        want.insert(4, w)
        monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    _stage(monkeypatch, "path_first")
    al = _open(case, pipeline_depth=3)
    try:
        got = _pieces_pipelined(al, pieces)
        assert [s for s, _ in got] == [0] * len(pieces)
        for (_, g), w in zip(got, want):
            _same(g, w)
        st = al.rescue_rec_stats()
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
    lo = 1100
    reads = list(case.reads[lo:])
    has = case.has[lo:]
    mid = next(i for i in range(300, len(reads)) if len(reads[i]) >= 48 and has[i])
    want = case.records_of(2, lo, case.batch.n)
    if kind == "long":
        reads[mid] = reads[mid] * 6                              # (288 bases and more: above the ctx's max_read_len of 256)
        code, want = -6, want[:0]
    elif kind == "short":
        reads[mid] = reads[mid][:5]
        code = -7
    else:
        reads[mid] = reads[mid].lower()
        code = -8
    _stage(monkeypatch, "path_first")
    al = _open(case)
    try:
        b = _of_reads(kind, reads)
        al.submit(b.seq, b.off)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == code
        _same(al.rescue_records(), want)
        _same(_one_batch(al, case.piece(0, lo)), case.records_of(2, 0, lo))
        assert al.rescue_rec_stats()["records"] == len(want) + len(case.records_of(2, 0, lo))
    finally:
        al.close()


@pytest.mark.gpu
def test_room(case, hip_lib, monkeypatch):
    """slots_per_batch exactly the batch's total passes; one less fails the batch with GROOT_E_NOSPACE and a message that names the
    capacity, its other results stay readable, the stats count it, and the next batch is clean"""
    want = case.records(2)
    small = case.piece(0, 700)
    _stage(monkeypatch, "path_first")
    al = _open(case, slots=len(want))
    try:
        _same(_one_batch(al, case.batch), want)
        n_travs, launches = len(al.travs()[0]), al.rescue_rec_stats()["launches"]
        al.rescue_rec_enable(len(want) - 1)
        assert al.rescue_rec_stats() == dict(records=0, reads=0, failed=0, slots=len(want) - 1, launches=launches)      # another capacity: from zero
        al.submit(case.batch.seq, case.batch.off)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == -6 and "slots_per_batch" in str(e.value) and str(len(want) - 1) in str(e.value) and str(len(want)) in str(e.value), e.value
        assert len(al.rescue_records()) == 0
        assert len(al.travs()[0]) == n_travs > 0
        st = al.rescue_rec_stats()
        assert st["failed"] == 1 and st["records"] == 0, st
        _same(_one_batch(al, small, first=case.batch.n), case.records_of(2, 0, 700))
        st = al.rescue_rec_stats()
        assert st["failed"] == 1 and st["records"] == len(case.records_of(2, 0, 700)), st
    finally:
        al.close()


@pytest.mark.gpu
def test_off_on_and_the_enable_rules(case, hip_lib, monkeypatch):
    want = case.records_of(2, 0, 700)
    small = case.piece(0, 700)
    alpha = np.full(case.index.view.n_paths, 1.0 / case.index.view.n_paths)
    _stage(monkeypatch, "path_first")
    al = _open(case, M=0, slots=0)
    try:
        with pytest.raises(host.GrootError) as e:                # needs mismatch rescue
            al.rescue_rec_enable(1000)
        assert e.value.code == -9 and "rescue" in str(e.value), e.value
        al.assign_enable(alpha)                                  # refused with assignment, in either order
        with pytest.raises(host.GrootError) as e:
            al.rescue_rec_enable(1000)
        assert e.value.code == -10 and "assignment" in str(e.value), e.value
        al.assign_enable(None)
        al.rescue_enable(2)
        al.rescue_rec_enable(1 << 16)
        with pytest.raises(host.GrootError) as e:
            al.assign_enable(alpha)
        assert e.value.code == -10 and "rescue" in str(e.value), e.value
        _same(_one_batch(al, small), want)
        on = al.rescue_rec_stats()
        assert on["launches"] >= 2
        al.rescue_rec_enable(0)                                  # off: nothing is launched, nothing is handed out
        _feed(al, [small])
        with pytest.raises(host.GrootError) as e:
            al.rescue_records()
        assert e.value.code == -9
        assert al.rescue_rec_stats() == dict(records=0, reads=0, failed=0, slots=0, launches=on["launches"])
        al.rescue_rec_enable(1 << 16)                            # on again
        _same(_one_batch(al, small), want)
        again = al.rescue_rec_stats()["launches"]
        assert again >= on["launches"] + 2
        al.rescue_enable(0)                                      # rescue off switches it off too
        assert al.rescue_rec_stats()["slots"] == 0
        _feed(al, [small])
        assert al.rescue_rec_stats()["launches"] == again
        al.submit(small.seq, small.off)                          # only while nothing is in flight
        with pytest.raises(host.GrootError) as e:
            al.rescue_rec_enable(1000)
        assert e.value.code == -9
        al.wait()
    finally:
        al.close()


@pytest.mark.gpu
def test_the_other_results_do_not_move(case, hip_lib, monkeypatch):
    """with the feature on, rescue's tables and stats and the other counters' results equal those of a run without it"""
    even = case.piece(0, case.batch.n & ~1)
    _stage(monkeypatch, "path_first")
    got = []
    for slots in (0, 1 << 17):
        al = _open(case, slots=slots)
        try:
            al.coverage_enable(); al.shared_enable(); al.ec_enable(); al.acov_enable()
            _feed(al, [even])
            st = al.rescue_stats()
            got.append((al.rescue(), {k: v for k, v in st.items() if k != "launches"}, al.coverage(), al.shared(), _dev_ecs(al), al.acov()))
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)
