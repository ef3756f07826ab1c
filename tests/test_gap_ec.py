"""Gap-placed reads in the equivalence classes (groot_hip_gap_ec_*, kernels_gap_ec.hpp) against a brute force of the definition
(tests/gap_sets_def.py): the device's ECs == the oracle's records' ECs plus the rescued reads' sets plus the gap-rescued reads' sets,
integers throughout.  The index and the batch are those of tests/gap_ec_case.py; tests/test_gap_ec_def.py checks on the CPU that they
hold every class."""
from collections import namedtuple
from itertools import product

import numpy as np
import pytest

import gap_ec_case
from gap_sets_def import ecs_plus3, gap_sets
from groot_amd import device, host
from rescue_def import path_texts
from rescue_sets_def import rescued_sets
from test_abundance import _dev_ecs
from test_counter_edges import THR, _feed, _feed_pipelined, _first_diff, _of_reads
from test_coverage import STAGES, _stage
from test_rescue import _has_record, _plain, _reads_of

SLOTS = 1 << 12
# ecs: {ids: reads}; res / res_slow: rescued reads added, slow ones among them; gap / gap_slow: gap-rescued likewise; mapped / mapped_slow:
# reads with a record likewise
Want = namedtuple("Want", "ecs res res_slow gap gap_slow mapped mapped_slow")


def _sum(a, b):
    ecs = dict(a)
    for k, v in b.items():
        ecs[k] = ecs.get(k, 0) + v
    return ecs


def _add(a, b):
    return Want(_sum(a.ecs, b.ecs), *(x + y for x, y in zip(a[1:], b[1:])))


def _want(case, ex, res, gap, reads, max_segs=4):
    slow = lambda s: case.graphs_of(s) > max_segs
    r, g, m = ([i for i in reads if i in d] for d in (res, gap, ex))
    return Want(ecs_plus3(ex, res, gap, reads), len(r), sum(slow(res[i].paths) for i in r), len(g), sum(slow(gap[i].paths) for i in g), len(m),
                sum(slow(ex[i]) for i in m))


def _expect(case, M=2, G=3, reads=None, max_segs=4, gapped=True, rescued=True):
    """the definition over `reads` of the batch (default: all); gapped / rescued off: what the run counts with that feature off"""
    return _want(case, case.exact(), case.rescued(M)[0] if rescued else {}, case.gapped(M, G)[0] if gapped and rescued else {},
                 range(case.batch.n) if reads is None else reads, max_segs)


def _expect_batch(case, batch, M=2, G=3):
    """the definition over another batch of the same index"""
    reads, has = _reads_of(batch), _has_record(batch, case.index)
    return _want(case, case.exact(batch), rescued_sets(case.index, M, reads, has)[0], gap_sets(case.index, M, G, reads, has, case.placements(M, G))[0], range(batch.n))


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return gap_ec_case.case(tmp_path_factory)


def _open(case, M=2, G=3, on=True, rec=True, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    kw.setdefault("max_batch_reads", max(1024, case.batch.n))
    al = device.Aligner(case.index, threshold=THR, **kw)
    al.ec_enable()
    al.rescue_enable(M)
    al.gap_enable(G, SLOTS)
    if rec:
        al.rescue_ec_enable()
    if on:
        al.gap_ec_enable()
    return al


def _assert_device(al, want, passes=None):
    got = dict(_dev_ecs(al))
    assert got == want.ecs, _first_diff(got, want.ecs)
    st, rs, es = al.gap_ec_stats(), al.rescue_ec_stats(), al.ec_stats()
    print("gap_ec", st, "rescue_ec", rs, "ec", es)
    assert (st["reads"], st["slow_reads"]) == (want.gap, want.gap_slow), (st, want[1:])
    assert (rs["reads"], rs["slow_reads"]) == (want.res, want.res_slow), (rs, want[1:])            # (the ungapped reads' alone, as ever)
    assert (es["reads"], es["distinct"], es["slow_reads"]) == (want.mapped + want.res + want.gap, len(want.ecs), want.mapped_slow), (es, want[1:])
    # two kernels per pass among the rescued reads' three (a pass that collect redoes launches them again, and they return at once)
    assert st["launches"] % 2 == 0 and (passes is None or st["launches"] >= 2 * passes), (st, passes)
    return st


def _pieces(case, cuts):
    return [(_of_reads("piece %d" % i, case.reads[a:b]), range(a, b)) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]


@pytest.mark.gpu
@pytest.mark.parametrize("M,G", [(2, 3), (2, 8), (1, 3), (1, 1)])
def test_every_class_at_once(case, hip_lib, monkeypatch, M, G):
    _stage(monkeypatch, "path_first")
    want = _expect(case, M, G)
    assert want.gap - want.gap_slow >= 10 and want.gap_slow >= 3 and want.res_slow >= 3, want[1:]
    al = _open(case, M, G)
    try:
        _feed(al, [case.batch])
        _assert_device(al, want, passes=1)
        assert al.gap_stats()["rescued"] == want.gap                # every gap-rescued read of the tables is in a class, and no other
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case, hip_lib, monkeypatch, stage, rod):
    _stage(monkeypatch, stage)
    al = _open(case, results_on_device=rod)
    try:
        _feed(al, [case.batch])
        _assert_device(al, _expect(case), passes=1)
    finally:
        al.close()


@pytest.mark.gpu
def test_every_sink_combination(case, hip_lib, monkeypatch):
    """the gapped records and the rescued records on or off beside the feature: the classes are the definition's, the records those of
    a run without the feature"""
    _stage(monkeypatch, "path_first")

    def run(on, gr, rr):
        al = _open(case, on=on)
        try:
            if rr:
                al.rescue_rec_enable(1 << 16)
            if gr:
                al.gap_rec_enable(1 << 16)
            al.submit(case.batch.seq, case.batch.off, first_read_id=0)
            al.wait()
            out = (al.rescue_records().tobytes() if rr else None, al.gap_records().tobytes() if gr else None)
            if on:
                _assert_device(al, _expect(case), passes=1)
            return out
        finally:
            al.close()

    ref = run(False, True, True)
    assert len(ref[0]) >= 100 * 20 and len(ref[1]) >= 100 * 24        # (20 and 24 bytes a record)
    for gr, rr in product((False, True), repeat=2):
        got = run(True, gr, rr)
        assert got[0] == (ref[0] if rr else None) and got[1] == (ref[1] if gr else None), (gr, rr)


@pytest.mark.gpu
def test_forced_slow_mode(case, hip_lib, monkeypatch):
    """GROOT_TEST_SHARED_SLOW: every set in more than one graph goes through the bitmaps"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    al = _open(case)
    try:
        _feed(al, [case.batch])
        want = _expect(case, max_segs=1)
        assert want.gap_slow >= 30 and want.gap_slow > _expect(case).gap_slow
        _assert_device(al, want, passes=1)
    finally:
        al.close()


@pytest.mark.gpu
def test_too_few_bitmaps_fail_the_batch(case, hip_lib, monkeypatch):
    """the rescued and the gap-rescued slow reads share the slot's bitmaps: one fewer than both need is GROOT_E_NOSPACE that names the
    knob, exactly as many counts every read"""
    _stage(monkeypatch, "path_first")
    want = _expect(case)
    need = want.res_slow + want.gap_slow
    assert want.res_slow >= 3 and want.gap_slow >= 3
    monkeypatch.setenv("GROOT_TEST_RESCUE_EC_ROWS", str(need - 1))
    al = _open(case)
    try:
        assert al.rescue_ec_stats()["rows"] == need - 1
        al.submit(case.batch.seq, case.batch.off, first_read_id=0)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == -6 and "GROOT_TEST_RESCUE_EC_ROWS" in str(e.value) and "gap-rescued" in str(e.value), e.value      # GROOT_E_NOSPACE
    finally:
        al.close()
    monkeypatch.setenv("GROOT_TEST_RESCUE_EC_ROWS", str(need))
    al = _open(case)
    try:
        _feed(al, [case.batch])
        _assert_device(al, want, passes=1)
        assert al.rescue_ec_stats()["rows"] == need
    finally:
        al.close()


CUTS = [0, 150, 150, 151, 250, 350, 450]


@pytest.mark.gpu
def test_table_growth_with_batches_in_flight(case, hip_lib, monkeypatch):
    """GROOT_TEST_EC_SLOTS small and three batches in flight: the table of classes grows between merges, the gap-placed sets among them"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_EC_SLOTS", "2")
    pieces = _pieces(case, CUTS + [case.batch.n])
    al = _open(case, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, [p for p, _ in pieces]) == [0] * len(pieces)
        _assert_device(al, _expect(case), passes=sum(1 for p, _ in pieces if p.n))
        assert al.ec_stats()["grows"] >= 1
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pipelined_pieces_sum_to_the_batch(case, hip_lib, monkeypatch, small):
    """the batch cut into seven, one piece empty and one of a single read, three in flight -- and the same with GROOT_TEST_SMALL_BUFFERS and
    a piece with more records than the small buffers hold, which is redone at collect and counts once"""
    pieces = _pieces(case, CUTS + [case.batch.n])
    assert [p.n for p, _ in pieces][1:3] == [0, 1]
    want = _expect(case)
    if small:
        texts, rng = path_texts(case.index), np.random.default_rng(26)
        clean = [texts[p][0][x:x + 100] for p, x in zip(rng.choice([2, 3, 4, 5], 300), rng.integers(1, 140, 300))]
        extra = _of_reads("mapped and not", clean + case.reads[:100])
        assert int(_has_record(extra, case.index).sum()) >= 280 and len(extra.want(case.index).alns) > 64          # (the small buffers hold 64 records)
        we = _expect_batch(case, extra)
        assert we.gap >= 10
        want = _add(want, we)
        pieces.insert(4, (extra, None))
        monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    _stage(monkeypatch, "path_first")
    al = _open(case, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, [p for p, _ in pieces]) == [0] * len(pieces)
        st = _assert_device(al, want)
        n = sum(1 for p, _ in pieces if p.n)
        assert st["launches"] > 2 * n if small else st["launches"] >= 2 * n, st      # (a pass that was redone launched its kernels again, and counted once)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["long", "short", "lower"])
def test_failing_batch(case, hip_lib, monkeypatch, kind):
    """a batch that fails with GROOT_E_NOSPACE adds nothing; one that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP counts whole (the bad
    read has no record and is no candidate)"""
    cut = 300
    reads, ex, gap = list(case.reads[cut:]), case.exact(), case.gapped(2, 3)[0]
    assert sum(1 for i in gap if i >= cut) >= 30
    mid = next(i for i in range(50, len(reads)) if len(reads[i]) >= 48 and cut + i in ex)
    reads[mid] = {"long": reads[mid] * 6, "short": reads[mid][:5], "lower": reads[mid].lower()}[kind]
    code = {"long": -6, "short": -7, "lower": -8}[kind]
    counted = list(range(cut)) + ([] if kind == "long" else [i for i in range(cut, case.batch.n) if i != cut + mid])
    _stage(monkeypatch, "path_first")
    al = _open(case)
    try:
        first = _feed(al, [_of_reads("good", case.reads[:cut])])
        b = _of_reads(kind, reads)
        al.submit(b.seq, b.off, first_read_id=first)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == code
        _assert_device(al, _expect(case, reads=counted))
    finally:
        al.close()


@pytest.mark.gpu
def test_two_ctxs_off_on_and_reset(case, hip_lib, monkeypatch):
    (a, ra), (b, rb) = _pieces(case, [0, 300, case.batch.n])
    wa, wb, whole = _expect(case, reads=ra), _expect(case, reads=rb), _expect(case)
    off = _expect(case, reads=rb, gapped=False)                 # what the run counts of b with the feature off: today's classes
    assert wa.gap >= 10 and wb.gap >= 10 and wb.gap_slow >= 3
    _stage(monkeypatch, "path_first")
    al, al2 = _open(case), _open(case)
    try:
        _feed(al, [b])
        al.ec_reset()                                           # the classes, the gap-placed reads in them and the stats start over
        assert _dev_ecs(al) == [] and al.gap_ec_stats()["reads"] == 0 and al.rescue_ec_stats()["reads"] == 0
        _feed(al, [a])
        s1 = _assert_device(al, wa, passes=2)
        _feed(al2, [b])
        s2 = _assert_device(al2, wb, passes=1)
        assert _sum(dict(_dev_ecs(al)), dict(_dev_ecs(al2))) == whole.ecs          # the merge of two ctxs is a sum by set
        assert s1["reads"] + s2["reads"] == whole.gap and s1["slow_reads"] + s2["slow_reads"] == whole.gap_slow
        al.gap_enable(8, SLOTS); al.gap_enable(3, SLOTS)        # another G and back: the gap tables start over, the classes stay
        al.rescue_enable(1); al.rescue_enable(2)                # another M and back: likewise
        _assert_device(al, wa, passes=2)
        al.gap_ec_enable(False)                                 # off: no launch, and the classes gain what today's code counts
        _feed(al, [b])
        assert al.gap_ec_stats() == dict(reads=0, slow_reads=0, launches=s1["launches"])
        ecs = _sum(wa.ecs, off.ecs)
        assert dict(_dev_ecs(al)) == ecs
        al.gap_ec_enable()                                      # on again: the classes stay, the counts of the gap-placed start from zero
        _feed(al, [b])
        ecs = _sum(ecs, wb.ecs)
        st = al.gap_ec_stats()
        assert dict(_dev_ecs(al)) == ecs
        assert (st["reads"], st["slow_reads"]) == (wb.gap, wb.gap_slow) and st["launches"] >= s1["launches"] + 2, st
        al.gap_enable(0)                                        # gapped rescue off takes it off too
        assert al.gap_ec_stats() == dict(reads=0, slow_reads=0, launches=st["launches"])
        al.gap_enable(3, SLOTS)
        _feed(al, [b])
        ecs = _sum(ecs, off.ecs)
        assert dict(_dev_ecs(al)) == ecs and al.gap_ec_stats()["launches"] == st["launches"]
        al.gap_ec_enable()
        al.rescue_ec_enable(False)                              # and so do the rescued reads in the classes going off
        assert al.gap_ec_stats() == dict(reads=0, slow_reads=0, launches=st["launches"])
        _feed(al, [b])
        ecs = _sum(ecs, _expect(case, reads=rb, rescued=False).ecs)
        assert dict(_dev_ecs(al)) == ecs and al.gap_ec_stats()["launches"] == st["launches"]
        al.rescue_ec_enable(); al.gap_ec_enable()
        al.rescue_enable(0)                                     # mismatch rescue off, and the classes off
        assert al.gap_ec_stats()["reads"] == 0
        al2.ec_enable(False)
        assert al2.gap_ec_stats() == dict(reads=0, slow_reads=0, launches=s2["launches"])
    finally:
        al.close()
        al2.close()


@pytest.mark.gpu
def test_feature_off_is_todays_code(case, hip_lib, monkeypatch):
    """with gapped rescue and the rescued reads in the classes on and the feature off, the classes are today's and nothing is launched"""
    _stage(monkeypatch, "path_first")
    al = _open(case, on=False)
    try:
        _feed(al, [case.batch])
        want = _expect(case, gapped=False)
        assert dict(_dev_ecs(al)) == want.ecs and want.gap == 0
        assert al.gap_ec_stats() == dict(reads=0, slow_reads=0, launches=0)
        assert al.rescue_ec_stats()["reads"] == want.res
    finally:
        al.close()


def _refused(call, code, *words):
    with pytest.raises(host.GrootError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), e.value


@pytest.mark.gpu
def test_refusals_in_both_orders(case, hip_lib, monkeypatch):
    _stage(monkeypatch, "path_first")
    al = device.Aligner(case.index, threshold=THR, memo_budget_mb=device.MEMO_OFF, max_read_len=256, max_batch_reads=max(1024, case.batch.n))
    try:
        _refused(al.gap_ec_enable, -9, "gapped rescue is off")                   # GROOT_E_STATE: nothing is on
        al.ec_enable(); al.rescue_enable(2); al.rescue_ec_enable()
        _refused(al.gap_ec_enable, -9, "gapped rescue is off")                   # the rescued reads in the classes alone
        al.rescue_ec_enable(False); al.gap_enable(3, SLOTS)
        _refused(al.gap_ec_enable, -9, "rescued reads in the equivalence classes are off")      # gapped rescue alone
        al.acov_enable(); al.rescue_acov_enable()                                # rescued assigned coverage first
        _refused(al.gap_ec_enable, -10, "assigned coverage")                     # GROOT_E_UNSUPPORTED
        al.rescue_acov_enable(False); al.acov_enable(False)
        al.rescue_ec_enable(); al.gap_ec_enable()                                # the feature first
        _refused(al.rescue_acov_enable, -10, "gap-placed reads")
        al.submit(case.batch.seq, case.batch.off, first_read_id=0)
        _refused(lambda: al.gap_ec_enable(False), -9, "in flight")
        _refused(al.gap_ec_enable, -9, "in flight")
        al.wait()
        _assert_device(al, _expect(case), passes=1)                              # none of the refusals left anything behind
    finally:
        al.close()


@pytest.mark.gpu
def test_everything_else_is_unchanged(case, hip_lib, monkeypatch):
    """coverage, shared reads, the rescue tables, the gap tables and events, their stats, the rescued reads' stats and the records with the
    feature on == without it"""
    _stage(monkeypatch, "path_first")
    got = []
    for on in (False, True):
        al = _open(case, on=False)
        try:
            al.coverage_enable(); al.shared_enable()
            if on:
                al.gap_ec_enable()
            al.submit(case.batch.seq, case.batch.off, first_read_id=0)
            counts = al.wait()
            alns = al.alns()
            order = np.lexsort([alns[f] for f in reversed(alns.dtype.names)])
            got.append((counts, alns[order].tolist(), al.coverage(), al.shared(), al.shared_stats(), al.rescue(), al.rescue_stats(), al.gap()[0], al.gap()[1].tolist(),
                        al.gap_stats(), al.rescue_ec_stats()))
            if on:
                _assert_device(al, _expect(case), passes=1)
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)
