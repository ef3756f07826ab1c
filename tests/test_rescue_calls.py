"""Rescued reads in assigned coverage (groot_hip_rescue_acov_*, kernels_rescue_acov.hpp) against a brute force of the definition
(tests/rescue_calls_def.py): the device's ECs and tuples == the oracle's records plus the rescued reads' kept placements under S+(r),
sorted integer arrays throughout.  The index and the batch are those of test_rescue_calls_def.py, which puts every input class at its
floor on the CPU."""
import numpy as np
import pytest

from groot_amd import device, host
from rescue_calls_def import exact_rows, rescued_records, table_of
from rescue_def import path_texts
from rescue_sets_def import rescued_sets
from test_abundance import _dev_ecs
from test_calls import Table, _dev_table, merge_tables
from test_counter_edges import THR, _feed, _feed_pipelined, _of_reads
from test_coverage import STAGES, _stage
from test_rescue import _has_record, _plain, _reads_of
from test_rescue_calls_def import CallsCase
from test_rescue_ec import CUTS, FLOOR, _refused

ROOM = 1 << 17      # slots that hold the batch's tuples (about 61 000 under M = 1) with half the table free


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return CallsCase(tmp_path_factory.mktemp("rescue_calls_gpu"))


def _open(case, M=1, on=True, min_slots=ROOM, acov=True, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    kw.setdefault("max_batch_reads", max(1024, case.batch.n))
    al = device.Aligner(case.index, threshold=THR, **kw)
    if acov:
        al.acov_enable()
    if M:
        al.rescue_enable(M)
    if on:
        al.rescue_acov_enable(min_slots=min_slots)
    return al


def _same(got, want):
    assert got.ecs == want.ecs, [x for x in zip(got.ecs, want.ecs) if x[0] != x[1]][:5]
    assert got.rows.shape == want.rows.shape, (got.rows.shape, want.rows.shape)
    assert np.array_equal(got.rows, want.rows), (got.rows[np.flatnonzero((got.rows != want.rows).any(axis=1))[:5]], want.rows[np.flatnonzero((got.rows != want.rows).any(axis=1))[:5]])
    assert np.array_equal(got.n, want.n), np.flatnonzero(got.n != want.n)[:10]


def _assert_device(al, want, records, passes=None):
    """want: the definition's Table; records: (rescued records, those folded on the host)"""
    _same(_dev_table(al), want)
    st, ast = al.rescue_acov_stats(), al.acov_stats()
    print("rescue_acov", st, "acov", ast)
    assert (st["records"], st["host_records"], st["dropped"]) == (records[0], records[1], 0), (st, records)
    assert ast["records"] == int(want.n.sum()) and ast["tuples"] == len(want.n), (ast, int(want.n.sum()), len(want.n))
    # three kernels per pass behind the rescued classes' (a pass that collect redoes launches them again, and they return at once in the pass that is not counted)
    assert st["launches"] % 3 == 0 and (passes is None or st["launches"] >= 3 * passes), (st, passes)
    return st


def _pieces(case, cuts):
    return [(_of_reads("piece %d" % i, case.reads[a:b]), range(a, b)) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 3])
def test_every_class_at_once(case, hip_lib, monkeypatch, M):
    _stage(monkeypatch, "path_first")
    al = _open(case, M)
    try:
        _feed(al, [case.batch])
        st = _assert_device(al, case.table(M), case.n_records(M), passes=1)
        assert st["log_rows"] == (8 << 20) // 16 and al.acov_stats()["slots"] >= ROOM
        assert dict(_dev_ecs(al)) == case.expect(M)[0]
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
        _assert_device(al, case.table(1), case.n_records(1), passes=1)
    finally:
        al.close()


@pytest.mark.gpu
def test_forced_slow_mode_and_the_size_of_the_log(case, hip_lib, monkeypatch):
    """GROOT_TEST_SHARED_SLOW: every rescued read whose set lies in more than one graph goes through the bitmaps and the placement log.
    One log entry fewer than those reads have kept placements: GROOT_E_NOSPACE that names the knob; exactly as many: every record counted"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    records = case.n_records(1, max_segs=1)
    assert records[1] >= 4 * FLOOR and records[1] > case.n_records(1)[1] >= 2 * FLOOR
    monkeypatch.setenv("GROOT_TEST_RESCUE_ACOV_LOG", str(records[1] - 1))
    al = _open(case)
    try:
        assert al.rescue_acov_stats()["log_rows"] == records[1] - 1
        al.submit(case.batch.seq, case.batch.off, first_read_id=0)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == -6 and "GROOT_TEST_RESCUE_ACOV_LOG" in str(e.value), e.value      # GROOT_E_NOSPACE
    finally:
        al.close()
    monkeypatch.setenv("GROOT_TEST_RESCUE_ACOV_LOG", str(records[1]))
    al = _open(case)
    try:
        _feed(al, [case.batch])
        assert _assert_device(al, case.table(1), records, passes=1)["log_rows"] == records[1]
    finally:
        al.close()


@pytest.mark.gpu
def test_a_table_too_small_drops_loudly(case, hip_lib, monkeypatch):
    """a table of eight slots and min_slots 0: the batch's rescued tuples exceed the free room, the table grows at collect only -- the
    export fails and says which knob; with a min_slots that holds the batch the same feed is exact"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_ACOV_SLOTS", "8")
    al = _open(case, min_slots=0)
    try:
        assert al.acov_stats()["slots"] == 8
        _feed(al, [case.batch])
        with pytest.raises(host.GrootError) as e:
            al.acov()
        assert e.value.code == -6 and "--callSlots" in str(e.value) and "min_slots" in str(e.value), e.value
        st = al.rescue_acov_stats()
        assert st["dropped"] > 0 and st["records"] + st["dropped"] == case.n_records(1)[0], st
        al.acov_reset()                                         # the table and `dropped` start over: the export works again
        assert al.rescue_acov_stats()["dropped"] == 0 and len(al.acov()[4]) == 0
    finally:
        al.close()
    al = _open(case, min_slots=ROOM)
    try:
        assert al.acov_stats()["slots"] == ROOM
        _feed(al, [case.batch])
        _assert_device(al, case.table(1), case.n_records(1), passes=1)
    finally:
        al.close()


@pytest.mark.gpu
def test_exact_table_grows_at_collect_with_batches_in_flight(case, hip_lib, monkeypatch):
    """eight slots, min_slots 0, three batches in flight.  The reads with a record come first (then an empty batch and one of a single
    read): collect grows the table for them and redoes their claim and add.  The rescued reads follow in pieces of at most 2000 records,
    so that the batches in flight fit the free half: their keys survive every rehash, and the redo adds no rescued record twice"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_ACOV_SLOTS", "8")
    ex, rec = case.exact(), case.records(1)
    mapped = [i for i in range(case.batch.n) if i in ex]
    rest = [i for i in range(case.batch.n) if i not in ex]
    groups, cur, n = [mapped[:-1], [], mapped[-1:]], [], 0
    for i in rest:
        k = len(rec[i]) if i in rec else 0
        if cur and n + k > 2000:
            groups.append(cur)
            cur, n = [], 0
        cur.append(i)
        n += k
    groups.append(cur)
    assert len(mapped) >= 100 and len(groups) >= 20 and len(case.table(1, on=False).n) >= 3 * 2000
    al = _open(case, min_slots=0, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, [_of_reads("group", [case.reads[i] for i in g]) for g in groups]) == [0] * len(groups)
        st = _assert_device(al, case.table(1), case.n_records(1))
        assert st["launches"] >= 3 * sum(1 for g in groups if g), st
        assert al.acov_stats()["grows"] >= 3
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pipelined_pieces_sum_to_the_batch(case, hip_lib, monkeypatch, small):
    """the batch cut into seven, one piece empty and one of a single read, three in flight -- and the same with GROOT_TEST_SMALL_BUFFERS and
    a piece with more records than the small buffers hold, which is redone at collect and counts once"""
    pieces = _pieces(case, CUTS[:-1] + [case.batch.n])
    assert [p.n for p, _ in pieces][1:3] == [0, 1]
    want, records = case.table(1), case.n_records(1)
    if small:
        texts, rng = path_texts(case.index), np.random.default_rng(16)
        clean = [texts[p][0][x:x + 64] for p, x in zip(rng.choice([0, 70, 134, 199, 329, 457], 300), rng.integers(1, 200, 300))]
        extra = _of_reads("mapped and not", clean + case.reads[:150])
        has = _has_record(extra, case.index)
        assert int(has.sum()) >= 280 and len(extra.want(case.index).alns) > 1000
        res = rescued_sets(case.index, 1, _reads_of(extra), has)[0]
        rec = rescued_records(case.index, 1, _reads_of(extra), has)
        want = merge_tables([want, table_of(case.exact(extra), exact_rows(case.index, extra.want(case.index).alns, extra.off), res, rec)])
        slow = sum(len(rec[i]) for i in rec if case.graphs_of(res[i].paths) > 4)
        records = (records[0] + sum(len(r) for r in rec.values()), records[1] + slow)
        pieces.insert(4, (extra, None))
        monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    _stage(monkeypatch, "path_first")
    al = _open(case, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, [p for p, _ in pieces]) == [0] * len(pieces)
        st = _assert_device(al, want, records)
        n = sum(1 for p, _ in pieces if p.n)
        assert st["launches"] > 3 * n if small else st["launches"] >= 3 * n, st
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["long", "short", "lower"])
def test_failing_batch(case, hip_lib, monkeypatch, kind):
    """a batch that fails with GROOT_E_NOSPACE adds nothing; one that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP counts whole (the bad
    read has no record and is no candidate)"""
    cut = 1100
    reads, ex = list(case.reads[cut:]), case.exact()
    mid = next(i for i in range(300, len(reads)) if len(reads[i]) >= 48 and cut + i in ex)
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
        _assert_device(al, case.table(1, counted), case.n_records(1, counted))
    finally:
        al.close()


@pytest.mark.gpu
def test_two_ctxs_merge_to_the_table_of_one(case, hip_lib, monkeypatch):
    (a, ra), (b, rb) = _pieces(case, [0, 2000, case.batch.n])
    _stage(monkeypatch, "path_first")
    al, al2 = _open(case), _open(case)
    try:
        _feed(al, [a])
        _feed(al2, [b])
        s1 = _assert_device(al, case.table(1, ra), case.n_records(1, ra), passes=1)
        s2 = _assert_device(al2, case.table(1, rb), case.n_records(1, rb), passes=1)
        assert (s1["records"] + s2["records"], s1["host_records"] + s2["host_records"]) == case.n_records(1)
        off, ids, cnt, rows, n = host.acov_merge(case.index.view.n_paths, [al.acov(), al2.acov()])
        merged = Table([(tuple(ids[off[i]:off[i + 1]].tolist()), int(cnt[i])) for i in range(len(cnt))], rows, n)
        _same(merged, case.table(1))
    finally:
        al.close()
        al2.close()


@pytest.mark.gpu
def test_off_on_and_every_reset(case, hip_lib, monkeypatch):
    (a, ra), (b, rb) = _pieces(case, [0, 2000, case.batch.n])
    ta, tb, tb_off = case.table(1, ra), case.table(1, rb), case.table(1, rb, on=False)
    _stage(monkeypatch, "path_first")
    al = _open(case)
    try:
        _feed(al, [b])
        al.ec_reset()                                           # the classes, the table, the rescued records in it and the stats start over
        st = al.rescue_acov_stats()
        assert _dev_table(al).ecs == [] and len(al.acov()[4]) == 0 and (st["records"], st["host_records"], st["dropped"]) == (0, 0, 0)
        _feed(al, [a])
        s1 = _assert_device(al, ta, case.n_records(1, ra), passes=2)
        al.rescue_reset()                                       # the rescue tables start over, the pileup stays
        al.rescue_enable(2); al.rescue_enable(1)                # another M and back: likewise
        _assert_device(al, ta, case.n_records(1, ra), passes=2)
        al.rescue_acov_enable(False)                            # off: no launch, the rescued classes off with it, and the table gains the exact records alone
        _feed(al, [b])
        assert al.rescue_acov_stats() == dict(records=0, host_records=0, dropped=0, log_rows=0, launches=s1["launches"])
        assert al.rescue_ec_stats()["rows"] == 0
        _same(_dev_table(al), merge_tables([ta, tb_off]))
        al.rescue_acov_enable()                                 # on again: the table stays, the counts of the rescued start from zero
        _feed(al, [b])
        _same(_dev_table(al), merge_tables([ta, tb_off, tb]))
        st = al.rescue_acov_stats()
        assert (st["records"], st["host_records"]) == case.n_records(1, rb) and st["launches"] >= s1["launches"] + 3, st
        al.acov_reset()                                         # the table and the rescued records' stats; the classes stay
        st = al.rescue_acov_stats()
        assert len(al.acov()[4]) == 0 and (st["records"], st["host_records"]) == (0, 0) and len(_dev_table(al).ecs) == len(merge_tables([ta, tb]).ecs)
        al.rescue_enable(0)                                     # rescue off takes it off too
        assert al.rescue_acov_stats()["log_rows"] == 0 and al.rescue_ec_stats()["rows"] == 0
        al.ec_reset()
        _feed(al, [b])
        assert al.rescue_acov_stats()["launches"] == st["launches"]
        _same(_dev_table(al), tb_off)
    finally:
        al.close()


@pytest.mark.gpu
def test_every_refusal(case, hip_lib, monkeypatch):
    _stage(monkeypatch, "path_first")
    al = _open(case, M=0, on=False, acov=False)
    try:
        _refused(al.rescue_acov_enable, -9, "mismatch rescue is off")                 # GROOT_E_STATE: nothing is on
        al.rescue_enable(1)
        _refused(al.rescue_acov_enable, -9, "equivalence classes are off")
        al.ec_enable()
        _refused(al.rescue_acov_enable, -9, "assigned coverage is off")
        al.pairs_enable()
        _refused(al.rescue_acov_enable, -10, "paired")                               # GROOT_E_UNSUPPORTED
        al.pairs_enable(False)
        al.acov_enable()
        _refused(lambda: al.rescue_acov_enable(min_slots=3 << 10), -1, "power of two")  # GROOT_E_INVALID
        _refused(al.rescue_ec_enable, -10, "assigned coverage")                     # the old enables refuse each other as before ...
        al.acov_enable(False); al.rescue_ec_enable()
        _refused(al.acov_enable, -10, "rescued read")
        al.rescue_ec_enable(False); al.acov_enable()
        assert al.rescue_acov_stats() == dict(records=0, host_records=0, dropped=0, log_rows=0, launches=0)     # nothing left behind
        al.rescue_acov_enable(min_slots=ROOM)
        _refused(al.rescue_ec_enable, -10, "assigned coverage")                     # ... and with the feature on
        _refused(al.pairs_enable, -10, "assigned coverage")
        al.submit(case.batch.seq, case.batch.off, first_read_id=0)
        _refused(lambda: al.rescue_acov_enable(False), -9, "in flight")
        _refused(al.rescue_acov_enable, -9, "in flight")
        al.wait()
        _assert_device(al, case.table(1), case.n_records(1), passes=1)
        al.acov_enable(False)                                   # assigned coverage off takes it and the rescued classes off
        assert al.rescue_acov_stats()["log_rows"] == 0 and al.rescue_ec_stats()["rows"] == 0
        al.acov_enable(); al.rescue_acov_enable()
        al.ec_enable(False)                                     # and so do the classes
        assert al.rescue_acov_stats()["log_rows"] == 0 and al.acov_stats()["slots"] == 0
        al.acov_enable(); al.rescue_acov_enable(min_slots=ROOM)
        _feed(al, [case.batch])
        _assert_device(al, case.table(1), case.n_records(1), passes=2)
    finally:
        al.close()


@pytest.mark.gpu
def test_everything_else_is_unchanged(case, hip_lib, monkeypatch):
    """coverage, shared reads, the rescue tables, the gap tables, their stats and the records with the feature on == without it; the
    classes with it == those of the rescued reads in the classes alone"""
    _stage(monkeypatch, "path_first")
    got = []
    for on in (False, True):
        al = _open(case, M=2, on=False, acov=on)
        try:
            al.ec_enable(); al.coverage_enable(); al.shared_enable(); al.gap_enable(3)
            if on:
                al.rescue_acov_enable(min_slots=ROOM)
            else:
                al.rescue_ec_enable()
            al.submit(case.batch.seq, case.batch.off, first_read_id=0)
            counts = al.wait()
            alns = al.alns()
            order = np.lexsort([alns[f] for f in reversed(alns.dtype.names)])
            got.append((counts, alns[order].tolist(), al.coverage(), al.shared(), al.shared_stats(), al.rescue(), al.rescue_stats(), al.gap()[0], al.gap()[1].tolist(),
                        al.gap_stats(), _dev_ecs(al), al.ec_stats(), {k: v for k, v in al.rescue_ec_stats().items() if k != "launches"}))
            if on:
                _assert_device(al, case.table(2), case.n_records(2), passes=1)
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)
