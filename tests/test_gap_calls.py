"""Gap-placed reads in assigned coverage (groot_hip_gap_acov_*, kernels_gap_acov.hpp) against a brute force of the definition
(tests/gap_calls_def.py): the device's ECs and tuples == the oracle's records plus the rescued reads' kept placements plus the gap-rescued
reads' gapped records (a DEL two, an INS one) under S++(r), sorted integer arrays throughout.  The index and the batch are those of
tests/gap_ec_case.py; tests/test_gap_calls_def.py puts every input class at its floor on the CPU."""
import numpy as np
import pytest

import gap_ec_case
from gap_calls_def import gap_calls, rows_of, table_of3
from gap_def import keep
from gap_sets_def import gap_sets
from groot_amd import device, host
from rescue_calls_def import exact_rows, rescued_records
from rescue_def import A, path_texts
from rescue_sets_def import rescued_sets
from test_calls import Table, _dev_table, merge_tables
from test_counter_edges import THR, _feed, _feed_pipelined, _of_reads
from test_coverage import STAGES, _stage
from test_gap_ec import CUTS, SLOTS, _pieces, _refused
from test_rescue import _has_record, _plain, _reads_of
from test_rescue_calls import _same

ROOM = 1 << 16      # slots that hold the batch's tuples with more than half the table free
ZERO = dict(placements=0, records=0, host_records=0, dropped=0)


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return gap_ec_case.case(tmp_path_factory)


@pytest.fixture(scope="module")
def gc(case):
    return gap_calls(case)


def _open(case, M=2, G=3, on=True, min_slots=ROOM, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    kw.setdefault("max_batch_reads", max(1024, case.batch.n))
    al = device.Aligner(case.index, threshold=THR, **kw)
    al.acov_enable()
    al.rescue_enable(M)
    al.gap_enable(G, SLOTS)
    al.rescue_acov_enable(min_slots=min_slots)
    if on:
        al.gap_acov_enable()
    return al


def _no_launches(st):
    return {k: v for k, v in st.items() if k != "launches"}


def _assert_stats(al, c, want, passes=None):
    """c: gap_calls_def.GapCalls.counts(); want: the definition's Table"""
    st, rs, ast, es = al.gap_acov_stats(), al.rescue_acov_stats(), al.acov_stats(), al.gap_ec_stats()
    print("gap_acov", st, "rescue_acov", rs, "acov", ast, "gap_ec", es)
    assert (st["placements"], st["records"], st["host_records"], st["dropped"]) == (c["placements"], c["records"], c["host_records"], 0), (st, c)
    assert (rs["records"], rs["host_records"], rs["dropped"]) == (c["res_records"], c["host_entries_res"], 0), (rs, c)      # (the ungapped reads' alone, as ever)
    assert (es["reads"], es["slow_reads"]) == (c["gap"], c["gap_slow"]), (es, c)
    assert ast["records"] == int(want.n.sum()) and ast["tuples"] == len(want.n), (ast, int(want.n.sum()), len(want.n))
    # four launches per pass (a pass that collect redoes launches them again, and they return at once in the pass that is not counted)
    assert st["launches"] % 4 == 0 and (passes is None or st["launches"] >= 4 * passes), (st, passes)
    return st


def _assert_device(al, gc, M=2, G=3, reads=None, max_segs=4, passes=None):
    want = gc.table(M, G, None if reads is None else list(reads))
    _same(_dev_table(al), want)
    return _assert_stats(al, gc.counts(M, G, reads, max_segs), want, passes)


@pytest.mark.gpu
@pytest.mark.parametrize("M,G", [(2, 3), (2, 8), (1, 3), (1, 1)])
def test_every_class_at_once(case, gc, hip_lib, monkeypatch, M, G):
    _stage(monkeypatch, "path_first")
    c = gc.counts(M, G)
    assert c["records"] > c["placements"] >= 20 and c["host_records"] >= 3 and c["records"] - c["host_records"] >= 20, c
    al = _open(case, M, G)
    try:
        _feed(al, [case.batch])
        _assert_device(al, gc, M, G, passes=1)
        gs = al.gap_stats()
        assert gs["placements"] == c["placements"] and gs["del_placements"] == c["records"] - c["placements"]      # every kept placement of the tables is piled up
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case, gc, hip_lib, monkeypatch, stage, rod):
    _stage(monkeypatch, stage)
    al = _open(case, results_on_device=rod)
    try:
        _feed(al, [case.batch])
        _assert_device(al, gc, passes=1)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("records", [False, True])
def test_beside_the_gapped_records(case, gc, hip_lib, monkeypatch, records):
    """both instantiations of rescue_gap_ec_kernel: the table is the definition's, the gapped records those of a run without the feature"""
    _stage(monkeypatch, "path_first")
    got = []
    for on in ((False, True) if records else (True,)):
        al = _open(case, on=on)
        try:
            if records:
                al.gap_rec_enable(1 << 16)
            al.submit(case.batch.seq, case.batch.off, first_read_id=0)
            al.wait()
            if records:
                got.append(al.gap_records().tobytes())
            if on:
                _assert_device(al, gc, passes=1)
        finally:
            al.close()
    if records:
        assert len(got[0]) >= 100 * 24 and got[0] == got[1]


@pytest.mark.gpu
def test_forced_slow_mode_and_the_size_of_the_log(case, gc, hip_lib, monkeypatch):
    """GROOT_TEST_SHARED_SLOW: every read whose set lies in more than one graph goes through the bitmaps and the log, which the rescued
    reads' placements and the gapped records share.  One entry fewer than both need: GROOT_E_NOSPACE that names the knob; exactly as many:
    every record counted"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    c = gc.counts(max_segs=1)
    assert c["host_records"] >= 100 and c["host_records"] > gc.counts()["host_records"] >= 10 and c["host_entries_res"] >= 10, c
    need = c["host_entries_res"] + c["host_records"]
    monkeypatch.setenv("GROOT_TEST_RESCUE_ACOV_LOG", str(need - 1))
    al = _open(case)
    try:
        assert al.rescue_acov_stats()["log_rows"] == need - 1
        al.submit(case.batch.seq, case.batch.off, first_read_id=0)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == -6 and "GROOT_TEST_RESCUE_ACOV_LOG" in str(e.value) and "gapped records" in str(e.value), e.value      # GROOT_E_NOSPACE
    finally:
        al.close()
    monkeypatch.setenv("GROOT_TEST_RESCUE_ACOV_LOG", str(need))
    al = _open(case)
    try:
        _feed(al, [case.batch])
        _assert_device(al, gc, max_segs=1, passes=1)
        assert al.rescue_acov_stats()["log_rows"] == need
    finally:
        al.close()


@pytest.mark.gpu
def test_too_few_bitmaps_fail_the_batch(case, gc, hip_lib, monkeypatch):
    """the bitmaps the two kinds of slow reads share: one fewer than both need fails the batch, exactly as many counts every record"""
    _stage(monkeypatch, "path_first")
    c = gc.counts()
    need = c["res_slow"] + c["gap_slow"]
    assert c["res_slow"] >= 3 and c["gap_slow"] >= 3
    monkeypatch.setenv("GROOT_TEST_RESCUE_EC_ROWS", str(need - 1))
    al = _open(case)
    try:
        al.submit(case.batch.seq, case.batch.off, first_read_id=0)
        with pytest.raises(host.GrootError) as e:
            al.wait()
        assert e.value.code == -6 and "GROOT_TEST_RESCUE_EC_ROWS" in str(e.value), e.value
    finally:
        al.close()
    monkeypatch.setenv("GROOT_TEST_RESCUE_EC_ROWS", str(need))
    al = _open(case)
    try:
        _feed(al, [case.batch])
        _assert_device(al, gc, passes=1)
    finally:
        al.close()


@pytest.mark.gpu
def test_a_table_too_small_drops_loudly(case, gc, hip_lib, monkeypatch):
    """a table of eight slots and min_slots 0: the gapped records exceed the free room, the table grows at collect only -- the export
    fails and says which knob, and `dropped` counts records; with a min_slots that holds the batch the same feed is exact"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_ACOV_SLOTS", "8")
    c = gc.counts()
    al = _open(case, min_slots=0)
    try:
        assert al.acov_stats()["slots"] == 8
        _feed(al, [case.batch])
        with pytest.raises(host.GrootError) as e:
            al.acov()
        assert e.value.code == -6 and "--callSlots" in str(e.value) and "min_slots" in str(e.value), e.value
        st = al.gap_acov_stats()
        assert st["dropped"] > 0 and st["records"] + st["dropped"] == c["records"] and st["placements"] == c["placements"], (st, c)
        al.acov_reset()                                         # the table and `dropped` start over: the export works again
        assert _no_launches(al.gap_acov_stats()) == ZERO and al.rescue_acov_stats()["dropped"] == 0 and len(al.acov()[4]) == 0
    finally:
        al.close()
    al = _open(case, min_slots=ROOM)
    try:
        assert al.acov_stats()["slots"] == ROOM
        _feed(al, [case.batch])
        _assert_device(al, gc, passes=1)
    finally:
        al.close()


@pytest.mark.gpu
def test_exact_table_grows_at_collect_with_batches_in_flight(case, gc, hip_lib, monkeypatch):
    """eight slots, min_slots 0, three batches in flight.  The reads with a record come first (then an empty batch and one of a single
    read): collect grows the table for them and redoes their claim and add.  The other reads follow in pieces whose rescued and gapped
    records fit the room the exact tuples have made, so that their keys survive every rehash and the redo adds none of them twice"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_ACOV_SLOTS", "8")
    ex, rrec, grec = case.exact(), gc.res_records(2), gc.gap_records(2, 3)
    n_exact = len(gc.table(rescued=False).n)
    per = max(n_exact // 4, max(len(r) for r in list(rrec.values()) + list(grec.values())))
    mapped = [i for i in range(case.batch.n) if i in ex]
    rest = [i for i in range(case.batch.n) if i not in ex]
    groups, cur, n = [mapped[:-1], [], mapped[-1:]], [], 0
    for i in rest:
        k = len(rrec.get(i, ())) + len(grec.get(i, ()))
        if cur and n + k > per:
            groups.append(cur)
            cur, n = [], 0
        cur.append(i)
        n += k
    groups.append(cur)
    assert len(mapped) >= 50 and len(groups) >= 6 and n_exact >= 3 * per, (len(mapped), len(groups), n_exact, per)
    al = _open(case, min_slots=0, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, [_of_reads("group", [case.reads[i] for i in g]) for g in groups]) == [0] * len(groups)
        st = _assert_device(al, gc)
        assert st["launches"] >= 4 * sum(1 for g in groups if g), st
        assert al.acov_stats()["grows"] >= 3
    finally:
        al.close()


def _table_of_batch(case, batch, M=2, G=3):
    """the definition over another batch of the same index -> (Table, counts as GapCalls.counts())"""
    reads, has = _reads_of(batch), _has_record(batch, case.index)
    res, left = rescued_sets(case.index, M, reads, has)
    rrec = rescued_records(case.index, M, reads, has)
    brute = case.placements(M, G)
    gap = gap_sets(case.index, M, G, reads, has, brute)[0]
    firsts = [t[1] for t in path_texts(case.index)]
    kept = {i: keep(brute(reads[i]), M, G)[1] for i in left if len(reads[i]) >= A * (M + 3)}
    kept = {i: k for i, k in kept.items() if k}
    grec = {i: rows_of(k, len(reads[i]), lambda p: firsts[p]) for i, k in kept.items()}
    t = table_of3(case.exact(batch), exact_rows(case.index, batch.want(case.index).alns, batch.off), res, rrec, gap, grec, kept)
    slow = lambda s: case.graphs_of(s) > 4
    gs = [i for i in gap if slow(gap[i].paths)]
    return t, dict(gap=len(gap), gap_slow=len(gs), placements=sum(len(k) for k in kept.values()), records=sum(len(r) for r in grec.values()),
                   host_records=sum(len(grec[i]) for i in gs), host_entries_res=sum(len(rrec[i]) for i in rrec if slow(res[i].paths)),
                   res_records=sum(len(r) for r in rrec.values()), res_slow=sum(1 for i in rrec if slow(res[i].paths)))


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pipelined_pieces_sum_to_the_batch(case, gc, hip_lib, monkeypatch, small):
    """the batch cut into seven, one piece empty and one of a single read, three in flight -- and the same with GROOT_TEST_SMALL_BUFFERS and
    a piece with more records than the small buffers hold, which is redone at collect and counts once"""
    pieces = _pieces(case, CUTS + [case.batch.n])
    assert [p.n for p, _ in pieces][1:3] == [0, 1]
    want, c = gc.table(), gc.counts()
    if small:
        texts, rng = path_texts(case.index), np.random.default_rng(26)
        clean = [texts[p][0][x:x + 100] for p, x in zip(rng.choice([2, 3, 4, 5], 300), rng.integers(1, 140, 300))]
        extra = _of_reads("mapped and not", clean + case.reads[:100])
        assert int(_has_record(extra, case.index).sum()) >= 280 and len(extra.want(case.index).alns) > 64          # (the small buffers hold 64 records)
        te, ce = _table_of_batch(case, extra)
        assert ce["records"] >= 10
        want, c = merge_tables([want, te]), {k: v + ce[k] for k, v in c.items()}
        pieces.insert(4, (extra, None))
        monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    _stage(monkeypatch, "path_first")
    al = _open(case, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, [p for p, _ in pieces]) == [0] * len(pieces)
        _same(_dev_table(al), want)
        st = _assert_stats(al, c, want)
        n = sum(1 for p, _ in pieces if p.n)
        assert st["launches"] > 4 * n if small else st["launches"] >= 4 * n, st      # (a pass that was redone launched its kernels again, and counted once)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["long", "short", "lower"])
def test_failing_batch(case, gc, hip_lib, monkeypatch, kind):
    """a batch that fails with GROOT_E_NOSPACE adds nothing; one that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP counts whole (the bad
    read has no record and is no candidate)"""
    cut = 300
    reads, ex = list(case.reads[cut:]), case.exact()
    assert sum(len(r) for i, r in gc.gap_records(2, 3).items() if i >= cut) >= 100
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
        _assert_device(al, gc, reads=counted)
    finally:
        al.close()


@pytest.mark.gpu
def test_two_ctxs_merge_to_the_table_of_one(case, gc, hip_lib, monkeypatch):
    (a, ra), (b, rb) = _pieces(case, [0, 300, case.batch.n])
    _stage(monkeypatch, "path_first")
    al, al2 = _open(case), _open(case)
    try:
        _feed(al, [a])
        _feed(al2, [b])
        s1 = _assert_device(al, gc, reads=ra, passes=1)
        s2 = _assert_device(al2, gc, reads=rb, passes=1)
        c = gc.counts()
        assert all(s1[k] + s2[k] == c[k] for k in ("placements", "records", "host_records")) and min(s1["records"], s2["records"]) >= 100
        off, ids, cnt, rows, n = host.acov_merge(case.index.view.n_paths, [al.acov(), al2.acov()])
        merged = Table([(tuple(ids[off[i]:off[i + 1]].tolist()), int(cnt[i])) for i in range(len(cnt))], rows, n)
        _same(merged, gc.table())
    finally:
        al.close()
        al2.close()


@pytest.mark.gpu
def test_off_on_every_reset_and_every_way_off(case, gc, hip_lib, monkeypatch):
    (a, ra), (b, rb) = _pieces(case, [0, 300, case.batch.n])
    ra, rb = list(ra), list(rb)
    ta, tb, tb_off, tb_exact = gc.table(reads=ra), gc.table(reads=rb), gc.table(reads=rb, gapped=False), gc.table(reads=rb, rescued=False)
    ca, cb = gc.counts(reads=ra), gc.counts(reads=rb)
    _stage(monkeypatch, "path_first")
    al = _open(case)
    try:
        _feed(al, [b])
        al.ec_reset()                                           # the classes, the table, the gapped records in it and the stats start over
        assert _dev_table(al).ecs == [] and len(al.acov()[4]) == 0 and _no_launches(al.gap_acov_stats()) == ZERO
        _feed(al, [a])
        s1 = _assert_device(al, gc, reads=ra, passes=2)
        al.rescue_reset(); al.gap_reset()                       # the rescue and gap tables start over, the pileup stays
        al.gap_enable(8, SLOTS); al.gap_enable(3, SLOTS)        # another G and back: likewise
        al.rescue_enable(1); al.rescue_enable(2)                # another M and back: likewise
        _assert_device(al, gc, reads=ra, passes=2)
        al.gap_acov_enable(False)                               # off: no launch, the gap-placed classes off with it, the rescued records stay on
        assert al.gap_acov_stats() == dict(ZERO, launches=s1["launches"]) and al.gap_ec_stats()["reads"] == 0
        assert al.rescue_acov_stats()["log_rows"] > 0
        _feed(al, [b])
        assert al.gap_acov_stats() == dict(ZERO, launches=s1["launches"])
        _same(_dev_table(al), merge_tables([ta, tb_off]))
        _refused(al.gap_ec_enable, -10, "assigned coverage")    # the old refusal stands while the feature is off
        al.gap_acov_enable()                                    # on again: the table stays, the counts of the gapped start from zero
        _feed(al, [b])
        _same(_dev_table(al), merge_tables([ta, tb_off, tb]))
        st = al.gap_acov_stats()
        assert (st["placements"], st["records"], st["host_records"]) == (cb["placements"], cb["records"], cb["host_records"]) and st["launches"] >= s1["launches"] + 4, st
        al.acov_reset()                                         # the table and the gapped records' stats; the classes stay
        assert len(al.acov()[4]) == 0 and _no_launches(al.gap_acov_stats()) == ZERO and len(_dev_table(al).ecs) == len(merge_tables([ta, tb]).ecs)
        launches = al.gap_acov_stats()["launches"]

        def again():                                            # everything on again, from an empty table
            al.acov_enable(); al.rescue_enable(2); al.gap_enable(3, SLOTS); al.rescue_acov_enable(min_slots=ROOM); al.gap_acov_enable()
            al.ec_reset()

        def is_off(table):
            assert al.gap_acov_stats() == dict(ZERO, launches=launches) and al.gap_ec_stats()["reads"] == 0
            if table is not None:
                al.ec_reset()
                _feed(al, [b])
                _same(_dev_table(al), table)
                assert al.gap_acov_stats() == dict(ZERO, launches=launches)

        al.gap_enable(0); is_off(tb_off); again()               # gapped rescue off
        al.gap_ec_enable(False); is_off(tb_off); again()        # the gap-placed classes off
        al.rescue_acov_enable(False); is_off(tb_exact); again() # the rescued reads in assigned coverage off (the rescued classes with them)
        al.rescue_ec_enable(False); is_off(tb_exact); again()   # the rescued classes off
        al.rescue_enable(0); is_off(tb_exact); again()          # mismatch rescue off
        al.acov_enable(False); is_off(None); again()            # assigned coverage off
        al.ec_enable(False); is_off(None); again()              # the classes off
        _feed(al, [b])
        st = al.gap_acov_stats()
        _same(_dev_table(al), tb)
        assert (st["placements"], st["records"]) == (cb["placements"], cb["records"]) and st["launches"] == launches + 4, st
    finally:
        al.close()


@pytest.mark.gpu
def test_every_refusal_in_both_orders(case, gc, hip_lib, monkeypatch):
    _stage(monkeypatch, "path_first")
    al = device.Aligner(case.index, threshold=THR, memo_budget_mb=device.MEMO_OFF, max_read_len=256, max_batch_reads=max(1024, case.batch.n))
    try:
        _refused(al.gap_acov_enable, -9, "gapped rescue is off")                    # GROOT_E_STATE: nothing is on
        al.gap_acov_enable(False)                                                    # off while off: nothing to do
        al.acov_enable(); al.rescue_enable(2); al.rescue_acov_enable(min_slots=ROOM)
        _refused(al.gap_acov_enable, -9, "gapped rescue is off")                    # the rescued reads in assigned coverage alone
        al.rescue_acov_enable(False); al.gap_enable(3, SLOTS)
        _refused(al.gap_acov_enable, -9, "rescued reads in assigned coverage are off")      # gapped rescue alone
        al.acov_enable(False); al.rescue_ec_enable(); al.gap_ec_enable()             # the gap-placed classes without the pileup
        _refused(al.gap_acov_enable, -9, "rescued reads in assigned coverage are off")
        assert al.gap_acov_stats() == dict(ZERO, launches=0)                         # nothing left behind
        # the old refusals between the two enables, in both orders, with their texts
        _refused(al.rescue_acov_enable, -10, "gap-placed reads in the equivalence classes are not supported: the pileup has no rule for a gapped record")
        al.gap_ec_enable(False); al.rescue_ec_enable(False)
        al.acov_enable(); al.rescue_acov_enable(min_slots=ROOM)
        _refused(al.gap_ec_enable, -10, "rescued reads in assigned coverage are not supported: the pileup has no rule for a gapped record, and a DEL covers two intervals")
        al.gap_acov_enable()                                                         # the one way both run together
        al.gap_acov_enable(); al.rescue_acov_enable(min_slots=ROOM); al.gap_ec_enable()      # each of the three again: nothing to do
        _refused(al.pairs_enable, -10, "assigned coverage")
        al.submit(case.batch.seq, case.batch.off, first_read_id=0)
        _refused(lambda: al.gap_acov_enable(False), -9, "in flight")
        _refused(al.gap_acov_enable, -9, "in flight")
        al.wait()
        _assert_device(al, gc, passes=1)                                             # none of the refusals left anything behind
    finally:
        al.close()


@pytest.mark.gpu
def test_everything_else_is_unchanged(case, gc, hip_lib, monkeypatch):
    """records, coverage, shared reads, the rescue and gap tables, events, their stats and the rescued reads' stats with the feature on ==
    without it; without it the table is that of the rescued reads in assigned coverage and none of its kernels is launched"""
    _stage(monkeypatch, "path_first")
    got = []
    for on in (False, True):
        al = _open(case, on=on)
        try:
            al.coverage_enable(); al.shared_enable()
            al.submit(case.batch.seq, case.batch.off, first_read_id=0)
            counts = al.wait()
            alns = al.alns()
            order = np.lexsort([alns[f] for f in reversed(alns.dtype.names)])
            got.append((counts, alns[order].tolist(), al.coverage(), al.shared(), al.shared_stats(), al.rescue(), al.rescue_stats(), al.gap()[0], al.gap()[1].tolist(),
                        al.gap_stats(), _no_launches(al.rescue_ec_stats()), al.rescue_acov_stats()))
            if on:
                _assert_device(al, gc, passes=1)
            else:
                _same(_dev_table(al), gc.table(gapped=False))
                assert al.gap_acov_stats() == dict(ZERO, launches=0) and al.gap_ec_stats() == dict(reads=0, slow_reads=0, launches=0)
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)
