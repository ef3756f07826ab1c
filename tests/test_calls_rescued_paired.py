"""Rescued mates in assigned coverage over fragments (groot_hip_rescue_acov_pairs_*, kernels_rescue_acov_pairs.hpp) against the rule in
plain Python (tests/calls_rescued_pairs_def.py): the device's table, its ECs and every stat == the definition, integers throughout.

The batches are those of test_calls_rescued_paired_def.py, which puts every kind of record at its floor on the CPU: the fragments of
test_rescue_pairs._CaseA (about 1 400 mates, every class of fragment) and test_paired's case (b) with one mate rescued (a graph both
mates share whose AND is empty).  Every expectation comes from the CPU oracle's records and the brute forces, never from device output."""
import numpy as np
import pytest

from calls_rescued_pairs_def import STATS, Want
from groot_amd import device, host
from test_calls import Table, _dev_table, merge_tables
from test_calls_rescued_paired_def import FLOOR, CallsFrags, calls_a, calls_b      # noqa: F401  (fixtures)
from test_counter_edges import THR, _feed, _feed_pipelined, _of_reads
from test_coverage import STAGES, _stage
from test_rescue import _plain
from test_rescue_ec import _refused
from test_rescue_pairs import _Frags, _assert_device as _assert_units, _total as _total_units, case_a, case_b      # noqa: F401  (fixtures)

ROOM = 1 << 17      # slots that hold the batch's tuples (about 26 000 under M = 1) with half the table free
LOG = (8 << 20) // 16


def _open(c, M=1, on=True, min_slots=ROOM, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    kw.setdefault("max_batch_reads", max(1024, c.n))
    al = device.Aligner(c.index, threshold=THR, **kw)
    if M:
        al.rescue_enable(M)
    if on:
        al.rescue_acov_pairs_enable(min_slots=min_slots)
    return al


def _total(wants):
    """what several batches add up to"""
    if len(wants) == 1:
        return wants[0]
    kinds = {}
    for w in wants:
        for k, v in w.kinds.items():
            kinds[k] = kinds.get(k, 0) + v
    return Want(merge_tables([w.table for w in wants]), _total_units([w.units for w in wants]), None, {k: sum(w.stats[k] for w in wants) for k in STATS},
                sum(w.log for w in wants), sum(w.ee_left for w in wants), kinds, None)


def _same(got, want):
    assert got.ecs == want.ecs, [x for x in zip(got.ecs, want.ecs) if x[0] != x[1]][:5]
    assert got.rows.shape == want.rows.shape, (got.rows.shape, want.rows.shape)
    bad = np.flatnonzero((got.rows != want.rows).any(axis=1))[:5]
    assert not len(bad), (got.rows[bad], want.rows[bad])
    assert np.array_equal(got.n, want.n), (np.flatnonzero(got.n != want.n)[:10], got.rows[got.n != want.n][:5], got.n[got.n != want.n][:5], want.n[got.n != want.n][:5])


def _assert_device(al, w, passes=None):
    """the table, the classes with every stat of the rescued mates' rule, and the record counts of this rule"""
    _same(_dev_table(al), w.table)
    _assert_units(al, w.units)
    st, ast, ps = al.rescue_acov_pairs_stats(), al.acov_stats(), al.acov_pairs_stats()
    print("rescue_acov_pairs", st, "acov", ast, "acov_pairs", ps)
    assert {k: st[k] for k in STATS} == w.stats and st["dropped"] == 0, (st, w.stats)
    assert ast["records"] == ps["records"] == int(w.table.n.sum()) and ast["tuples"] == len(w.table.n), (ast, ps, int(w.table.n.sum()), len(w.table.n))
    assert ps["left_out"] == w.ee_left, (ps, w.ee_left)
    # three kernels per pass behind the merge (a pass that collect redoes launches them again; they return at once in the pass that is not counted)
    assert st["launches"] % 3 == 0 and (passes is None or st["launches"] >= 3 * passes), (st, passes)
    return st


def _pieces(c, cuts):
    """the batch cut at the fragments `cuts` -> [(batch, its fragments)]"""
    return [(c.f.piece(a, b), range(a, b)) for a, b in zip(cuts, cuts[1:])]


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 3])
def test_every_kind_at_once(calls_a, hip_lib, monkeypatch, M):
    _stage(monkeypatch, "path_first")
    al = _open(calls_a, M)
    try:
        _feed(al, [calls_a.batch])
        st = _assert_device(al, calls_a.want(M), passes=1)
        assert st["log_rows"] == LOG and al.acov_stats()["slots"] >= ROOM
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(calls_a, calls_b, hip_lib, monkeypatch, stage, rod):
    _stage(monkeypatch, stage)
    for c in (calls_a, calls_b):
        al = _open(c, results_on_device=rod)
        try:
            _feed(al, [c.batch])
            _assert_device(al, c.want(1), passes=1)
        finally:
            al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pipelined_pieces_sum_to_the_batch(calls_a, hip_lib, monkeypatch, small):
    """the batch cut into pieces, one empty and one of a single fragment (two reads), three in flight, from an odd first_read_id -- and the
    same with GROOT_TEST_SMALL_BUFFERS and a piece with more records than the small buffers hold, which is redone at collect and counts once"""
    c = calls_a
    nf = c.n // 2
    pieces = _pieces(c, [0, 150, 150, 151, 300, nf])
    assert [p.n for p, _ in pieces][1:3] == [0, 2]
    wants, batches = [c.want(1)], [p for p, _ in pieces]
    if small:
        ex = c.exact()
        clean = [c.reads[r] for r in sorted(ex) if len(ex[r]) > 60][:80]
        extra = CallsFrags(_Frags(c.index, "mapped and not", (clean * 8)[:600] + c.reads[:200], c.f._tables))
        assert len(extra.alns()) > 20000
        wants.append(extra.want(1))
        batches.insert(4, extra.batch)
        monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    _stage(monkeypatch, "path_first")
    al = _open(c, pipeline_depth=3, min_slots=2 * ROOM)
    try:
        assert _feed_pipelined(al, batches, first=1) == [0] * len(batches)
        st = _assert_device(al, _total(wants))
        n = sum(1 for b in batches if b.n)
        assert st["launches"] > 3 * n if small else st["launches"] >= 3 * n, st
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_table_of_eight_slots_grows_at_collect_with_batches_in_flight(calls_a, hip_lib, monkeypatch, depth):
    """GROOT_TEST_ACOV_SLOTS=8, min_slots 0.  The first batch holds two fragments of an exact and a rescued mate, joined, whose one-pass
    records are four tuples at the most -- they find room in the eight slots -- and the fragments of two exact mates, whose claim runs out
    of room: collect grows the table and counts the batch again.  By then the batches behind it -- other fragments -- have overwritten the
    unit rows and the per-batch table: a redo that read a row, or counted the exact records beside a rescued partner again, would differ
    from the definition.  The other fragments follow in pieces whose tuples fit the free half of the table with the pieces in flight"""
    c = calls_a
    ex, nf = c.exact(), c.n // 2
    per = {f: c.want(1, frags=[f]) for f in range(nf)}
    ee = [f for f in range(nf) if 2 * f in ex and 2 * f + 1 in ex]
    tiny = [f for f in range(nf) if f not in ee and per[f].units.cls["joined"] and per[f].stats["exact_records"] and not per[f].log and per[f].one_pass <= 2][:2]
    assert len(tiny) == 2 and all(per[f].stats["exact_records"] >= 1 and per[f].stats["rescued_records"] >= 1 for f in tiny)
    head = [tiny + ee[:len(ee) // 2], ee[len(ee) // 2:], []]
    K = 1000
    assert len(c.want(1, frags=head[0]).table.n) > 8 * 128 and len(c.want(1, frags=head[0] + head[1]).table.n) >= 3 * K
    groups, cur, n = list(head), [], 0
    for f in range(nf):
        if f in ee or f in tiny:
            continue
        k = 0 if per[f].log else len(per[f].table.n)             # (the tuples of a fragment on bitmaps are the host's)
        assert k <= K
        if cur and n + k > K:
            groups.append(cur)
            cur, n = [], 0
        cur.append(f)
        n += k
    groups.append(cur)
    assert len(groups) >= 8
    batches = [_of_reads("group", [c.reads[r] for f in g for r in (2 * f, 2 * f + 1)]) for g in groups]
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_ACOV_SLOTS", "8")
    al = _open(c, min_slots=0, pipeline_depth=depth)
    try:
        assert al.acov_stats()["slots"] == 8
        assert _feed_pipelined(al, batches, depth=depth) == [0] * len(batches)
        _same(_dev_table(al), c.want(1).table)
        st, ast = al.rescue_acov_pairs_stats(), al.acov_stats()
        print(st, ast)
        assert {k: st[k] for k in STATS} == c.want(1).stats and st["dropped"] == 0, st
        assert ast["grows"] >= 3 and ast["slots"] > 8 * 2 ** ast["grows"], ast      # (some growths were fourfold: a claim that ran out of room, counted again)
    finally:
        al.close()


@pytest.mark.gpu
def test_a_table_too_small_drops_loudly(calls_a, hip_lib, monkeypatch):
    """eight slots and min_slots 0: the one-pass records of the batch exceed the room, and the table grows at collect only -- the export
    fails and names the knob; with a min_slots that holds the batch the same feed is exact"""
    c = calls_a
    w = c.want(1)
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_ACOV_SLOTS", "8")
    al = _open(c, min_slots=0)
    try:
        assert al.acov_stats()["slots"] == 8
        _feed(al, [c.batch])
        with pytest.raises(host.GrootError) as e:
            al.acov()
        assert e.value.code == -6 and "--callSlots" in str(e.value) and "min_slots" in str(e.value), e.value
        st = al.rescue_acov_pairs_stats()
        assert st["dropped"] > 0 and st["exact_records"] + st["rescued_records"] + st["dropped"] == w.stats["exact_records"] + w.stats["rescued_records"], st
        assert (st["exact_left_out"], st["rescued_left_out"], st["host_records"]) == (w.stats["exact_left_out"], w.stats["rescued_left_out"], w.stats["host_records"])
        al.acov_reset()                                         # the table and `dropped` start over: the export works again
        assert al.rescue_acov_pairs_stats()["dropped"] == 0 and len(al.acov()[4]) == 0
    finally:
        al.close()
    al = _open(c, min_slots=ROOM)
    try:
        assert al.acov_stats()["slots"] == ROOM
        _feed(al, [c.batch])
        _assert_device(al, w, passes=1)
    finally:
        al.close()


def _fails_alone(c, al, monkeypatch, knob, first, rest, small, w_first, w_small):
    """batch `first` counts; `rest` fails with GROOT_E_NOSPACE naming the knob and counts nothing anywhere; `small`, fed after it, counts"""
    n0 = _feed(al, [first])
    before = _assert_device(al, w_first, passes=1)
    al.submit(rest.seq, rest.off, first_read_id=n0)
    with pytest.raises(host.GrootError) as e:
        al.wait()
    assert e.value.code == -6 and knob in str(e.value), e.value
    after = _assert_device(al, w_first)                         # the table, the classes and every stat: unchanged
    assert {k: after[k] for k in after if k != "launches"} == {k: before[k] for k in before if k != "launches"}
    _feed(al, [small], first=n0)                                # and the ctx goes on
    _assert_device(al, _total([w_first, w_small]))


@pytest.mark.gpu
def test_forced_slow_mode_and_the_bitmaps(calls_a, calls_b, hip_lib, monkeypatch):
    """GROOT_TEST_SHARED_SLOW: every fragment with a mate in more than one graph goes through the bitmaps and the log.  Exactly as many
    bitmaps as the batch needs: every record counted; one fewer in a later batch: that batch fails alone"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    for c in (calls_a, calls_b):
        w = c.want(1, max_segs=1)
        assert w.log >= 10 * FLOOR and w.stats["host_records"] >= 10 * FLOOR
        monkeypatch.setenv("GROOT_TEST_RESCUE_EC_ROWS", str(w.units.bitmap_rows))
        al = _open(c)
        try:
            _feed(al, [c.batch])
            _assert_device(al, w, passes=1)
            assert al.rescue_ec_stats()["rows"] == w.units.bitmap_rows
        finally:
            al.close()
    c = calls_a
    nf = c.n // 2
    first, rest, small = c.want(1, 1, range(100)), c.want(1, 1, range(100, nf)), c.want(1, 1, range(100, 260))
    assert 0 < first.units.bitmap_rows < rest.units.bitmap_rows and 0 < small.units.bitmap_rows < rest.units.bitmap_rows
    monkeypatch.setenv("GROOT_TEST_RESCUE_EC_ROWS", str(rest.units.bitmap_rows - 1))
    al = _open(c)
    try:
        _fails_alone(c, al, monkeypatch, "GROOT_TEST_RESCUE_EC_ROWS", c.f.piece(0, 100), c.f.piece(100, nf), c.f.piece(100, 260), first, small)
    finally:
        al.close()


@pytest.mark.gpu
def test_the_size_of_the_log(calls_a, hip_lib, monkeypatch):
    """GROOT_TEST_RESCUE_ACOV_LOG: exactly as many entries as the batch's fragments on bitmaps have records: every record counted; one
    fewer in a later batch: GROOT_E_NOSPACE that names the knob, nothing of that batch counted, and the ctx goes on"""
    _stage(monkeypatch, "path_first")
    c = calls_a
    w = c.want(1)
    assert w.log >= 10 * FLOOR
    monkeypatch.setenv("GROOT_TEST_RESCUE_ACOV_LOG", str(w.log))
    al = _open(c)
    try:
        _feed(al, [c.batch])
        assert _assert_device(al, w, passes=1)["log_rows"] == w.log
    finally:
        al.close()
    nf = c.n // 2
    first, rest, small = c.want(1, 4, range(100)), c.want(1, 4, range(100, nf)), c.want(1, 4, range(100, 260))
    assert 0 < first.log < rest.log and 0 < small.log < rest.log
    monkeypatch.setenv("GROOT_TEST_RESCUE_ACOV_LOG", str(rest.log - 1))
    al = _open(c)
    try:
        _fails_alone(c, al, monkeypatch, "GROOT_TEST_RESCUE_ACOV_LOG", c.f.piece(0, 100), c.f.piece(100, nf), c.f.piece(100, 260), first, small)
    finally:
        al.close()


@pytest.mark.gpu
def test_two_ctxs_merge_to_the_table_of_one(calls_a, hip_lib, monkeypatch):
    c = calls_a
    nf = c.n // 2
    (a, ra), (b, rb) = _pieces(c, [0, 400, nf])
    _stage(monkeypatch, "path_first")
    al, al2 = _open(c), _open(c)
    try:
        _feed(al, [a])
        _feed(al2, [b])
        s1 = _assert_device(al, c.want(1, frags=ra), passes=1)
        s2 = _assert_device(al2, c.want(1, frags=rb), passes=1)
        assert {k: s1[k] + s2[k] for k in STATS} == c.want(1).stats
        off, ids, cnt, rows, n = host.acov_merge(c.index.view.n_paths, [al.acov(), al2.acov()])
        _same(Table([(tuple(ids[off[i]:off[i + 1]].tolist()), int(cnt[i])) for i in range(len(cnt))], rows, n), c.want(1).table)
    finally:
        al.close()
        al2.close()


ZERO = dict(dict.fromkeys(STATS, 0), dropped=0, log_rows=0)


@pytest.mark.gpu
def test_off_on_and_every_reset(calls_a, hip_lib, monkeypatch):
    c = calls_a
    nf = c.n // 2
    (a, ra), (b, rb) = _pieces(c, [0, 400, nf])
    wa, wb = c.want(1, frags=ra), c.want(1, frags=rb)
    _stage(monkeypatch, "path_first")
    al = _open(c)
    try:
        _feed(al, [b])
        al.ec_reset()                                           # the classes, the table, the records in it and every stat start over; the rule stays on
        st = al.rescue_acov_pairs_stats()
        assert _dev_table(al).ecs == [] and len(al.acov()[4]) == 0 and {k: st[k] for k in ZERO} == dict(ZERO, log_rows=LOG)
        _feed(al, [a])
        s1 = _assert_device(al, wa, passes=2)
        al.rescue_reset()                                       # the rescue tables start over, the pileup stays
        al.rescue_enable(2); al.rescue_enable(1)                # another M and back: likewise
        _assert_device(al, wa, passes=2)
        al.rescue_acov_pairs_enable(False)                      # off: the rule and assigned coverage go; the classes, pairing and the rescued mates' rule stay
        assert al.rescue_acov_pairs_stats() == dict(ZERO, launches=s1["launches"]) and al.acov_stats()["slots"] == 0
        assert al.rescue_ec_stats()["rows"] > 0 and al.pairs_stats() == {k: wa.units.cls[k] for k in ("joined", "split", "single")}
        _feed(al, [b])
        _assert_units(al, _total_units([wa.units, wb.units]))   # == --rescuedPaired alone
        assert al.rescue_acov_pairs_stats()["launches"] == s1["launches"]
        al.ec_reset()
        al.rescue_acov_pairs_enable(min_slots=ROOM)             # on again
        _feed(al, [b])
        s2 = _assert_device(al, wb)
        assert s2["launches"] == s1["launches"] + 3
        al.acov_reset()                                         # the table and these stats; the classes stay
        st = al.rescue_acov_pairs_stats()
        assert len(al.acov()[4]) == 0 and {k: st[k] for k in ZERO} == dict(ZERO, log_rows=LOG) and len(_dev_table(al).ecs) == len(wb.table.ecs)
        al.ec_reset()
        _feed(al, [a])
        _assert_device(al, wa)
        al.rescue_pairs_enable(False)                           # the rescued mates' rule off takes this rule with it: assigned coverage over fragments alone is left
        assert al.rescue_acov_pairs_stats()["log_rows"] == 0 and al.rescue_ec_stats()["rows"] == 0 and al.acov_stats()["slots"] >= ROOM
        al.ec_reset()
        _feed(al, [a])
        off = c.want(1, frags=ra, on=False)                     # == --calls --callsPaired
        _same(_dev_table(al), off.table)
        assert al.acov_pairs_stats()["left_out"] == off.ee_left
        al.rescue_acov_pairs_enable(min_slots=ROOM)             # from that state on again
        al.ec_reset()
        _feed(al, [c.batch])
        _assert_device(al, c.want(1))
        al.rescue_enable(0)                                     # rescue off takes the rule off too
        assert al.rescue_acov_pairs_stats()["log_rows"] == 0 and al.rescue_ec_stats()["rows"] == 0
    finally:
        al.close()


@pytest.mark.gpu
def test_every_refusal(calls_a, hip_lib, monkeypatch):
    c = calls_a
    _stage(monkeypatch, "path_first")
    al = _open(c, M=0, on=False)
    try:
        _refused(al.rescue_acov_pairs_enable, -9, "mismatch rescue is off")                        # GROOT_E_STATE
        al.rescue_acov_pairs_enable(False)                                                         # off while off: nothing
        al.rescue_enable(1)
        _refused(lambda: al.rescue_acov_pairs_enable(min_slots=3 << 10), -1, "power of two")       # GROOT_E_INVALID
        al.shared_enable()
        _refused(al.rescue_acov_pairs_enable, -10, "shared reads")                                 # GROOT_E_UNSUPPORTED
        al.shared_enable(False)
        al.gap_enable(3); al.ec_enable(); al.rescue_ec_enable(); al.gap_ec_enable()
        _refused(al.rescue_acov_pairs_enable, -10, "gap-placed reads")
        al.gap_ec_enable(False); al.rescue_ec_enable(False); al.ec_enable(False)
        assert al.rescue_acov_pairs_stats() == dict(ZERO, launches=0) and al.acov_stats()["slots"] == 0      # nothing left behind
        # the old enables refuse each other as before, word for word
        al.rescue_pairs_enable()
        _refused(al.acov_enable, -10, "assigned coverage with paired-end units is not supported")
        _refused(al.acov_pairs_enable, -10, "assigned coverage over fragments with rescued reads in the equivalence classes is not supported: mates are rescued one by one")
        al.rescue_pairs_enable(False); al.pairs_enable(False)
        al.acov_pairs_enable()
        _refused(al.rescue_pairs_enable, -10, "rescued mates in paired-end units with assigned coverage over fragments are not supported: a rescued mate has no record to weigh")
        _refused(al.rescue_ec_enable, -10, "mates are rescued one by one")
        al.acov_pairs_enable(False); al.pairs_enable(False)
        al.acov_enable()
        _refused(al.rescue_pairs_enable, -10, "rescued mates in paired-end units with assigned coverage are not supported: a rescued mate has no record to weigh")
        al.rescue_acov_enable(min_slots=ROOM)                   # from the unpaired rule of the rescued records: it goes, the rescued classes stay
        al.rescue_acov_pairs_enable(min_slots=ROOM)
        assert al.rescue_acov_stats()["log_rows"] == 0 and al.rescue_ec_stats()["rows"] > 0
        # ... and with the rule on, from whichever enable comes second
        _refused(al.shared_enable, -10, "rescued mates in paired-end units")
        _refused(al.gap_ec_enable, -10, "rescued mates in paired-end units")
        _refused(al.rescue_acov_enable, -10, "paired-end units")
        _refused(lambda: al.assign_enable(np.ones(c.index.view.n_paths)), -10, "assignment")
        _refused(al.gap_acov_enable, -9, "rescued reads in assigned coverage are off")
        al.gap_enable(0)
        al.submit(c.batch.seq, c.batch.off, first_read_id=0)
        _refused(lambda: al.rescue_acov_pairs_enable(False), -9, "in flight")
        _refused(al.rescue_acov_pairs_enable, -9, "in flight")
        al.wait()
        _assert_device(al, c.want(1), passes=1)
        al.acov_enable(False)                                   # assigned coverage off takes the rule off; the rescued mates' rule stays
        assert al.rescue_acov_pairs_stats()["log_rows"] == 0 and al.rescue_ec_stats()["rows"] > 0 and al.acov_stats()["slots"] == 0
        _refused(al.acov_enable, -10, "assigned coverage with paired-end units is not supported")      # (no way to the two without the rule)
        _refused(al.acov_pairs_enable, -10, "mates are rescued one by one")
        al.rescue_acov_pairs_enable(min_slots=ROOM)
        al.ec_enable(False)                                     # and so do the classes, with everything that stands on them
        assert al.rescue_acov_pairs_stats()["log_rows"] == 0 and al.acov_stats()["slots"] == 0 and al.rescue_ec_stats()["rows"] == 0
        al.rescue_acov_pairs_enable(min_slots=ROOM)
        al.pairs_enable(False)                                  # and pairing
        assert al.rescue_acov_pairs_stats()["log_rows"] == 0 and al.acov_stats()["slots"] == 0 and al.rescue_ec_stats()["rows"] == 0
        al.rescue_acov_pairs_enable(min_slots=ROOM)
        _feed(al, [c.batch])
        _assert_device(al, c.want(1))
    finally:
        al.close()


@pytest.mark.gpu
def test_consequences_of_the_rule(calls_a, hip_lib, monkeypatch):
    """no candidate in the batch: the table of --calls --callsPaired, and the device agrees with that rule's own run; fragments (r, r): the
    unpaired --callsRescued run's table with every n doubled, against that run on the device"""
    _stage(monkeypatch, "path_first")
    c = calls_a
    ex = c.exact()
    mapped = [c.reads[r] for r in sorted(ex)]
    plain = CallsFrags(_Frags(c.index, "no candidates", mapped[:len(mapped) & ~1], c.f._tables))
    got = []
    for rule in (True, False):
        al = _open(plain, on=rule)
        try:
            if not rule:
                al.acov_pairs_enable()
            _feed(al, [plain.batch])
            got.append((_dev_table(al), al.acov_pairs_stats()))
            if rule:
                _assert_device(al, plain.want(1), passes=1)
            else:
                assert al.rescue_acov_pairs_stats()["launches"] == 0
        finally:
            al.close()
    _same(got[0][0], got[1][0])
    assert got[0][1] == got[1][1]
    k = 600
    dbl = CallsFrags(_Frags(c.index, "doubled", [r for r in c.reads[:k] for _ in (0, 1)], c.f._tables))
    al = _open(c, on=False)
    try:
        al.acov_enable(); al.rescue_acov_enable(min_slots=ROOM)
        _feed(al, [_of_reads("originals", c.reads[:k])])
        unpaired = _dev_table(al)
    finally:
        al.close()
    al = _open(dbl)
    try:
        _feed(al, [dbl.batch])
        _assert_device(al, dbl.want(1), passes=1)
        _same(_dev_table(al), Table(unpaired.ecs, unpaired.rows, 2 * unpaired.n))
    finally:
        al.close()


@pytest.mark.gpu
def test_everything_else_is_unchanged(calls_a, hip_lib, monkeypatch):
    """records, coverage, the rescue tables and the rescued records with the rule on == with the rescued mates' rule alone"""
    _stage(monkeypatch, "path_first")
    c = calls_a
    got = []
    for on in (False, True):
        al = _open(c, M=2, on=False)
        try:
            al.coverage_enable(); al.rescue_rec_enable(1 << 18)
            if on:
                al.rescue_acov_pairs_enable(min_slots=ROOM)
            else:
                al.rescue_pairs_enable()
            al.submit(c.batch.seq, c.batch.off, first_read_id=0)
            counts = al.wait()
            alns = al.alns()
            order = np.lexsort([alns[x] for x in reversed(alns.dtype.names)])
            got.append((counts, alns[order].tolist(), al.coverage(), al.rescue(), al.rescue_stats(), al.rescue_records().tolist(), al.pairs_stats(),
                        {k: v for k, v in al.rescue_pairs_stats().items() if k != "launches"}))
            if on:
                _assert_device(al, c.want(2), passes=1)
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)
