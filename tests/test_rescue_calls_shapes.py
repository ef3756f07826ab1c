"""Rescued reads in assigned coverage (kernels_rescue_acov.hpp) at the shapes tests/test_rescue_calls.py does not reach, against the same
brute force (tests/rescue_calls_def.py); the index and the reads are in tests/rescue_sets_shapes_case.py:

    repeats         tandem repeats of period 1, 3, 16 and 20: rescue_acov_kernel and the slow walk find a read's kept placements through
                    rescue_each_kept, a second copy of rescue_place's second sweep, and a placement that two blocks anchor must be ONE
                    record there too (a duplicate is n(e, p, X, last), `records` and the --calls depth one too high); keys 0, 0xAAAAAAAA
                    and 0xFFFFFFFF, many occurrences of one key in one path, every block of a read under one key;
    many placements  25 kept placements of one read on each of four paths, and dozens of reads with the same 100 tuples: one new key claimed
                    by many threads at once and one slot added to by all of them; forced into the slow path, dozens of log entries per read;
    long reads      up to 512 bases (16 words, 32 blocks): rd[j >> 1], w0 and x + len - 1 in the key;
    a text-less path  {gap, full} and {gap} are ECs of exact reads, {full} of rescued and exact ones: the pileup of `full` mixes both kinds,
                    and no rescued record lies on `gap`;
    short paths     the path of 46 bases filled exactly at M = 1: X = 0, last = path_len - 1;
    path_words == 1 and a full buffer: max_batch_reads candidates of max_batch_bases bases.

The definition's tuple counts, measured on the CPU: 1 717 (M = 1), 2 268 (M = 2) and 1 803 (M = 3) tuples for the batch of every class,
so min_slots -- the smallest power of two that leaves half the table free -- is 4 096, 8 192 and 4 096; every test computes its own from
the table it expects (_slots).  Every comparison is exact."""
import numpy as np
import pytest

import rescue_sets_shapes_case as shapes
from groot_amd import host
from rescue_calls_def import table_of
from rescue_def import _rc
from rescue_sets_def import Rescued
from test_abundance import _dev_ecs
from test_calls import Table, _group, merge_tables
from test_counter_edges import _feed, _feed_pipelined, _of_reads
from test_coverage import STAGES, _stage
from test_rescue import _plain
from test_rescue_calls import _assert_device, _open, _same
from test_rescue_calls_def import _hand
from test_rescue_ec import FLOOR
from test_rescue_shapes import SHIFTED, _candidates_only

TUPLES = {1: 1717, 2: 2268, 3: 1803}       # the definition's, as the module's text says (test_inputs_hold_every_class keeps them true)


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    """(rescue_sets_shapes_case.Sets of the batch, {path name: global path}, {path name: text})"""
    return shapes.build(tmp_path_factory)


def _slots(table):
    """the smallest power of two >= twice the tuples of the table: the table doubles when it is more than half full, and a batch's rescued
    tuples must fit the free half"""
    return 1 << max(3, (2 * len(table.n) - 1).bit_length())


def _on(c, M=2, min_slots=None, **kw):
    return _open(c, M, min_slots=min_slots or _slots(c.table(M)), max_read_len=512, **kw)


# ---- CPU: the definition alone --------------------------------------------------------------------------------------------------------------

def test_brute_force_on_a_hand_made_repeat(case):
    """path 0 = U . W W W W . V with a word W of 16 bases, first Position 3; the read is W' W W with one substitution in W' (block 0), M = 1.
    It lies at the first W and one period on (W' over W: distance 1); a third copy would hang over V.  Blocks 1 and 2 are error-free at
    both, under one key: two blocks anchor each placement, and each is ONE record -- two tuples with n = 1, not n = 2"""
    c = case[0]
    u, w, v = b"GGATCCTTAGGCATTGACCG", b"ACGTTGCAAGGCTTAC", b"TTGACCGTAAGC"
    text = u + w * 4 + v
    assert len(text) == 96 and w[5:6] == b"G"
    read = w[:5] + b"T" + w[6:] + w * 2
    for strand, r in enumerate((read, _rc(read))):              # (the reverse complement of the read: the same placements on strand 1)
        res, rec = _hand(c, [(text, 3)], [99], [r])
        assert res[0] == Rescued(1, (0,), frozenset({strand}), 2, True)
        assert rec[0].tolist() == [[0, 23, 70, strand], [0, 39, 86, strand]]        # X = 3 + 20 and 3 + 36, last = X + 47
        assert shapes.clean_blocks([(text, 3)], rec[0], r) == [2, 2]
        tab = table_of({}, np.zeros((0, 4), dtype=np.int64), res, rec)
        assert tab.ecs == [((0,), 1)]
        assert tab.rows.tolist() == [[0, 0, 23, 70], [0, 0, 39, 86]] and tab.n.tolist() == [1, 1]


def test_inputs_hold_every_class(case):
    c, paths, T = case
    assert c.batch.n < 4000
    counts = {M: shapes.classes(c, paths, M) for M in (1, 2, 3)}
    for M in (1, 2, 3):
        print("M =", M, counts[M], "records", c.n_records(M), "forced slow", c.n_records(M, max_segs=1), "tuples", c.n_tuples(M),
              "of them exact", len(c.table(M, on=False).n), "min_slots", _slots(c.table(M)))
    assert {M: c.n_tuples(M) for M in (1, 2, 3)} == TUPLES
    k = counts[2]
    for name in SHIFTED:                                         # two or more kept placements in one (path, strand)
        assert k["shifted/" + name] >= FLOOR, (name, k)
    assert k["many_on_one_path"] >= FLOOR and k["contended_tuples"] >= FLOOR and k["most_reads_on_one_tuple"] >= FLOOR, k
    assert k["long"] >= FLOOR and k["fewest_of_a_long_length"] >= 8, k
    assert k["exact_on_textless"] >= FLOOR and k["exact_on_both"] >= FLOOR and k["exact_on_textless_only"] >= FLOOR, k
    assert k["rescued_on_full_only"] >= FLOOR and k["exact_on_full_only"] >= FLOOR and k["rescued_on_textless"] == 0, k
    assert counts[1]["fills_p46"] >= FLOOR and k["fills_p46"] == 0, (counts[1], k)      # (46 bases are too few for M = 2)
    assert k["at_the_start_of_a_long_path"] >= FLOOR and k["at_the_end_of_a_long_path"] >= FLOOR, k
    assert k["in_rescued_only_ecs"] >= FLOOR and k["in_ecs_with_exact_reads"] >= FLOOR and k["rescued_only_ecs"] >= 2 and k["ecs_of_both"] >= 2, k
    assert k["two_graphs"] >= FLOOR and k["two_graphs_exact"] >= FLOOR, k
    for M in (1, 3):                                             # the other thresholds keep what they can hold (a read of 48 bases is too short for M = 3)
        assert counts[M]["long"] >= FLOOR and counts[M]["fewest_of_a_long_length"] >= 8 and counts[M]["two_graphs"] >= FLOOR, (M, counts[M])
        assert counts[M]["rescued_on_full_only"] >= FLOOR and counts[M]["shifted/homopolymer"] >= 10, (M, counts[M])
    assert counts[1]["many_on_one_path"] >= FLOOR and counts[1]["contended_tuples"] >= FLOOR, counts[1]
    # the ECs {gap, full} and {full} of one graph: the first of exact reads only, and (EC, full) rows of both kinds
    gap, full = paths["gap"], paths["full"]
    tab, exact = c.table(2), c.table(2, on=False)
    ecs = [ids for ids, _ in tab.ecs]
    assert (gap, full) in ecs and (full,) in ecs and (gap,) in ecs
    rows_of = lambda t, ids: t.rows[t.rows[:, 0] == [x for x, _ in t.ecs].index(ids)]
    both, both_exact = rows_of(tab, (gap, full)), rows_of(exact, (gap, full))
    assert np.array_equal(both[:, 1:], both_exact[:, 1:]) and set(both[:, 1].tolist()) == {gap, full}
    assert len(rows_of(tab, (full,))) > len(rows_of(exact, (full,))) > 0 and set(rows_of(tab, (full,))[:, 1].tolist()) == {full}
    assert int(tab.n.sum()) == len(c.rows()) + c.n_records(2)[0]
    # the forced slow path: sets in two graphs, and their placements in the log
    assert c.n_records(2, max_segs=1)[1] >= 16 * FLOOR and c.n_records(2)[1] == 0
    assert c.expect(2, max_segs=1)[2] >= 4 * FLOOR and c.expect(2)[2] == 0


def test_a_count_per_anchoring_block_differs(case):
    """the discrimination check: a wrong brute force that counts a kept placement once per error-free block of the read there (what
    rescue_each_kept would do without the count-once rule of rescue_distance's `j`) differs from the definition on the reads of this
    batch, in every repeat class and in the table as a whole"""
    c, paths, T = case
    texts = c._tables.texts
    res, rec = c.rescued(2)[0], c.records(2)

    def wrong_records(i):
        """a row per (placement, error-free block)"""
        return np.repeat(rec[i], shapes.clean_blocks(texts, rec[i], c.reads[i]), axis=0)

    differ = [i for i in rec if len(wrong_records(i)) != len(rec[i])]
    by_class = {}
    for i in differ:
        by_class[c.names[i]] = by_class.get(c.names[i], 0) + 1
    print("reads on which the wrong count differs", len(differ), "of", len(rec), by_class)
    assert len(differ) >= FLOOR
    # (period16/keep2 at 48 bases has a substitution in blocks 0 and 1: one block anchors its placements, and no count can go wrong there)
    for name in tuple(x for x in SHIFTED if x != "period16/keep2") + ("many", "long", "long/pos", "full", "short"):
        assert by_class.get(name, 0) >= FLOOR, (name, by_class)
    assert all(min(shapes.clean_blocks(texts, rec[i], c.reads[i])) >= 1 for i in rec)      # (d* <= M < the blocks of a candidate: one is clean)
    want = c.table(2)
    index = {ids: e for e, (ids, _) in enumerate(want.ecs)}
    rows = [np.column_stack([np.full(len(w), index[res[i].paths]), w[:, :3]]) for i in rec for w in [wrong_records(i)]]
    ex = c.table(2, on=False)
    ex_rows = ex.rows.copy()
    ex_rows[:, 0] = np.array([index[ids] for ids, _ in ex.ecs])[ex.rows[:, 0]]      # (the exact records, under the ECs' numbers in the whole table)
    wrong = Table(want.ecs, *_group(np.concatenate(rows + [ex_rows]), np.concatenate([np.ones(sum(map(len, rows)), dtype=np.int64), ex.n])))
    assert np.array_equal(wrong.rows, want.rows) and int((wrong.n != want.n).sum()) >= 16 * FLOOR      # the same tuples, other counts
    assert int(wrong.n.sum()) - int(want.n.sum()) == sum(len(wrong_records(i)) - len(rec[i]) for i in rec)


# ---- the device side -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 3])
def test_every_shape_at_once(case, hip_lib, monkeypatch, M):
    c = case[0]
    assert c.batch.n < 4000
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_ACOV_SLOTS", "8")            # the table starts small: min_slots is what holds the batch
    al = _on(c, M)
    try:
        assert al.acov_stats()["slots"] == _slots(c.table(M))
        _feed(al, [c.batch])
        assert al.acov_stats()["slots"] == _slots(c.table(M))   # (less than half full behind the batch: collect did not grow it)
        _assert_device(al, c.table(M), c.n_records(M), passes=1)
        assert dict(_dev_ecs(al)) == c.expect(M)[0]
        st = al.rescue_ec_stats()
        assert (st["reads"], st["slow_reads"]) == c.expect(M)[1:3], st
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_under_every_align_stage(case, hip_lib, monkeypatch, stage):
    c = case[0]
    _stage(monkeypatch, stage)
    al = _on(c)
    try:
        _feed(al, [c.batch])
        _assert_device(al, c.table(2), c.n_records(2), passes=1)
    finally:
        al.close()


@pytest.mark.gpu
def test_forced_slow_repeats_through_bitmap_and_log(case, hip_lib, monkeypatch):
    """GROOT_TEST_SHARED_SLOW: the reads of the repeats have their sets in two graphs and go through rescue_acov_slow_kernel -- a bitmap
    each and a log entry per kept placement, up to 100 per read -- and the host folds the log; the table is that of the unforced run"""
    c = case[0]
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    records = c.n_records(2, max_segs=1)
    assert records[1] >= 16 * FLOOR and c.n_records(2)[1] == 0
    al = _on(c)
    try:
        _feed(al, [c.batch])
        st = _assert_device(al, c.table(2), records, passes=1)
        assert st["host_records"] == records[1]
        assert dict(_dev_ecs(al)) == c.expect(2)[0]
        st = al.rescue_ec_stats()
        assert (st["reads"], st["slow_reads"]) == c.expect(2, max_segs=1)[1:3], st
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pieces_in_flight(case, hip_lib, monkeypatch, small):
    """five pieces, one of long reads only, three in flight: the table of the whole batch -- and with a piece in front that outgrows the
    buffers of GROOT_TEST_SMALL_BUFFERS: its pass is redone at collect, launches the kernels again, and its rescued records count once"""
    c = case[0]
    pieces, want, records = shapes.five_pieces(c), c.table(2), c.n_records(2)
    if small:
        f = shapes.redone_piece(c)
        pieces.insert(0, f.batch)
        want, records = merge_tables([want, f.table(2)]), tuple(x + y for x, y in zip(records, f.n_records(2)))
    _stage(monkeypatch, "path_first")
    launches = []
    for tiny in (False, True)[:1 + small]:
        if tiny:
            monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
        al = _on(c, min_slots=_slots(want), pipeline_depth=3)
        try:
            assert _feed_pipelined(al, pieces) == [0] * len(pieces)
            launches.append(_assert_device(al, want, records, passes=len(pieces))["launches"])
        finally:
            al.close()
    assert not small or launches[1] > launches[0], launches


@pytest.mark.gpu
def test_batch_that_fills_the_buffer(case, hip_lib, monkeypatch):
    """max_batch_reads candidates of exactly max_batch_bases bases, none with a record: cand_ser[n_reads], dstar[n_reads], a row per read and
    n = min(*n_cand, n_reads) at equality"""
    c, paths, T = case
    n = 1024
    full, t = _candidates_only(c.index, T["l0"], n)
    f = c.of(full)
    want, records = f.table(2), f.n_records(2)
    assert not f.exact() and records[0] >= t.stats["rescued"] >= 100 and len(want.ecs) >= 2
    _stage(monkeypatch, "path_first")
    al = _on(f, max_batch_reads=n, max_batch_bases=int(full.off[-1]))
    try:
        assert al.params.max_batch_reads == n and al.params.max_batch_bases == int(np.diff(full.off.astype(np.int64)).sum())
        _feed(al, [full])
        _assert_device(al, want, records, passes=1)
        assert dict(_dev_ecs(al)) == f.expect(2)[0]
        st, es = al.rescue_stats(), al.rescue_ec_stats()
        assert st["candidates"] == n and st["rescued"] == t.stats["rescued"] == es["reads"] and es["slow_reads"] == 0, (st, es, t.stats)
    finally:
        al.close()


@pytest.mark.gpu
def test_two_ctxs_merge_over_a_textless_path(case, hip_lib, monkeypatch):
    """two halves on two contexts: host.acov_merge of the two exports is the table of the whole batch and the ECs sum by set; no rescued
    record lies on `gap` (its tuples are the exact reads'), and the EC {gap, full} carries exact records only"""
    c, paths, T = case
    half = c.batch.n // 2
    ra, rb = range(half), range(half, c.batch.n)
    a, b = _of_reads("a", c.reads[:half]), _of_reads("b", c.reads[half:])
    whole, exact = c.table(2), c.table(2, on=False)
    _stage(monkeypatch, "path_first")
    al, al2 = _on(c), _on(c)
    try:
        _feed(al, [a])
        _feed(al2, [b])
        s1 = _assert_device(al, c.table(2, ra), c.n_records(2, ra), passes=1)
        s2 = _assert_device(al2, c.table(2, rb), c.n_records(2, rb), passes=1)
        assert (s1["records"] + s2["records"], s1["host_records"] + s2["host_records"]) == c.n_records(2)
        off, ids, cnt, rows, n = host.acov_merge(c.index.view.n_paths, [al.acov(), al2.acov()])
        merged = Table([(tuple(ids[off[i]:off[i + 1]].tolist()), int(cnt[i])) for i in range(len(cnt))], rows, n)
        _same(merged, whole)
        ecs = dict(_dev_ecs(al))
        for k, v in _dev_ecs(al2):
            ecs[k] = ecs.get(k, 0) + v
        assert ecs == c.expect(2)[0] == dict(merged.ecs)
        gap, full = paths["gap"], paths["full"]
        on_gap = lambda t: (t.rows[t.rows[:, 1] == gap][:, 1:].tolist(), t.n[t.rows[:, 1] == gap].tolist())
        assert on_gap(merged) == on_gap(exact) and len(on_gap(exact)[0]) >= FLOOR
        of = lambda t: (lambda e: (t.rows[t.rows[:, 0] == e][:, 1:].tolist(), t.n[t.rows[:, 0] == e].tolist()))([x for x, _ in t.ecs].index((gap, full)))
        assert of(merged) == of(exact) and dict(merged.ecs)[(gap, full)] == dict(exact.ecs)[(gap, full)] >= FLOOR
    finally:
        al.close()
        al2.close()


@pytest.mark.gpu
def test_everything_else_is_unchanged(case, hip_lib, monkeypatch):
    """coverage, shared reads, the rescue tables, the gap tables, their stats and the records with the feature on == without it; the
    classes with it == those of the rescued reads in the classes alone"""
    c = case[0]
    _stage(monkeypatch, "path_first")
    got = []
    for on in (False, True):
        al = _open(c, M=2, on=False, acov=on, max_read_len=512)
        try:
            al.ec_enable(); al.coverage_enable(); al.shared_enable(); al.gap_enable(3)
            if on:
                al.rescue_acov_enable(min_slots=_slots(c.table(2)))
            else:
                al.rescue_ec_enable()
            al.submit(c.batch.seq, c.batch.off, first_read_id=0)
            counts = al.wait()
            alns = al.alns()
            order = np.lexsort([alns[f] for f in reversed(alns.dtype.names)])
            got.append((counts, alns[order].tolist(), al.coverage(), al.shared(), al.shared_stats(), al.rescue(), al.rescue_stats(), al.gap()[0], al.gap()[1].tolist(),
                        al.gap_stats(), _dev_ecs(al), al.ec_stats(), {k: v for k, v in al.rescue_ec_stats().items() if k != "launches"}))
            if on:
                _assert_device(al, c.table(2), c.n_records(2), passes=1)
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)
