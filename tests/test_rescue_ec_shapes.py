"""Rescued reads in the equivalence classes (kernels_rescue_ec.hpp) at the shapes tests/test_rescue_ec.py does not reach, against the same
brute force (tests/rescue_sets_def.py); the index and the reads are in tests/rescue_sets_shapes_case.py, and
tests/test_rescue_calls_shapes.py puts every input class at its floor on the CPU:

    path_words == 1  RescueRow's row arithmetic with one mask word per segment;
    repeats         up to 100 kept placements of one read, in two graphs and on both paths of each: the (segment, word) in hand changes
                    with every occurrence list, and forced into the slow path (GROOT_TEST_SHARED_SLOW) rescue_ec_slow_kernel walks them
                    again through rescue_each_kept and ORs them into a bitmap;
    long reads      RescueRow through up to 32 blocks x 2 strands of one read;
    a text-less path  {gap, full} and {gap} are ECs of exact reads only, {full} of rescued and exact ones;
    a full buffer   max_batch_reads candidates of max_batch_bases bases: dstar[n_reads] and a row per read.

Every comparison is exact."""
import numpy as np
import pytest

import rescue_sets_shapes_case as shapes
from rescue_sets_def import ecs_plus
from test_abundance import _dev_ecs, ecs_of_alns
from test_counter_edges import _feed, _feed_pipelined, _of_reads
from test_coverage import STAGES, _stage
from test_rescue import _plain
from test_rescue_ec import FLOOR, _assert_device, _open, _sum
from test_rescue_shapes import _candidates_only


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    """(rescue_sets_shapes_case.Sets of the batch, {path name: global path}, {path name: text})"""
    return shapes.build(tmp_path_factory)


def _on(c, M=2, **kw):
    return _open(c, M, max_read_len=512, **kw)


# ---- CPU: the definition alone --------------------------------------------------------------------------------------------------------------

def test_inputs_hold_every_class(case):
    """the ECs of the definition == the oracle's records' ECs plus the rescued sets; sets in two graphs, rescued-only ECs and ECs of both
    kinds (the floors of the pileup's classes are in test_rescue_calls_shapes.py)"""
    c, paths, T = case
    gap, full = paths["gap"], paths["full"]
    for M in (1, 2, 3):
        res, left = c.rescued(M)
        ex = c.exact()
        assert not set(res) & set(ex) and not set(left) & set(ex)                   # a candidate has no record
        want = dict(ecs_of_alns(c.batch.want(c.index).alns))
        for r in res.values():
            want[r.paths] = want.get(r.paths, 0) + 1
        ecs, added, slow, mapped, mapped_slow = c.expect(M)
        assert ecs == want == ecs_plus(ex, res) and (added, slow, mapped, mapped_slow) == (len(res), 0, len(ex), 0)
        forced = c.expect(M, max_segs=1)
        per_graphs = np.bincount([c.graphs_of(r.paths) for r in res.values()], minlength=3)
        print("M =", M, "rescued", len(res), "left", len(left), "sets by graphs", per_graphs.tolist(), "ECs", ecs, "forced slow", forced[2], forced[4])
        assert per_graphs[1] >= FLOOR and per_graphs[2] >= FLOOR and len(per_graphs) == 3 and forced[2] == per_graphs[2] and forced[4] >= FLOOR
        exact_sets = set(ex.values())
        assert sum(r.paths in exact_sets for r in res.values()) >= FLOOR and sum(r.paths not in exact_sets for r in res.values()) >= FLOOR
        assert sum(len(r.paths) == 4 and r.kept >= 64 for r in res.values()) >= (FLOOR if M < 3 else 0)      # 16 and more on each of four paths
        assert sum(len(c.reads[i]) > 256 for i in res) >= FLOOR and len(left) >= FLOOR
        assert ecs[(gap, full)] >= FLOOR and ecs[(gap,)] >= FLOOR and not any(gap in r.paths for r in res.values())
        assert sum(r.paths == (full,) for r in res.values()) >= FLOOR and sum(s == (full,) for s in ex.values()) >= FLOOR


# ---- the device side -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 3])
def test_every_shape_at_once(case, hip_lib, monkeypatch, M):
    c = case[0]
    assert c.batch.n < 4000
    _stage(monkeypatch, "path_first")
    al = _on(c, M)
    try:
        _feed(al, [c.batch])
        _assert_device(al, c.expect(M), passes=1)
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
        _assert_device(al, c.expect(2), passes=1)
    finally:
        al.close()


@pytest.mark.gpu
def test_forced_slow_repeats_through_bitmap(case, hip_lib, monkeypatch):
    """GROOT_TEST_SHARED_SLOW: the reads of the repeats have their sets in two graphs and go through rescue_ec_slow_kernel, which walks up
    to 100 kept placements of a read into one bitmap; the ECs are those of the unforced run"""
    c = case[0]
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    want = c.expect(2, max_segs=1)
    assert want[2] >= 16 * FLOOR and want[4] >= FLOOR and want[0] == c.expect(2)[0]
    al = _on(c)
    try:
        _feed(al, [c.batch])
        _assert_device(al, want, passes=1)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("small", [False, True])
def test_pieces_in_flight(case, hip_lib, monkeypatch, small):
    """five pieces, one of long reads only, three in flight: the ECs of the whole batch -- and with a piece in front that outgrows the
    buffers of GROOT_TEST_SMALL_BUFFERS: its pass is redone at collect, launches the kernels again, and its rescued reads count once"""
    c = case[0]
    pieces, want = shapes.five_pieces(c), c.expect(2)
    if small:
        f = shapes.redone_piece(c)
        pieces.insert(0, f.batch)
        want = (_sum(want[0], f.expect(2)[0]),) + tuple(x + y for x, y in zip(want[1:], f.expect(2)[1:]))
    _stage(monkeypatch, "path_first")
    launches = []
    for tiny in (False, True)[:1 + small]:
        if tiny:
            monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
        al = _on(c, pipeline_depth=3)
        try:
            assert _feed_pipelined(al, pieces) == [0] * len(pieces)
            launches.append(_assert_device(al, want, passes=len(pieces))["launches"])
        finally:
            al.close()
    assert not small or launches[1] > launches[0], launches


@pytest.mark.gpu
def test_batch_that_fills_the_buffer(case, hip_lib, monkeypatch):
    """max_batch_reads candidates of exactly max_batch_bases bases, none with a record: dstar[n_reads], a row per read and
    n = min(*n_cand, n_reads) at equality"""
    c, paths, T = case
    n = 1024
    full, t = _candidates_only(c.index, T["l0"], n)
    f = c.of(full)
    want = f.expect(2)
    assert want[1] == t.stats["rescued"] >= 100 and want[3] == 0 and len(want[0]) >= 2
    _stage(monkeypatch, "path_first")
    al = _on(f, max_batch_reads=n, max_batch_bases=int(full.off[-1]))
    try:
        assert al.params.max_batch_reads == n and al.params.max_batch_bases == int(np.diff(full.off.astype(np.int64)).sum())
        _feed(al, [full])
        assert _assert_device(al, want, passes=1)["rows"] == n
        assert al.rescue_stats()["candidates"] == n
    finally:
        al.close()


@pytest.mark.gpu
def test_two_ctxs_sum_over_a_textless_path(case, hip_lib, monkeypatch):
    """two halves on two contexts: the ECs sum by set to those of the whole batch; {gap, full} and {gap} count exact reads only"""
    c, paths, T = case
    half = c.batch.n // 2
    a, b = _of_reads("a", c.reads[:half]), _of_reads("b", c.reads[half:])
    wa, wb, whole = c.expect(2, range(half)), c.expect(2, range(half, c.batch.n)), c.expect(2)
    _stage(monkeypatch, "path_first")
    al, al2 = _on(c), _on(c)
    try:
        _feed(al, [a])
        _feed(al2, [b])
        s1 = _assert_device(al, wa, passes=1)
        s2 = _assert_device(al2, wb, passes=1)
        ecs = _sum(dict(_dev_ecs(al)), dict(_dev_ecs(al2)))
        assert ecs == whole[0] and s1["reads"] + s2["reads"] == whole[1]
        exact = c.expect(2, on=False)[0]
        for s in ((paths["gap"], paths["full"]), (paths["gap"],)):
            assert ecs[s] == exact[s] >= FLOOR
        assert ecs[(paths["full"],)] >= exact[(paths["full"],)] + FLOOR
    finally:
        al.close()
        al2.close()


@pytest.mark.gpu
def test_everything_else_is_unchanged(case, hip_lib, monkeypatch):
    """coverage, shared reads, the rescue tables, the gap tables, their stats and the records with the feature on == without it"""
    c = case[0]
    _stage(monkeypatch, "path_first")
    got = []
    for on in (False, True):
        al = _on(c, on=False)
        try:
            al.coverage_enable(); al.shared_enable(); al.gap_enable(3)
            if on:
                al.rescue_ec_enable()
            al.submit(c.batch.seq, c.batch.off, first_read_id=0)
            counts = al.wait()
            alns = al.alns()
            order = np.lexsort([alns[f] for f in reversed(alns.dtype.names)])
            got.append((counts, alns[order].tolist(), al.coverage(), al.shared(), al.shared_stats(), al.rescue(), al.rescue_stats(), al.gap()[0], al.gap()[1].tolist(),
                        al.gap_stats()))
            if on:
                _assert_device(al, c.expect(2), passes=1)
        finally:
            al.close()
    for x, y in zip(*got):
        assert _plain(x) == _plain(y)
