"""Every legal combination of the rescue family's switches (rescue.hip) over one batch: mismatch rescue with or without gapped rescue,
each kind's records on or off, and the family's reads in nothing, in the equivalence classes or in assigned coverage, with or without
the gap-placed reads beside the rescued ones.  The index and the batch are those of tests/gap_ec_case.py, which holds every read class
at once; each combination is a fresh Aligner with roomy buffers.  Every output that is on equals the brute force of its definition (the
helpers of the modules that test each output alone), the pileups do not depend on what else is on, and every launch counter says how
many kernels the combination launched for its family per pass."""
from itertools import product

import pytest

import gap_def
import gap_ec_case
import gap_records_def
import rescue_records_def
import test_gap_records
import test_rescue_records
from gap_calls_def import gap_calls
from groot_amd import device
from test_abundance import _dev_ecs
from test_calls import _dev_table
from test_counter_edges import THR, _first_diff
from test_coverage import _stage
from test_gap_ec import SLOTS, _expect
from test_rescue import _plain
from test_rescue_calls import _same as _same_table

M, G = 2, 3
ROOM = 1 << 16       # record slots per batch, and slots of the assigned-coverage table: the batch's with room to spare

# Kernels a pass launches for each part of the family beyond mismatch rescue's own two (the pack and the count kernel), as rescue_launch
# counts them: the gap kernel; the scan and the emit kernel of either kind of record; slow, insert and merge of the rescued classes;
# serial, clear and add of the rescued calls; slow and insert of the gap classes; slow, serial and add of the gap calls and one more
# for the kind of kernel they make the gap kernel.
PER_PASS = {"gap": 1, "rescue_rec": 2, "gap_rec": 2, "rescue_ec": 3, "rescue_acov": 3, "gap_ec": 2, "gap_acov": 4}

# level -> the parts of the family that are on with it
LEVELS = {"none": (), "classes": ("rescue_ec",), "classes+gap": ("rescue_ec", "gap_ec"), "calls": ("rescue_ec", "rescue_acov"),
          "calls+gap": ("rescue_ec", "rescue_acov", "gap_ec", "gap_acov")}
COMBOS = [(False, rr, False, lv) for rr, lv in product((False, True), ("none", "classes", "calls"))] + \
         [(True, rr, gr, lv) for rr, gr, lv in product((False, True), (False, True), LEVELS)]
assert len(COMBOS) == 26

_PILEUPS = {}        # (M, G or None) -> the pileups of the first combination that ran with them


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return gap_ec_case.case(tmp_path_factory)


@pytest.fixture(scope="module")
def want_records(case):
    """the definition's rescued and gapped records of the batch"""
    brute = gap_def.Brute(case.index, 2, g_max=3)
    return (rescue_records_def.records(case.index, M, case.reads, case.has, case._tables),
            gap_records_def.records(case.index, M, G, brute, case.reads, case.has))


def _open(case, gap, rr, gr, level):
    al = device.Aligner(case.index, threshold=THR, memo_budget_mb=device.MEMO_OFF, max_read_len=256, max_batch_reads=max(1024, case.batch.n))
    on = LEVELS[level]
    if "rescue_acov" in on:
        al.acov_enable()
    elif on:
        al.ec_enable()
    al.rescue_enable(M)
    if gap:
        al.gap_enable(G, SLOTS)
    if "rescue_acov" in on:
        al.rescue_acov_enable(min_slots=ROOM)
        if "gap_acov" in on:
            al.gap_acov_enable()
    elif on:
        al.rescue_ec_enable()
        if "gap_ec" in on:
            al.gap_ec_enable()
    if rr:
        al.rescue_rec_enable(ROOM)
    if gr:
        al.gap_rec_enable(ROOM)
    return al


@pytest.mark.gpu
@pytest.mark.parametrize("gap,rr,gr,level", COMBOS, ids=["%s-%s%s%s" % ("gap" if g else "nogap", lv, "-rr" if rr else "", "-gr" if gr else "") for g, rr, gr, lv in COMBOS])
def test_combination(case, want_records, hip_lib, monkeypatch, gap, rr, gr, level):
    _stage(monkeypatch, "path_first")
    on = set(LEVELS[level]) | ({"gap"} if gap else set()) | ({"rescue_rec"} if rr else set()) | ({"gap_rec"} if gr else set())
    al = _open(case, gap, rr, gr, level)
    try:
        al.submit(case.batch.seq, case.batch.off, first_read_id=0)
        assert al.wait()["received"] == case.batch.n
        if rr:
            test_rescue_records._same(al.rescue_records(), want_records[0])
        if gr:
            test_gap_records._same(al.gap_records(), want_records[1])
        if "rescue_acov" in on:                                    # the classes and the tuples
            _same_table(_dev_table(al), gap_calls(case).table(M, G, gapped="gap_acov" in on))
        elif "rescue_ec" in on:
            got, want = dict(_dev_ecs(al)), _expect(case, M, G, gapped="gap_ec" in on).ecs
            assert got == want, _first_diff(got, want)
        pile = (_plain(al.rescue()),) + ((_plain(al.gap()[0]), al.gap()[1].tolist()) if gap else ())
        assert pile == _PILEUPS.setdefault((M, G if gap else None), pile)
        launches = {"gap": al.gap_stats(), "rescue_rec": al.rescue_rec_stats(), "gap_rec": al.gap_rec_stats(), "rescue_ec": al.rescue_ec_stats(),
                    "rescue_acov": al.rescue_acov_stats(), "gap_ec": al.gap_ec_stats(), "gap_acov": al.gap_acov_stats()}
        launches = {k: v["launches"] for k, v in launches.items()}
        res = al.rescue_stats()["launches"]
        assert res >= 2 and res % 2 == 0, res
        assert launches == {k: res // 2 * n if k in on else 0 for k, n in PER_PASS.items()}, (launches, res, sorted(on))
    finally:
        al.close()
