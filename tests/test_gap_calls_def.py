"""CPU: the brute force of the gap-placed reads in assigned coverage (tests/gap_calls_def.py) on hand-worked cases with the tuples written
out, and the inputs of its device tests (tests/gap_ec_case.py) at the floors of every class the definition (include/groot_hip.h,
"gap-placed reads in assigned coverage") tells apart:

    type DEL:  TWO gapped records of r on p, covering [X, X + k* - 1] and [X + k* + g, X + len + g - 1]
    type INS:  ONE gapped record of r on p, covering [X, X + len - g - 1]          (X = first Position of p + x)"""
from collections import namedtuple

import numpy as np
import pytest

import gap_def
import gap_ec_case
from gap_calls_def import gap_calls, rows_of, table_of3
from gap_def import DEL, INS
from gap_sets_def import Gapped
from rescue_def import _rc

FLOOR = 10
M, G = 2, 3
FIRST = 5               # the first Position of the hand-made texts


def _text(seed, n):
    return bytes(np.random.default_rng(seed).choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))


def _kept(texts, read):
    brute = gap_def.Brute(None, M, texts=[(t, FIRST) for t in texts], g_max=G)
    return gap_def.keep(brute.placements(read), M, G)


def _rows(texts, read):
    e, kept = _kept(texts, read)
    return e, kept, rows_of(kept, len(read), lambda p: FIRST).tolist()


T = _text(301, 150)


def test_one_deletion_is_two_records_around_the_hole():
    assert T[60] != T[63]                                   # (the deletion cannot move to the left: k* is the planted cut)
    read = T[21:61] + T[64:104]                             # 80 bases, T[61:64] deleted: x = 21, k* = 40, g = 3
    e, kept, rows = _rows([T], read)
    assert (e, kept) == (3, [(0, 0, 21, DEL, 3, 0, 40)])
    assert rows == [[0, 26, 65], [0, 69, 108]]              # [X, X + 39] and [X + 43, X + 82], X = 5 + 21: 40 + 40 bases, the hole is 66..68
    assert _rows([T], _rc(read))[2] == rows                 # the other strand covers the same text bases


def test_one_insertion_is_one_record():
    ins = b"ACA"
    assert ins[:1] != T[60:61] and ins[2:] != T[59:60]      # (no insertion that repeats the text beside it: k* is the planted cut)
    read = T[20:60] + ins + T[60:97]                        # 80 bases, three inserted behind base 40: x = 20, k* = 40, g = 3
    e, kept, rows = _rows([T], read)
    assert (e, kept) == (3, [(0, 0, 20, INS, 3, 0, 40)])
    assert rows == [[0, 25, 101]]                           # [X, X + 80 - 3 - 1]: the 77 text bases under the read's 77 aligned bases


def test_a_deletion_whose_first_interval_is_the_anchor():
    assert T[35] != T[37]
    read = T[20:36] + T[38:102]                             # k* = 16 = A, the shortest part in front of a gap; g = 2
    e, kept, rows = _rows([T], read)
    assert (e, kept) == (2, [(0, 0, 20, DEL, 2, 0, 16)])
    assert rows == [[0, 25, 40], [0, 43, 106]]              # exactly 16 bases, then 64


def test_kept_placements_at_two_x_of_one_path():
    rep = _text(302, 100)
    text = _text(303, 12) + rep + _text(304, 14) + rep + _text(305, 12)        # the repeat at 12 and at 126
    assert rep[49] != rep[50]
    read = rep[10:50] + rep[51:91]                          # one base deleted: x = 12 + 10 and 126 + 10
    e, kept, rows = _rows([text], read)
    assert e == 1 and [pl[:5] for pl in kept] == [(0, 0, 22, DEL, 1), (0, 0, 136, DEL, 1)]
    assert [pl[6] for pl in kept] == [40, 40]
    assert rows == [[0, 27, 66], [0, 68, 107], [0, 141, 180], [0, 182, 221]]   # two records per x: the read is piled up on both copies


def test_a_gap_read_and_a_rescued_read_of_one_class_on_one_path():
    """S++ of both is (0,): one EC of two reads, whose tuples are the rescued read's one interval and the gap read's two"""
    Rescued = namedtuple("Rescued", "paths kept")
    read = T[21:61] + T[64:104]
    e, kept, rows = _rows([T], read)
    gapped = {1: Gapped(e, (0,), frozenset([0]), frozenset([DEL]), 1, False)}
    # read 0: T[25:105] with one substitution, rescued ungapped at x = 25: one rescued record [X, X + 79], X = 5 + 25 (path, X, last, strand)
    t = table_of3({}, np.zeros((0, 4), dtype=np.int64), {0: Rescued((0,), 1)}, {0: np.array([[0, 30, 109, 0]])}, gapped, {1: np.array(rows)}, {1: kept})
    assert t.ecs == [((0,), 2)]
    assert t.rows.tolist() == [[0, 0, 26, 65], [0, 0, 30, 109], [0, 0, 69, 108]] and t.n.tolist() == [1, 1, 1]
    # the same gap read twice: counts of 2, no new tuple
    t2 = table_of3({}, np.zeros((0, 4), dtype=np.int64), {}, {}, {1: gapped[1], 2: gapped[1]}, {1: np.array(rows), 2: np.array(rows)})
    assert t2.ecs == [((0,), 2)] and t2.rows.tolist() == [[0, 0, 26, 65], [0, 0, 69, 108]] and t2.n.tolist() == [2, 2]


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return gap_ec_case.case(tmp_path_factory)


def test_inputs_hold_every_class(case):
    gc = gap_calls(case)
    kept, rec = gc.kept(M, G), gc.gap_records(M, G)
    gap = case.gapped(M, G)[0]
    plen = case.index.arrays["path_len"].astype(np.int64)
    all_kept = [(i, pl) for i, k in kept.items() for pl in k]
    n_del = sum(1 for _, pl in all_kept if pl[3] == DEL)
    n_ins = sum(1 for _, pl in all_kept if pl[3] == INS)
    both = sum(1 for k in kept.values() if {pl[3] for pl in k} == {DEL, INS})
    rows = np.concatenate(list(rec.values()))
    at0 = sum(1 for i, k in kept.items() for j in range(len(k)) if rows_of(k[j:j + 1], len(case.reads[i]), lambda p: 0)[0, 1] == 0)
    at_end = sum(1 for i, k in kept.items() for j in range(len(k)) if rows_of(k[j:j + 1], len(case.reads[i]), lambda p: 0)[-1, 2] == plen[k[j][0]] - 1)
    slow = [i for i in gap if case.graphs_of(gap[i].paths) > 4]
    t = gc.table(M, G)
    t_off = gc.table(M, G, gapped=False)
    # tuples of the gapped records under their EC: (EC of G(r), path, Pos, last)
    ec_of = {ids: e for e, (ids, _) in enumerate(t.ecs)}
    keyed = np.concatenate([np.column_stack([np.full(len(r), ec_of[gap[i].paths], dtype=np.int64), r]) for i, r in rec.items()])
    tu, tc = np.unique(keyed, axis=0, return_counts=True)
    print("gap-rescued", len(gap), "DEL", n_del, "INS", n_ins, "records", len(rows), "tuples", len(tu), "count >= 2", int((tc >= 2).sum()), "both types", both,
          "X = 0", at0, "ends at path_len - 1", at_end, "slow reads", len(slow), "their placements", sum(len(kept[i]) for i in slow))
    assert n_del >= FLOOR and n_ins >= FLOOR and both >= FLOOR and at0 >= FLOOR and at_end >= FLOOR and len(slow) >= FLOOR
    assert int((tc >= 2).sum()) >= FLOOR
    # records = placements + the DEL placements among them
    assert len(rows) == len(all_kept) + n_del == n_ins + 2 * n_del
    c = gc.counts(M, G)
    assert (c["placements"], c["records"], c["gap"], c["gap_slow"]) == (len(all_kept), len(rows), len(gap), len(slow))
    # the table gains exactly these records over the rescued reads' table, and none of its tuples loses a count
    assert int(t.n.sum()) == int(t_off.n.sum()) + len(rows) and len(t.n) >= len(t_off.n) + 1
    # every interval lies inside its path
    assert (rows[:, 1] >= 0).all() and (rows[:, 1] <= rows[:, 2]).all() and (rows[:, 2] < plen[rows[:, 0]]).all()
    # the other thresholds of the device tests hold both types and slow reads as well
    for m, g in ((2, 8), (1, 3), (1, 1)):
        cm = gc.counts(m, g)
        km = gc.kept(m, g)
        d = sum(1 for k in km.values() for pl in k if pl[3] == DEL)
        print((m, g), cm, "DEL", d)
        assert d >= FLOOR and cm["placements"] - d >= FLOOR and cm["gap_slow"] >= 3 and cm["records"] == cm["placements"] + d


def test_interval_lengths_sum_to_gdepth(case):
    """per path, the gapped records cover as many bases as the brute force's gdepth holds: the records lie on the bases gdepth grows on"""
    gc = gap_calls(case)
    rec = gc.gap_records(M, G)
    case.placements(M, G)(case.reads[0])                    # (the brute force of gaps up to 3 exists)
    gt = gap_def.GapTables(case.index, M, G, case._brute[3])
    gt.add(case.reads, case.has)
    n_paths = case.index.view.n_paths
    covered = np.zeros(n_paths, dtype=np.int64)
    depth = np.zeros(int(gt.base[-1]), dtype=np.int64)
    for r in rec.values():
        np.add.at(covered, r[:, 0], r[:, 2] - r[:, 1] + 1)
        for p, a, b in r.tolist():
            depth[int(gt.base[p]) + a:int(gt.base[p]) + b + 1] += 1
    want = np.array([int(gt.gdepth[int(gt.base[p]):int(gt.base[p + 1])].sum()) for p in range(n_paths)])
    assert covered.sum() >= 100000 and np.array_equal(covered, want), np.flatnonzero(covered != want)[:10]
    assert np.array_equal(depth, gt.gdepth)                 # base by base, too
    assert gt.stats["placements"] == gc.counts(M, G)["placements"]
