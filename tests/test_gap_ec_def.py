"""CPU: the inputs of the tests of the gap-placed reads in the equivalence classes (tests/gap_ec_case.py) hold every class the definition
(include/groot_hip.h, "gap-placed reads in the equivalence classes") tells apart, from the brute force alone (tests/gap_sets_def.py):

    G(r)    for a gap-rescued read r: the set of global paths p for which r has a kept gapped placement -- any strand, x, type, g.
    S++(r)  = S(r) when r has a record;  R(r) when r is rescued ungapped;  G(r) when r is gap-rescued;  empty otherwise."""
import numpy as np
import pytest

import gap_def
import gap_ec_case
from gap_sets_def import ecs_plus3

FLOOR = 10
M, G = 2, 3


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return gap_ec_case.case(tmp_path_factory)


def test_inputs_hold_every_class(case):
    gap, left = case.gapped(M, G)
    res, res_left = case.rescued(M)
    ex = case.exact()
    # the three kinds exclude each other: a candidate has no record, a gap candidate is a candidate that ended unplaced
    assert not set(ex) & set(res) and not set(ex) & set(gap) and not set(res) & set(gap)
    assert set(gap) | set(left) <= set(res_left)
    count = lambda f: sum(1 for r in gap.values() if f(r))
    per_graphs = np.bincount([case.graphs_of(r.paths) for r in gap.values()], minlength=8)
    print("gap-rescued", len(gap), "left", len(left), "rescued", len(res), "exact", len(ex), "sets by graphs", per_graphs.tolist())
    assert per_graphs[1] >= FLOOR and per_graphs[2:5].sum() >= FLOOR and per_graphs[5:].sum() >= FLOOR, per_graphs
    assert per_graphs[2] >= FLOOR and per_graphs[3] >= FLOOR                # (S2: two graphs; S3: three)

    def two_words(ids):                     # more than 64 paths of one graph, with a bit in two mask words of that graph's segment
        ids = np.array(ids)
        g = np.searchsorted(case.gpo, ids, side="right") - 1
        return any((g == x).sum() > 64 and len(set(((ids[g == x] - case.gpo[x]) >> 6).tolist())) == 2 for x in set(g.tolist()))

    assert count(lambda r: two_words(r.paths)) >= FLOOR
    assert count(lambda r: 0 in r.strands) >= FLOOR and count(lambda r: 1 in r.strands) >= FLOOR
    assert count(lambda r: gap_def.DEL in r.types) >= FLOOR and count(lambda r: gap_def.INS in r.types) >= FLOOR
    assert count(lambda r: r.multi_x) >= FLOOR
    exact_sets, rescued_sets = set(ex.values()), {r.paths for r in res.values()}
    assert count(lambda r: r.paths in exact_sets) >= FLOOR
    assert count(lambda r: r.paths in rescued_sets) >= FLOOR
    assert count(lambda r: r.paths not in exact_sets and r.paths not in rescued_sets) >= FLOOR
    by_set = {}
    for r in gap.values():
        by_set[r.paths] = by_set.get(r.paths, 0) + 1
    assert sum(c for c in by_set.values() if c >= 2) >= FLOOR, sorted(by_set.values())
    assert len(left) >= 1
    # rescued ungapped although a gapped placement costs less: stays in R(r)
    brute = case.placements(M, G)
    cheaper = [i for i, r in res.items() if len(case.reads[i]) >= gap_def.A * (M + 3) and (gap_def.keep(brute(case.reads[i]), M, G)[0] or 99) < r.d]
    print("rescued ungapped, cheaper gapped:", len(cheaper), sorted({case.names[i] for i in cheaper}))
    assert len(cheaper) >= 1
    # every EC of the definition counts each read once
    ecs = ecs_plus3(ex, res, gap)
    assert sum(ecs.values()) == len(ex) + len(res) + len(gap)
    # the other thresholds of the device tests hold gap-rescued reads of both kinds of row as well
    for m, g in ((1, 3), (1, 1)):
        gm, lm = case.gapped(m, g)
        pg = np.bincount([case.graphs_of(r.paths) for r in gm.values()], minlength=8)
        print((m, g), "gap-rescued", len(gm), "left", len(lm), "sets by graphs", pg.tolist())
        assert pg[1:5].sum() >= FLOOR and pg[5:].sum() >= 3 and len(lm) >= 1         # (G = 1 keeps the one-base gaps only: a few wide sets)


def test_brute_force_on_hand_made_reads(case):
    """a stretch of S6 with a planted gap lies on every path of the six graphs that hold it; one of the repeat at two x of its one path"""
    gap, _ = case.gapped(M, G)
    s6 = tuple(range(int(case.gpo[3]), int(case.gpo[9])))
    a = [i for i, n in enumerate(case.names) if n == "gapS6" and i in gap]
    assert len(a) >= FLOOR and all(gap[i].paths == s6 for i in a), [gap[i].paths for i in a][:3]
    twice = int(case.gpo[9])
    r = [i for i, n in enumerate(case.names) if n == "gapR" and i in gap]
    assert sum(1 for i in r if gap[i].paths == (twice,) and gap[i].multi_x) >= FLOOR
    fan = tuple(range(int(case.gpo[6]), int(case.gpo[7]))) + tuple(range(int(case.gpo[10]), int(case.gpo[11])))
    f = [i for i, n in enumerate(case.names) if n == "gapS2" and i in gap]
    assert len(f) >= FLOOR and all(gap[i].paths == fan for i in f)
