"""The definition of the gap-placed reads in the equivalence classes (include/groot_hip.h, "gap-placed reads in the equivalence classes") as
a brute force, for tests/test_gap_ec_def.py, tests/test_gap_ec.py and tests/test_abundance_gapped_cli.py:

    G(r)    for a read r that is GAP-RESCUED (a gap candidate with a kept gapped placement, e*(r) <= M + G): the set of global paths p for
            which r has a kept gapped placement -- any strand, x, type, g; each p once.  Not defined for any other read.
    S++(r)  = S(r) when r has a record;  R(r) when r is rescued ungapped;  G(r) when r is gap-rescued;  empty otherwise.

gap_sets takes the gap candidates from rescue_def.Tables (a candidate that mismatch rescue leaves unplaced, long enough for a gap), every
gapped placement from gap_def.Brute.placements and the kept ones from gap_def.keep, and keeps the set of their paths.  No anchors, no
tables, no knowledge of the kernels.  numpy only."""
from collections import namedtuple

from gap_def import keep
from rescue_def import A, Tables

# e: e*(r); paths: G(r), ascending; strands / types: those of the kept placements; kept: their number; multi_x: some path carries kept
# placements at more than one x
Gapped = namedtuple("Gapped", "e paths strands types kept multi_x")


def gap_sets(index, M, G, reads, has_record, placements):
    """-> ({read: Gapped} of the gap-rescued reads, [read] of the gap candidates left unplaced); placements(read bytes) -> every gapped
    placement (p, strand, x, type, g, d, k*) with d <= M and g <= G at least (gap_def.Brute.placements)"""
    t = Tables(index, M)
    t.add(reads, has_record)
    out, left = {}, []
    for i, d_star, _ in t.d_star:
        if d_star is not None or len(reads[i]) < A * (M + 3):
            continue                                                   # rescued ungapped, or too short for a gap: no gap candidate
        e, kept = keep(placements(reads[i]), M, G)
        if e is None:
            left.append(i)
            continue
        xs = {}
        for p, strand, x, typ, g, d, k in kept:
            xs.setdefault(p, set()).add(x)
        out[i] = Gapped(e, tuple(sorted(xs)), frozenset(pl[1] for pl in kept), frozenset(pl[3] for pl in kept), len(kept), any(len(v) > 1 for v in xs.values()))
    return out, left


def ecs_plus3(exact, rescued, gapped, reads=None):
    """the ECs of the definition: {ids tuple: reads} over S++(r) of `reads` (default: every read); exact: {read: S(r) as a tuple}, rescued:
    rescue_sets_def.rescued_sets' first result, gapped: gap_sets' first result"""
    out = {}
    for i in (sorted(set(exact) | set(rescued) | set(gapped)) if reads is None else reads):
        s = exact.get(i) or (rescued[i].paths if i in rescued else None) or (gapped[i].paths if i in gapped else None)
        if s:
            out[s] = out.get(s, 0) + 1
    return out
