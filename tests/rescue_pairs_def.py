"""The rule of the rescued mates in paired-end units (include/groot_hip.h, "rescued mates in paired-end units") in plain
Python, for tests/test_rescue_pairs.py and tests/test_rescued_paired_cli.py:

    S(r), R(r), S+(r), candidate, rescued, d*, kept placement: exactly as in "mismatch rescue" and "rescued reads in the equivalence classes".
    Fragments, joined / split / single / none, units, ECs over units: exactly as in "paired-end reads" (DESIGN §12), with
        A = S+(r_2i),  B = S+(r_2i+1)
    in place of S(.).  So a mate counts with its records' paths when it has records, with R(r) when mismatch rescue places it, and as
    empty otherwise (no record and: no candidate, or a candidate left unplaced, or placed only with a gap).
      joined:  A n B not empty: one unit, A n B.     split: both non-empty, disjoint: two units, A and B.
      single:  one non-empty: one unit.              none: no unit.
    R(r) is the set at d*(r) and nothing else: a rescued mate whose kept placements miss every path of its partner is SPLIT from it, even where
    a placement at a larger distance would have met one.  Mates are still rescued one by one; no insert size, no orientation.
    The run's ECs are the distinct unit sets with their unit counts; a unit made of exact mates, of rescued mates or of one of each, with the
    same set, is one EC.  joined + 2 split + single = ec_stats.reads.

It is test_paired.units_of_alns over S+(r): S(r) comes from the CPU oracle's records, R(r) from rescue_sets_def.rescued_sets (brute force,
no anchors), and a rescued read enters units_of_alns as one pseudo-record per path of R(r).  Nothing here ever sees device output."""
from collections import namedtuple

import numpy as np

from test_paired import units_of_alns

# ecs: {unit set: units};  cls: fragments joined / split / single / none;  kinds: groot_rescue_pairs_stats' six fragment counts;
# rescued_mates: rescued mates in a unit;  bitmap_rows / bitmap_units / bitmap_mates: what the fragments with a mate in more than max_segs
# graphs take of the pool (one bitmap per non-empty mate), the units they make, the rescued mates in those;  exact_slow: the slow-path
# units among the fragments whose mates both have records (groot_hip_ec_stats' slow_reads)
Want = namedtuple("Want", "ecs cls kinds rescued_mates bitmap_rows bitmap_units bitmap_mates exact_slow units")

KINDS = ("exact_rescued_joined", "exact_rescued_split", "rescued_rescued_joined", "rescued_rescued_split", "single_exact", "single_rescued")


def splus_alns(exact, rescued, n_reads, first=0):
    """S+(r) of the batch as the records units_of_alns reads: (read_id, ref_id) once per path.  exact: {read: S(r) as a tuple} of the reads
    with a record, rescued: {read: R(r) as a tuple} of the rescued reads (batch-relative reads; the two exclude each other)"""
    assert not set(exact) & set(rescued)
    rows = [(first + r, p) for src in (exact, rescued) for r, s in src.items() if r < n_reads for p in s]
    out = np.zeros(len(rows), dtype=[("read_id", np.int64), ("ref_id", np.int64)])
    if rows:
        out["read_id"], out["ref_id"] = zip(*rows)
    return out


def expect(gpo, exact, rescued, n_reads, max_segs=4, frags=None):
    """the definition over the fragments `frags` (default: all) of a batch of n_reads mates.  gpo: graph_path_off"""
    gpo = np.asarray(gpo, dtype=np.int64)
    graphs = lambda s: len(set((np.searchsorted(gpo, np.array(sorted(s)), side="right") - 1).tolist())) if s else 0
    frags = range(n_reads // 2) if frags is None else frags
    keep = {r for f in frags for r in (2 * f, 2 * f + 1)}
    ex = {r: s for r, s in exact.items() if r in keep}
    rs = {r: s for r, s in rescued.items() if r in keep}
    units, cls = units_of_alns(splus_alns(ex, rs, n_reads), n_reads)
    cls = dict(cls, none=cls["none"] - (n_reads // 2 - len(list(frags))))
    ecs = {}
    for u in units:
        ecs[u] = ecs.get(u, 0) + 1
    kinds = dict.fromkeys(KINDS, 0)
    mates = rows = b_units = b_mates = exact_slow = 0
    for f in frags:
        x, y = 2 * f, 2 * f + 1
        a, b = set(ex.get(x) or rs.get(x) or ()), set(ex.get(y) or rs.get(y) or ())
        n_resc = (x in rs) + (y in rs)
        two, joined = bool(a and b), bool(a & b)
        if x in ex and y in ex:                      # the unchanged path: what ec_collect folds of it on the host
            exact_slow += graphs(a & b) > max_segs if joined else (graphs(a) > max_segs) + (graphs(b) > max_segs)
            continue
        if not a and not b:
            continue
        mates += n_resc
        if two:
            kinds[("rescued_rescued_" if n_resc == 2 else "exact_rescued_") + ("joined" if joined else "split")] += 1
        else:
            kinds["single_rescued" if n_resc else "single_exact"] += 1
        if graphs(a) > max_segs or graphs(b) > max_segs:
            rows += 2 if two else 1
            b_units += 2 if two and not joined else 1
            b_mates += n_resc
    return Want(ecs, cls, kinds, mates, rows, b_units, b_mates, exact_slow, units)
