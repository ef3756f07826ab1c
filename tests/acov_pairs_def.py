"""Assigned coverage over fragments (`--calls --callsPaired`, groot_hip_acov_pairs_enable): the rule restated in plain Python over the
CPU oracle's expanded records.  Quoted from include/groot_hip.h:

    S(r), fragments, A = S(r_2i), B = S(r_2i+1), joined / split / single / none, units, ECs over units, canonical order, alpha, w(e,p):
    exactly as in "paired-end reads"  and "assigned coverage" (DESIGN 13).
    U(r), the UNIT SET of a read r with records:   A n B  when r's fragment is joined (both mates get the same set);
                                                   S(r)   when it is split or single.
    A record of read r on path p COUNTS when p is in U(r); it is then a record of the pileup under e = EC of U(r), covering [Pos, last],
    last = min(Pos + M, path_len(p) - 1), M the record's own M op (its own mate's length less its clips): the interval of DESIGN 13, unchanged.
    A record of a joined fragment on a path outside A n B is LEFT OUT: the unit the EM counted has no posterior there (w(e,p) is defined for
    p in e only), so its weight is zero.  Both mates' records count, each as one record; every strand, primary and secondary, as in DESIGN 13.
    The assigned-coverage table of a run with the feature on is the multiset of counting records grouped by (e, p, Pos, last).

The ECs are those of test_paired.units_of_alns, the grouping that of test_calls._group; nothing here looks at device output."""
import numpy as np

from test_calls import Table, _group
from test_paired import units_of_alns


def unit_sets_of_alns(alns, n_reads, first=0):
    """U(r) per batch-relative read: a sorted tuple of global path ids, None for a read without records; and the reads of joined fragments"""
    assert n_reads % 2 == 0
    sets = [set() for _ in range(n_reads)]
    for r, p in zip((alns["read_id"].astype(np.int64) - first).tolist(), alns["ref_id"].tolist()):
        sets[r].add(p)
    unit, joined = [None] * n_reads, 0
    for i in range(n_reads // 2):
        a, b = sets[2 * i], sets[2 * i + 1]
        if a & b:
            unit[2 * i] = unit[2 * i + 1] = tuple(sorted(a & b))
            joined += 2
        else:
            unit[2 * i] = tuple(sorted(a)) if a else None
            unit[2 * i + 1] = tuple(sorted(b)) if b else None
    return unit, joined


def paired_table_of_alns(index, alns, seq_off, first=0):
    """-> (the assigned-coverage table of one batch of fragments as a test_calls.Table, the records left out).  seq_off: the batch's read
    offsets; the records' read ids are `first` + the batch position"""
    lens = index.arrays["path_len"].astype(np.int64)
    off = np.asarray(seq_off, dtype=np.int64)
    n_reads = len(off) - 1
    units, _ = units_of_alns(alns, n_reads, first)
    count = {}
    for u in units:
        count[u] = count.get(u, 0) + 1
    ecs = sorted(count.items())
    ec_index = {ids: i for i, (ids, _) in enumerate(ecs)}
    unit, _ = unit_sets_of_alns(alns, n_reads, first)
    rid, ref, pos = alns["read_id"].astype(np.int64) - first, alns["ref_id"].astype(np.int64), alns["pos"].astype(np.int64)
    m = (off[rid + 1] - off[rid]) - alns["start_clip"].astype(np.int64) - alns["end_clip"].astype(np.int64)
    last = np.minimum(pos + m, lens[ref] - 1)
    rows, left = [], 0
    for r, p, x, y in zip(rid.tolist(), ref.tolist(), pos.tolist(), last.tolist()):
        u = unit[r]
        if p in u:           # (u is a short tuple)
            rows.append((ec_index[u], p, x, y))
        else:
            left += 1
    return Table(ecs, *_group(rows if rows else np.zeros((0, 4)), np.ones(len(rows), dtype=np.int64))), left
