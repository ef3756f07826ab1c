"""The rule of the rescued mates in assigned coverage over fragments (include/groot_hip.h, "rescued mates in assigned coverage over
fragments") in plain Python, for tests/test_calls_rescued_paired*.py:

    S(r), R(r), S+(r), candidate, rescued, d*, kept placement (p, strand, x), X, len: exactly as in "mismatch rescue" and "rescued reads in the
    equivalence classes".  Fragments, A = S+(r_2i), B = S+(r_2i+1), joined / split / single / none, units, ECs over units: exactly as in
    "rescued mates in paired-end units" (DESIGN §25).  Canonical order, alpha, w(e,p): as for --abundance over those ECs.
    U(r), the UNIT SET of a mate r with S+(r) non-empty:   A n B when r's fragment is joined (both mates the same set);  S+(r) when split or single.
    An exact record of r on p COUNTS when p is in U(r), covering [Pos, min(Pos + M, path_len(p) - 1)]           (§13 / §24's interval, unchanged).
    A kept placement (p, strand, x) of a rescued mate r COUNTS when p is in U(r), as one rescued record covering [X, X + len - 1]   (§19's interval).
    A record or placement on a path outside U(r) is LEFT OUT (w(e,p) is defined for p in e only).  Every counting one counts once: both mates,
    both strands, every x, several on one path, primary and secondary.  The two interval rules are not made alike.
    The table is the multiset of counting exact AND rescued records grouped by (e = EC of U(r), p, Pos, last): n(e,p,Pos,last), integers.
    A mate placed only with a gap, left unplaced, too short or with a non-ACGT base has the empty set and no record, as in §25.
    A pass that collect redoes counts once; a batch under kCovSkipFlags counts nothing; a batch that fails counts nothing anywhere.
    The table depends on the reads, their pairing and the index alone: not on batch size, pipeline depth, align stage, --ctxPerGpu or --gpus.

From existing pieces: the units and U(r) are rescue_pairs_def.expect / test_paired.units_of_alns over S+(r), the exact rows
rescue_calls_def.exact_rows over the CPU oracle's records, the rescued rows rescue_calls_def.rescued_records (every window of every text),
the grouping test_calls._group.  Nothing here ever sees device output."""
from collections import namedtuple

import numpy as np

from rescue_pairs_def import expect as units_expect
from test_calls import Table, _group

# table: test_calls.Table (ECs canonical, rows ascending);  units: rescue_pairs_def.Want of the same fragments;  unit: {read: U(r)};
# stats: groot_rescue_acov_pairs_stats' record counts;  log: the records, counting or not, of the fragments on bitmaps (the slot's log);
# ee_left: the records left out of the fragments whose mates both have records (groot_acov_pairs_stats.left_out);
# kinds: records by the kind of fragment, for the floors of the tests;  one_pass: the distinct tuples of the records the device claims and adds
# in one pass (kept placements, exact records beside a rescued partner; not those of the fragments on bitmaps), which need room when they come
Want = namedtuple("Want", "table units unit stats log ee_left kinds one_pass")

STATS = ("exact_records", "exact_left_out", "rescued_records", "rescued_left_out", "host_records")


def unit_sets(exact, rescued, n_reads, frags=None):
    """{read: U(r) as a sorted tuple} of the mates with S+(r) non-empty, and per fragment 'joined' / 'split' / 'single' / 'none'"""
    unit, cls = {}, {}
    for f in (range(n_reads // 2) if frags is None else frags):
        x, y = 2 * f, 2 * f + 1
        a, b = set(exact.get(x) or rescued.get(x) or ()), set(exact.get(y) or rescued.get(y) or ())
        if a & b:
            unit[x] = unit[y] = tuple(sorted(a & b))
            cls[f] = "joined"
        else:
            if a:
                unit[x] = tuple(sorted(a))
            if b:
                unit[y] = tuple(sorted(b))
            cls[f] = "split" if a and b else "single" if a or b else "none"
    return unit, cls


def rows_by_read(ex_rows):
    """exact_rows grouped: {read: [(path, Pos, last)]} (expect takes either; a caller with many subsets groups once)"""
    by_read = {}
    for row in np.asarray(ex_rows, dtype=np.int64).reshape(-1, 4).tolist():
        by_read.setdefault(row[0], []).append(tuple(row[1:]))
    return by_read


def expect(gpo, exact, rescued, ex_rows, records, n_reads, max_segs=4, frags=None):
    """the definition over the fragments `frags` (default: all) of a batch of n_reads mates.  gpo: graph_path_off; exact {read: S(r)} and
    rescued {read: R(r)} exclude each other; ex_rows: rescue_calls_def.exact_rows (read, path, Pos, last) of the batch's records, or rows_by_read of them;
    records: rescue_calls_def.rescued_records {read: rows (path, X, last, strand)}"""
    gpo = np.asarray(gpo, dtype=np.int64)
    graphs = lambda s: len(set((np.searchsorted(gpo, np.array(sorted(s)), side="right") - 1).tolist())) if s else 0
    frags = list(range(n_reads // 2) if frags is None else frags)
    units = units_expect(gpo, exact, rescued, n_reads, max_segs, frags)
    unit, cls = unit_sets(exact, rescued, n_reads, frags)
    ecs = sorted(units.ecs.items())
    assert sorted(set(unit.values())) == [ids for ids, _ in ecs]          # U(r) names the units rescue_pairs_def counted
    index = {ids: i for i, (ids, _) in enumerate(ecs)}
    by_read = ex_rows if isinstance(ex_rows, dict) else rows_by_read(ex_rows)
    stats, kinds = dict.fromkeys(STATS, 0), {}
    rows, log, ee_left, one = [], 0, 0, set()

    def count(kind, n=1):
        kinds[kind] = kinds.get(kind, 0) + n

    for f in frags:
        x, y = 2 * f, 2 * f + 1
        ee = x in exact and y in exact
        sp = lambda r: set(exact.get(r) or rescued.get(r) or ())
        bitmap = not ee and (graphs(sp(x)) > max_segs or graphs(sp(y)) > max_segs)
        n_resc = (x in rescued) + (y in rescued)
        for r in (x, y):
            if r in exact:
                assert {p for p, _, _ in by_read[r]} == set(exact[r])      # the records of r are on S(r)
                one_pass = not ee and (cls[f] == "joined" or bitmap)       # (else the ordinary count's: both mates exact, or a mate of its own)
                for p, pos, last in by_read[r]:
                    if p in unit[r]:
                        rows.append((index[unit[r]], p, pos, last))
                        if one_pass and not bitmap:
                            one.add(rows[-1])
                        stats["exact_records"] += one_pass
                        stats["host_records"] += bitmap
                        if not ee and cls[f] == "joined":
                            count("exact beside rescued")
                    else:
                        stats["exact_left_out"] += one_pass
                        ee_left += ee
                        if not ee:
                            count("exact left out")
                    log += bitmap
                    count("bitmap records", bitmap)
            elif r in rescued:
                rec = records[r]
                assert tuple(np.unique(rec[:, 0]).tolist()) == tuple(rescued[r])      # the two brute forces agree on R(r)
                for p, pos, last, _ in rec.tolist():
                    if p in unit[r]:
                        rows.append((index[unit[r]], p, pos, last))
                        if not bitmap:
                            one.add(rows[-1])
                        stats["rescued_records"] += 1
                        stats["host_records"] += bitmap
                        if cls[f] == "joined":
                            count("placements, exact + rescued joined" if n_resc == 1 else "placements, rescued + rescued joined")
                    else:
                        stats["rescued_left_out"] += 1
                        count("placements left out")
                    log += bitmap
                    count("bitmap records", bitmap)
        if not ee and cls[f] in ("split", "single"):
            count(cls[f] + " fragments")
    table = Table(ecs, *_group(rows if rows else np.zeros((0, 4)), np.ones(len(rows), dtype=np.int64)))
    return Want(table, units, unit, stats, log, ee_left, kinds, len(one))
