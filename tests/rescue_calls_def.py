"""The definition of the rescued reads in assigned coverage (include/groot_hip.h, "rescued reads in assigned coverage") as a brute force,
for tests/test_rescue_calls_def.py, tests/test_rescue_calls.py and tests/test_calls_rescued_cli.py:

    A kept placement (p, strand, x) of a rescued read r of length len is one RESCUED RECORD of r on p covering [X, X + len - 1].
    The table of a run is the multiset of exact records AND rescued records grouped by (e = EC of S+(r), p, Pos, last).

Exact tuples come from the CPU oracle's expanded records, as test_calls.table_of_alns takes them; rescued tuples from every window of every
text (rescue_def.Tables' windows: no anchors, no tables, no knowledge of the kernels); both are keyed by S+(r) of rescue_sets_def.  numpy
only."""
import numpy as np

from rescue_def import A, Tables, _ACGT, _rc
from rescue_sets_def import ecs_plus
from test_calls import Table, _group


def rescued_records(index, M, reads, has_record, tables=None):
    """-> {read: int64[n, 4] rows (path, X, last, strand), one per kept placement} of the rescued reads.  X is the slot of the window's
    first base within its path (Position of the path's first node + the window's offset in the text): the coordinate of an exact
    record's Pos."""
    t = tables or Tables(index, M)
    by_len, out = {}, {}
    for i, r in enumerate(reads):
        if not has_record[i] and all(c in b"ACGT" for c in r) and len(r) >= A * (M + 1):
            by_len.setdefault(len(r), []).append(i)
    for L, idx in sorted(by_len.items()):
        oh, w, at = t._windows(L)
        if not len(w):
            continue
        path = np.searchsorted(t.base, at, side="right") - 1
        x = at - t.base[path]
        for c0 in range(0, len(idx), 256):
            chunk = idx[c0:c0 + 256]
            ori = np.array([np.frombuffer(o, dtype=np.uint8) for i in chunk for o in (reads[i], _rc(reads[i]))])
            d = L - np.rint(oh @ (ori[:, :, None] == _ACGT).reshape(len(ori), 4 * L).astype(np.float32).T).astype(np.int64)
            for j, i in enumerate(chunk):
                dj = d[:, 2 * j:2 * j + 2]
                best = int(dj.min())
                if best > M:
                    continue
                rows, strand = np.nonzero(dj == best)
                out[i] = np.stack([path[rows], x[rows], x[rows] + L - 1, strand], axis=1).astype(np.int64)
    return out


def exact_rows(index, alns, seq_off):
    """(read, path, Pos, last) of every expanded record, int64[n, 4]: the interval of test_calls.table_of_alns"""
    lens = index.arrays["path_len"].astype(np.int64)
    off = np.asarray(seq_off, dtype=np.int64)
    rid, ref, pos = alns["read_id"].astype(np.int64), alns["ref_id"].astype(np.int64), alns["pos"].astype(np.int64)
    m = (off[rid + 1] - off[rid]) - alns["start_clip"].astype(np.int64) - alns["end_clip"].astype(np.int64)
    return np.stack([rid, ref, pos, np.minimum(pos + m, lens[ref] - 1)], axis=1).reshape(-1, 4)


def table_of(exact, ex_rows, rescued, records, reads=None):
    """the table of the definition over `reads` (default: all): exact {read: S(r)}, ex_rows exact_rows(), rescued {read: Rescued} of
    rescue_sets_def.rescued_sets, records rescued_records() -> test_calls.Table (ECs canonical, rows ascending)"""
    keep = None if reads is None else set(reads)
    ecs = sorted(ecs_plus(exact, rescued, None if reads is None else list(reads)).items())
    index = {ids: i for i, (ids, _) in enumerate(ecs)}
    rows = [np.zeros((0, 4), dtype=np.int64)]
    if len(ex_rows):
        sel = ex_rows if keep is None else ex_rows[np.isin(ex_rows[:, 0], sorted(keep))]
        e = np.array([index[exact[int(r)]] for r in sel[:, 0]], dtype=np.int64)
        rows.append(np.column_stack([e, sel[:, 1:]]).reshape(-1, 4))
    for i, rec in records.items():
        if keep is not None and i not in keep:
            continue
        assert tuple(np.unique(rec[:, 0]).tolist()) == rescued[i].paths and len(rec) == rescued[i].kept      # the two brute forces agree on R(r)
        rows.append(np.column_stack([np.full(len(rec), index[rescued[i].paths], dtype=np.int64), rec[:, :3]]))
    rows = np.concatenate(rows)
    return Table(ecs, *_group(rows, np.ones(len(rows), dtype=np.int64)))
