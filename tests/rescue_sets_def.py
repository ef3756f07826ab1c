"""The definition of the rescued reads in the equivalence classes (include/groot_hip.h, "rescued reads in the equivalence classes") as a
brute force, for tests/test_rescue_ec.py and tests/test_abundance_rescued_cli.py:

    R(r)   for a read r that is RESCUED under mismatch rescue (a candidate with d*(r) <= M): the set of global paths p for which r has a
           KEPT placement (p, strand, x) -- any strand, any x, each p once.
    S+(r)  = S(r) when r has a record;  R(r) when r is rescued;  empty otherwise.

rescued_sets compares every oriented candidate with every window of every text (rescue_def.Tables' windows: the comparison of one window
with one read is a sum over one-hot columns, exact in float32) and keeps, per rescued read, the paths at d*.  No anchors, no tables, no
knowledge of the kernels.  numpy only."""
from collections import namedtuple

import numpy as np

from rescue_def import A, Tables, _ACGT, _rc

# d: d*(r); paths: R(r), ascending; strands: the strands of the kept placements; kept: their number; multi_x: some path carries kept
# placements at more than one x
Rescued = namedtuple("Rescued", "d paths strands kept multi_x")


def rescued_sets(index, M, reads, has_record, tables=None):
    """-> ({read: Rescued} of the rescued reads, [read] of the candidates left unrescued); tables: a rescue_def.Tables of the index whose
    windows are used (they do not depend on M: a caller with several M builds them once)"""
    t = tables or Tables(index, M)
    by_len, out, left = {}, {}, []
    for i, r in enumerate(reads):
        if not has_record[i] and all(c in b"ACGT" for c in r) and len(r) >= A * (M + 1):
            by_len.setdefault(len(r), []).append(i)
    for L, idx in sorted(by_len.items()):
        oh, w, at = t._windows(L)
        path = np.searchsorted(t.base, at, side="right") - 1          # the path of every window, and its slot's offset in it
        x = at - t.base[path]
        for c0 in range(0, len(idx), 256):
            chunk = idx[c0:c0 + 256]
            ori = np.array([np.frombuffer(o, dtype=np.uint8) for i in chunk for o in (reads[i], _rc(reads[i]))])
            d = L - np.rint(oh @ (ori[:, :, None] == _ACGT).reshape(len(ori), 4 * L).astype(np.float32).T).astype(np.int64) if len(w) else np.zeros((0, len(ori)), dtype=np.int64)
            for j, i in enumerate(chunk):
                dj = d[:, 2 * j:2 * j + 2]
                best = int(dj.min()) if dj.size else M + 1
                if best > M:
                    left.append(i)
                    continue
                rows, strand = np.nonzero(dj == best)
                px = np.unique(path[rows] * (1 << 32) + x[rows])        # (path, x), each once whatever the strand
                per_path = np.bincount(np.searchsorted(np.unique(path[rows]), px >> 32))
                out[i] = Rescued(best, tuple(int(p) for p in np.unique(path[rows])), frozenset(int(s) for s in strand), len(rows), bool((per_path > 1).any()))
    return out, left


def ecs_plus(exact, rescued, reads=None):
    """the ECs of the definition: {ids tuple: reads} over S+(r) of `reads` (default: every read); exact: {read: S(r) as a tuple}, rescued:
    rescued_sets' first result"""
    out = {}
    for i in (sorted(set(exact) | set(rescued)) if reads is None else reads):
        s = exact.get(i) or (rescued[i].paths if i in rescued else None)
        if s:
            out[s] = out.get(s, 0) + 1
    return out
