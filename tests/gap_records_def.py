"""The definition of the gapped records (include/groot_hip.h, "gapped records") as a brute force, for tests/test_gap_records_def.py and
tests/test_gap_records.py:

    A GAPPED RECORD is one kept gapped placement (p, strand, x, type, g) of a gap-rescued read: read = position of r in its batch,
    path = p, pos = X = first Position of p + x, k = k*, strand, d, type, g, and mm[3] = the offsets i, ascending, in the ORIENTED read at
    which an ALIGNED read base differs from the text base it lies on:
        i < k: R[i] != T[x+i];    DEL, i >= k: R[i] != T[x+g+i];    INS, i >= k+g: R[i] != T[x+i-g]
    (the inserted bases R[k, k+g) are never listed); the d first entries are set, the rest are 0xFFFF.  The gapped records of a batch are
    ALL kept gapped placements of ALL its gap-rescued reads, each once, in ascending (read, path, strand, pos, type, g) order.

The placements are gap_def.GapTables.per_read's -- every (path, strand, x, type, g, k), no anchors, no tables, no knowledge of the kernels;
this module adds the mismatch offsets, read off the text base by base, and the order.  numpy only."""
import numpy as np

from gap_def import DEL, INS, GapTables
from rescue_def import _rc

RECORD_DTYPE = np.dtype([("read", "<u4"), ("path", "<u4"), ("pos", "<u4"), ("k", "<u2"), ("mm", "<u2", (3,)), ("strand", "u1"), ("d", "u1"), ("type", "u1"),
                         ("g", "u1")])   # groot_gap_record
NONE = 0xFFFF


def offsets(R, T, x, typ, g, k):
    """mm of the placement of the oriented read R on the text T: a direct comparison, base by base"""
    mm = []
    for i in range(len(R)):
        if i < k:
            y = x + i
        elif typ == DEL:
            y = x + g + i
        elif i < k + g:
            continue                                                 # an inserted base lies on no text base
        else:
            y = x + i - g
        if R[i] != T[y]:
            mm.append(i)
    return mm


def rows_of(brute, read, kept):
    """(path, strand, pos, type, g, d, k, mm) of the kept placements of one read, sorted"""
    rows = []
    for p, strand, x, typ, g, d, k in kept:
        T, first = brute.texts[p][0].tobytes(), brute.texts[p][1]
        mm = offsets(_rc(read) if strand else read, T, x, typ, g, k)
        assert len(mm) == d, (mm, d)
        rows.append((p, strand, first + x, typ, g, d, k, tuple(mm + [NONE] * (3 - len(mm)))))
    assert len({r[:5] for r in rows}) == len(rows)                   # each (p, strand, x, type, g) once
    return sorted(rows)


def records(index, M, G, brute, reads, has_record):
    """the gapped records of the batch `reads` as RECORD_DTYPE, in the definition's order"""
    t = GapTables(index, M, G, brute)
    t.add(reads, has_record)
    rows = []
    for i, e, kept in sorted(t.per_read, key=lambda v: v[0]):
        if e is None:
            continue
        assert all(x[5] + x[4] == e for x in kept)                   # every kept placement of a read is at e*
        rows += [(i,) + r for r in rows_of(brute, reads[i], kept)]
    out = np.zeros(len(rows), dtype=RECORD_DTYPE)
    for n, (i, p, strand, X, typ, g, d, k, mm) in enumerate(rows):
        out[n] = (i, p, X, k, mm, strand, d, typ, g)
    return out


def plain(rec):
    """records as a list of (read, path, pos, k, strand, d, type, g, (mm0, mm1, mm2)): what an assert prints"""
    return [(int(r["read"]), int(r["path"]), int(r["pos"]), int(r["k"]), int(r["strand"]), int(r["d"]), int(r["type"]), int(r["g"]), tuple(int(x) for x in r["mm"]))
            for r in rec]
