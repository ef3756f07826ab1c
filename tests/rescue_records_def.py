"""The definition of the rescued records (include/groot_hip.h, "rescued records") as a brute force, for tests/test_rescue_records_def.py
and tests/test_rescue_records.py:

    A RESCUED RECORD is one kept placement of a rescued read: read = position of r in its batch, path = global path p, pos = X,
    strand, d = d*(r), mm[3] = the offsets i, ascending, in the ORIENTED read with oriented[i] != text_p[x + i]; the d first entries
    are set, the rest are 0xFFFF.  The rescued records of a batch are ALL kept placements of ALL its rescued reads, each once, in
    ascending (read, path, strand, pos) order.

The placements are rescue_calls_def.rescued_records' -- every window of every text, no anchors, no tables, no knowledge of the kernels;
this module adds the mismatch offsets, read off the text byte by byte, and the order.  numpy only."""
import numpy as np

from rescue_calls_def import rescued_records
from rescue_def import Tables, _rc

RECORD_DTYPE = np.dtype([("read", "<u4"), ("path", "<u4"), ("pos", "<u4"), ("mm", "<u2", (3,)), ("strand", "u1"), ("d", "u1")])   # groot_rescue_record
NONE = 0xFFFF


def records(index, M, reads, has_record, tables=None):
    """the rescued records of the batch `reads` as RECORD_DTYPE, in the definition's order"""
    t = tables or Tables(index, M)
    placed = rescued_records(index, M, reads, has_record, t)
    rows = []
    for i in sorted(placed):
        for path, X, last, strand in placed[i].tolist():
            text, first = t.texts[path]
            o = _rc(reads[i]) if strand else reads[i]
            assert last - X + 1 == len(o)
            w = text[X - first:X - first + len(o)]
            mm = [k for k in range(len(o)) if o[k] != w[k]]
            assert len(mm) <= M
            rows.append((i, path, strand, X, len(mm), mm + [NONE] * (3 - len(mm))))
        assert len({r[4] for r in rows[-len(placed[i]):]}) == 1      # every kept placement of a read is at d*
    rows.sort(key=lambda r: r[:4])
    out = np.zeros(len(rows), dtype=RECORD_DTYPE)
    for k, (i, path, strand, X, d, mm) in enumerate(rows):
        out[k] = (i, path, X, mm, strand, d)
    return out


def plain(rec):
    """records as a list of (read, path, pos, strand, d, (mm0, mm1, mm2)): what an assert prints"""
    return [(int(r["read"]), int(r["path"]), int(r["pos"]), int(r["strand"]), int(r["d"]), tuple(int(x) for x in r["mm"])) for r in rec]
