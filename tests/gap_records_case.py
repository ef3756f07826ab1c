"""The case of tests/test_gap_records_def.py and tests/test_gap_records.py, in two parts, one per index (a record names a path):

    classes   the index and the batch of tests/gap_case.py, plus reads of its own
    shapes    the index and the batch of tests/gap_shapes_case.py (reads up to 512 bases, thirteen paths), plus reads of its own
    pal       the index of tests/rescue_records_shapes_case.py, whose paths q0 and q1 hold (ACGT) x 24 and an 80-base reverse-complement
              palindrome, and reads of its own alone: an insertion into the whole palindrome, and into 80 bases of the period-4 repeat --
              both strands, and several x on one path

The reads of its own are the classes of RECORD those two leave out -- their generators keep substitutions at least 3 bases away from the
gap: a substitution at k - 1, on the first aligned base behind the gap, at oriented offset 0 and at len - 1, k* at 31, 32, 33, 63, 64 and
65, offsets above 255, g = 1 and g = 8 of both types.  Each is drawn again until the brute force (tests/gap_records_def.py) puts it in
its class under (M, G) = (2, 8): a substitution next to the gap can move k*.  CLASSES tells a read's class from its records alone, and
tests/test_gap_records_def.py holds a floor of ten records per class.  Built once per process and shared by the two test files."""
import numpy as np

import gap_case
import gap_shapes_case
from gap_case import DEL, INS, gapped
from gap_def import Brute, keep
from gap_records_def import NONE, RECORD_DTYPE, records, rows_of
from rescue_def import A, _rc, path_texts
from test_counter_edges import _of_reads
from test_rescue import _has_record, _reads_of

_CASE = []


def _mm(rows):
    return [[m for m in r[7] if m != NONE] for r in rows]


# class -> (rows of ONE read as gap_records_def.rows_of gives them, the read's length) -> the read's records are in the class
CLASSES = {
    "sub at k-1": lambda rows, L: any(r[6] - 1 in m for r, m in zip(rows, _mm(rows))),
    "sub behind the gap": lambda rows, L: any((r[6] + (r[4] if r[3] == INS else 0)) in m for r, m in zip(rows, _mm(rows))),
    "sub at 0": lambda rows, L: any(0 in m for m in _mm(rows)),
    "sub at len-1": lambda rows, L: any(L - 1 in m for m in _mm(rows)),
    "offset above 255": lambda rows, L: any(x > 255 for m in _mm(rows) for x in m),
    "two paths": lambda rows, L: len({r[0] for r in rows}) >= 2,
    "both strands": lambda rows, L: len({r[1] for r in rows}) == 2,
    "two x on one path": lambda rows, L: len({r[:3] for r in rows}) > len({r[:2] for r in rows}),
    "DEL and INS alike": lambda rows, L: len({r[3] for r in rows}) == 2,
}
for _k in (31, 32, 33, 63, 64, 65):
    CLASSES["k*=%d" % _k] = (lambda k: lambda rows, L: any(r[6] == k for r in rows))(_k)
for _g in (1, 8):
    for _t in (DEL, INS):
        CLASSES["g=%d %s" % (_g, "DI"[_t])] = (lambda g, t: lambda rows, L: any(r[3] == t and r[4] == g for r in rows))(_g, _t)
OPTIONAL = {"DEL and INS alike"}          # (held if the brute force finds one in a repeat: the floor is checked where it does)


def _own_reads(rng, brute, texts, long_texts):
    """-> [(class, read)]: twelve reads per class that the generators of the two cases leave out, each in its class by the brute force"""
    out = []

    def draw(name, make, tries=400):
        for _ in range(tries):
            r = make()
            e, kept = keep(brute.placements(r), 2, 8)
            if e is not None and CLASSES[name](rows_of(brute, r, kept), len(r)):
                out.append((name, _rc(r) if len(out) & 1 else r))
                return
        raise AssertionError("no read of class " + name)

    def read(t, L, typ, g, k, subs):
        wlen = L + g if typ == DEL else L - g
        x = int(rng.integers(1, len(t) - wlen - 1))
        return gapped(rng, t, x, L, typ, g, k, [s for s in subs if 0 <= s < L])

    def anyk(L, typ, g):
        return int(rng.integers(A + 4, (L if typ == DEL else L - g) - A - 4))

    for i in range(12 if texts else 0):
        t, L, typ, g = texts[i % len(texts)], (80, 96, 100, 129, 150)[i % 5], i & 1, 1 + i % 3
        # (d(k - 1) <= d(k) when R[k - 1] is a mismatch in front of the gap, and the smallest k wins: only k* = A has a mismatch at k* - 1)
        draw("sub at k-1", lambda: read(t, L, typ, g, A, [A - 1]))
        draw("sub behind the gap", lambda: (lambda k: read(t, L, typ, g, k, [k + (g if typ == INS else 0)]))(anyk(L, typ, g)))
        draw("sub at 0", lambda: read(t, L, typ, g, anyk(L, typ, g), [0]))
        draw("sub at len-1", lambda: read(t, L, typ, g, anyk(L, typ, g), [L - 1]))
        for g2 in (1, 8):
            draw("g=%d %s" % (g2, "DI"[typ]), lambda: read(t, L, typ, g2, anyk(L, typ, g2), [int(rng.integers(2, A - 2))][:i % 3 == 0]))
            draw("g=%d %s" % (g2, "DI"[1 - typ]), lambda: read(t, L, 1 - typ, g2, anyk(L, 1 - typ, g2), []))
    for k in (31, 32, 33, 63, 64, 65) if texts else ():
        for i in range(12):
            t, L, typ, g = texts[i % len(texts)], (100, 129, 150)[i % 3], i & 1, 1 + i % 3
            draw("k*=%d" % k, lambda: read(t, L, typ, g, k, [int(rng.integers(k + g + 4, L - 2))][:i % 2]))
    for i in range(12 if long_texts else 0):
        t, L, typ, g = long_texts[i & 1], (300, 400, 511, 512)[i % 4], i >> 1 & 1, (1, 3, 8)[i % 3]
        draw("offset above 255", lambda: read(t, L, typ, g, (anyk(L, typ, g), int(rng.integers(260, L - g - A - 4)))[i % 3 == 0],
                                              sorted({int(rng.integers(256, L)), int(rng.integers(2, L))})[:1 + i % 2] + [L - 1][:i % 4 == 0]))
    return out


def _pal_reads(rng, brute, q0, spans):
    out = []
    (s4, e4), (sp, ep) = spans["pal4"], spans["palindrome"]
    for i in range(24):
        for _ in range(200):
            g = 1 + i % 3
            if i & 1:
                r = gapped(rng, q0, sp, ep - sp + g, INS, g, int(rng.integers(20, 60)))
            else:
                r = gapped(rng, q0, s4 + int(rng.integers(0, 9)), 80 + g, INS, g, int(rng.integers(20, 56)))
            e, kept = keep(brute.placements(r), 2, 8)
            if e is not None and CLASSES["both strands"](rows_of(brute, r, kept), len(r)):
                break
        else:
            raise AssertionError("no read on both strands")
        out.append(("palindrome" if i & 1 else "pal4", r))
    out += [("random", bytes(rng.choice(list(b"ACGT"), 90).tolist())) for _ in range(6)]
    return out


class Part:
    def __init__(self, name, index, batch, has, brute, extra):
        self.name, self.index, self.brute = name, index, brute
        self.reads = (_reads_of(batch) if batch is not None else []) + [r for _, r in extra]
        order = np.random.default_rng(33).permutation(len(self.reads))
        self.reads = [self.reads[i] for i in order]
        self.batch = _of_reads("gap records " + name, self.reads)
        self.has = _has_record(self.batch, index)
        self.max_read_len = 512 if max(len(r) for r in self.reads) > 256 else 256
        self._rec = {}

    def records(self, M, G):
        """the definition's records of the whole batch under (M, G)"""
        if (M, G) not in self._rec:
            self._rec[M, G] = records(self.index, M, G, self.brute, self.reads, self.has)
        return self._rec[M, G]

    def records_of(self, M, G, lo, hi):
        """... of the piece [lo, hi) of the batch as a batch of its own: a read's records do not depend on its batch, `read` does"""
        rec = self.records(M, G)
        out = rec[(rec["read"] >= lo) & (rec["read"] < hi)].copy()
        out["read"] -= lo
        return out

    def piece(self, lo, hi):
        return _of_reads("reads %d..%d" % (lo, hi), self.reads[lo:hi])

    def in_class(self, name, M=2, G=8):
        """the records of the batch whose read is in the class"""
        rec = self.records(M, G)
        hit = np.zeros(len(rec), dtype=bool)
        for i in np.unique(rec["read"]):
            sel = rec["read"] == i
            rows = [(int(r["path"]), int(r["strand"]), int(r["pos"]), int(r["type"]), int(r["g"]), int(r["d"]), int(r["k"]), tuple(int(x) for x in r["mm"])) for r in rec[sel]]
            if CLASSES[name](rows, len(self.reads[i])):
                hit |= sel
        return rec[hit]


def the_case(tmp_path_factory):
    """-> {"classes": Part, "shapes": Part}"""
    if not _CASE:
        index, batch, _, has, _ = gap_case.case(tmp_path_factory)
        brute = Brute(index, 3)                                      # (gap_case's own stops at M = 2)
        t = path_texts(index)
        clean = [t[0][0][121:], t[2][0], t[4][0], t[6][0][:200]]
        a = Part("classes", index, batch, has, brute, _own_reads(np.random.default_rng(31), brute, clean, []))
        index, batch, _, has, brute, paths = gap_shapes_case.case(tmp_path_factory)
        t = path_texts(index)
        long_texts = [t[paths["l0"]][0], t[paths["l1"]][0]]
        b = Part("shapes", index, batch, has, brute, _own_reads(np.random.default_rng(32), brute, [], long_texts))
        import rescue_records_shapes_case
        c, paths, T, spans = rescue_records_shapes_case.build(tmp_path_factory)
        brute = Brute(c.index, 3)
        pal = Part("pal", c.index, None, None, brute, _pal_reads(np.random.default_rng(34), brute, T["q0"], spans))
        _CASE.append({"classes": a, "shapes": b, "pal": pal})
    return _CASE[0]
