"""The index and the reads of tests/test_rescue_records_shapes.py: the rescued records (kernels_rescue_rec.hpp) at the shapes
tests/test_rescue_records.py does not reach, with the definition's records per M (tests/rescue_records_def.py).  CPU only.

Six graphs, thirteen paths, path_words == 1.  The first five graphs and their seeds are those of tests/rescue_sets_shapes_case.py (r0, r1 |
gap, full | main, p11, p46 | l0, l1 | r0b, r1b), and the batch begins with that module's batch, read for read.  The sixth graph is made of
reverse-complement palindromes, on the paths q0 and q1 (they differ in one bubble base behind everything named here):

    60 u . (ACGT)x24 . 40 u . (AT)x40 . 40 u . H rc(H) with 40 bases of H . 40 u . (A | C) . 60 u

A window of (ACGT)x24 or of (AT)x40 is its own reverse complement up to a shift, so a read from there has kept placements on BOTH strands of
one path.  A window of the period-4 repeat that begins with C or T has its strand-1 copies two bases away from its strand-0 copies: the two
strands interleave in pos.  One that begins with A or G, and every window of the period-2 repeat, has both strands at the same pos.  In
either case the list's order -- (read, path, strand, pos): all of strand 0, then all of strand 1 -- differs from (read, path, pos, strand),
which no read of tests/rescue_records_case.py and none of the first five graphs here can tell apart.  The classes behind the batch:

    pal4, pal2      48 / 64 / 80 bases of the period-4 and the period-2 repeat with 1, 2 and 3 substitutions, both input strands; among them a
                    substitution in the first base, in the last base, and one in every 16-base block but the last (the first clean block
                    -- the anchor -- is the last one);
    palindrome      windows centred on the 80-base palindrome, 1 .. 3 substitutions: both strands at the same pos;
    palindrome/off  windows that hang 12 .. 20 bases out of it into unique sequence: one strand only;
    palindrome/in   windows inside it and off its centre: one placement on each strand, at mirrored pos;
    pal/edge        windows of the period-4 repeat that hang 8 .. 16 bases out of either end into unique sequence: a shifted copy would put
                    the unique bases onto the repeat, and the reverse complement puts them at the other end, so such a read keeps the one
                    placement it was cut from, on one strand.  (The (read, path) pairs with both strands at different sets of pos are those
                    of pal4 that begin with C or T and of palindrome/in.);
    long/at         reads of 300 .. 512 bases of l0 / l1 with a substitution at offset 255, 256, 287, 288, 479, 480, 510 or 511 of the
                    oriented read, both strands: either side of the word edges of rescue_diff and the last bits of the last word.

The expectation comes from rescue_records_def.records and the oracle's records (test_rescue._has_record) only.

Not covered: a path whose first node's Position is not 0.  A Position is the running length over the path's own nodes, so every path a GFA
file gives starts at 0 (tests/gap_shapes_case.py); the hand-worked cases of tests/test_rescue_records_def.py keep the definition's
X = first Position + offset."""
import numpy as np

import rescue_sets_shapes_case as sets_shapes
from groot_amd import host
from rescue_def import Tables, _rc, path_texts
from rescue_records_def import RECORD_DTYPE, records
from test_counter_edges import _of_reads
from test_path_pass import _gfa, _seq
from test_rescue import _has_record, _mut, _reads_of
from test_rescue_shapes import _long_graph, _no_text_graph, _repeat_graph, _short_graph

PATHS = sets_shapes.PATHS + ("q0", "q1")
OFFSETS = (255, 256, 287, 288, 479, 480, 510, 511)
PAL_LENGTHS = (48, 64, 80)


def _palindromic_graph(rng, path):
    """-> (file, {name: (first base, behind the last)} of the period-4 repeat, the period-2 repeat and the palindrome)"""
    half = _seq(rng, 40).encode()
    parts = [(None, _seq(rng, 60)), ("pal4", "ACGT" * 24), (None, _seq(rng, 40, "A")), ("pal2", "AT" * 40), (None, _seq(rng, 40, "A")),
             ("palindrome", (half + _rc(half)).decode()), (None, _seq(rng, 40))]
    spans, at = {}, 0
    for name, s in parts:
        if name:
            spans[name] = (at, at + len(s))
        at += len(s)
    nodes = {1: "".join(s for _, s in parts), 2: "A", 3: "C", 4: _seq(rng, 60)}
    return _gfa(path, nodes, [(1, 2), (1, 3), (2, 4), (3, 4)], [("q0", [1, 2, 4]), ("q1", [1, 3, 4])]), spans


def _more_reads(rng, T, spans):
    """-> [(class name, read)] behind the batch of rescue_sets_shapes_case"""
    out = []
    q0, l0, l1 = T["q0"], T["l0"], T["l1"]

    def add(name, t, x, L, at, strand=None):
        assert 0 <= x and x + L <= len(t), (name, x, L, len(t))
        s = _mut(rng, t[x:x + L], at)
        out.append((name, _rc(s) if (len(out) & 1 if strand is None else strand) else s))

    def subs(L, n, k):
        """n offsets: the first base, the last base, one in every block but the last (n of them at most), or anywhere"""
        if k % 4 == 0:
            return [0] + rng.choice(np.arange(1, L), n - 1, replace=False).tolist()
        if k % 4 == 1:
            return [L - 1] + rng.choice(L - 1, n - 1, replace=False).tolist()
        if k % 4 == 2 and n == L // 16 - 1:
            return [16 * b + int(rng.integers(16)) for b in range(n)]
        return rng.choice(L, n, replace=False).tolist()

    for name in ("pal4", "pal2"):
        s, e = spans[name]
        for L in PAL_LENGTHS:
            for n in (1, 2, 3):
                for k in range(8):                               # (every phase of the period, both input strands)
                    room = e - s - L
                    phase = k % 4 if room else 0
                    add(name, q0, s + phase + 4 * int(rng.integers(0, (room - phase) // 4 + 1)), L, subs(L, n, k), strand=k >> 2 & 1)
    s, e = spans["palindrome"]
    for L in PAL_LENGTHS:
        for n in (1, 2, 3):
            for k in range(4):
                add("palindrome", q0, s + (e - s - L) // 2, L, subs(L, n, k + 2))
        for k in range(8):
            h = 12 + k                                           # bases outside the palindrome, to its left or to its right
            add("palindrome/off", q0, s - h if k & 1 else e + h - L, L, subs(L, 1 + k % 2, 3))
    for k in range(24):                                          # inside the 80 bases, 1 .. 16 bases off the centre
        L = PAL_LENGTHS[k % 2]
        c = s + (e - s - L) // 2
        by = 1 + int(rng.integers(min(16, c - s)))
        add("palindrome/in", q0, c - by if k & 2 else c + by, L, subs(L, 1 + k % 2, 3))
    s, e = spans["pal4"]
    for k in range(36):
        L, h = PAL_LENGTHS[k % 3], 8 + k % 9
        add("pal/edge", q0, s - h if k & 1 else e + h - L, L, subs(L, 1 + k % 3, k))
    for at in OFFSETS:                                           # the offset in the ORIENTED read: the read is reversed after the substitution
        for k in range(16):
            L = 512 if k & 1 else max(at + 1, 300)
            more = [] if k % 3 else [int(rng.integers(at - 1))]
            add("long/at", (l0, l1)[k >> 1 & 1], int(rng.integers(0, len(l0) - L + 1)), L, [at] + more, strand=k >> 2 & 1)
    return out


class RecordsShapes:
    """the definition's records of any batch over one index, cached per M; the windows of the texts are shared by every M and every batch"""

    def __init__(self, index, batch, names=None, win=None):
        self.index, self.batch, self.names = index, batch, names
        self.reads = _reads_of(batch)
        self.has = _has_record(batch, index)
        self._win, self._rec = {} if win is None else win, {}

    def of(self, batch):
        """the same over another batch of this index"""
        return RecordsShapes(self.index, batch, win=self._win)

    def tables(self, M):
        t = Tables(self.index, M)
        t._win = self._win
        return t

    def records(self, M):
        """the definition's records of the whole batch under M"""
        if M not in self._rec:
            self._rec[M] = records(self.index, M, self.reads, self.has, self.tables(M))
        return self._rec[M]

    def records_for(self, M, idx):
        """... of the reads `idx` of the batch, in that order, as a batch of their own: a read's records do not depend on its batch or on
        its place in it, `read` does"""
        rec = self.records(M)
        lo, hi = np.searchsorted(rec["read"], idx, side="left"), np.searchsorted(rec["read"], idx, side="right")
        out = np.concatenate([rec[a:b] for a, b in zip(lo, hi)] + [rec[:0]])
        out["read"] = np.repeat(np.arange(len(lo), dtype=np.int64), hi - lo)
        return out

    def records_of(self, M, lo, hi):
        return self.records_for(M, np.arange(lo, hi))

    def per_read(self, M):
        """the number of records of every read of the batch"""
        return np.bincount(self.records(M)["read"].astype(np.int64), minlength=self.batch.n)

    def piece(self, lo, hi):
        return self.pick(np.arange(lo, hi))

    def pick(self, idx):
        return _of_reads("%d reads" % len(idx), [self.reads[i] for i in idx])


_CASE = {}


def build(tmp_path_factory):
    """-> (RecordsShapes of the batch of every class with its class names, {path name: global path}, {path name: text}, the spans of the
    sixth graph): built once per process"""
    if not _CASE:
        before, _, T5 = sets_shapes.build(tmp_path_factory)     # its batch, read for read, and the texts of its eleven paths
        tmp = tmp_path_factory.mktemp("rescue_records_shapes")
        rng = np.random.default_rng(31)                          # the first five graphs: the seeds and the order of sets_shapes.build
        f0, _ = _repeat_graph(rng, tmp / "g0.gfa")
        files = [f0, _no_text_graph(rng, tmp / "g1.gfa")[0], _short_graph(rng, tmp / "g2.gfa"), _long_graph(rng, tmp / "g3.gfa")]
        again = tmp / "g4.gfa"
        again.write_text(open(f0).read().replace("P\tr0\t", "P\tr0b\t").replace("P\tr1\t", "P\tr1b\t"))
        f5, spans = _palindromic_graph(np.random.default_rng(41), tmp / "g5.gfa")      # (a generator of its own: the five stay as they are)
        index = host.Index.from_gfa_files(files + [str(again), f5], host.index_params(k=7, s=10, w=64))
        texts = path_texts(index)
        paths = dict(zip(PATHS, range(len(PATHS))))
        assert index.view.n_paths == len(PATHS) == 13 and index.view.path_words == 1 and index.view.n_graphs == 6
        assert [t is None for t in texts] == [n == "gap" for n in PATHS]
        assert all(t[1] == 0 and len(t[0]) == int(index.arrays["path_len"][p]) for p, t in enumerate(texts) if t is not None)
        T = {n: texts[p][0] for n, p in paths.items() if texts[p] is not None}
        assert all(T[n] == T5[n] for n in T5) and set(T) == set(T5) | {"q0", "q1"}
        q0, q1 = T["q0"], T["q1"]
        (s4, e4), (s2, e2), (sp, ep) = spans["pal4"], spans["pal2"], spans["palindrome"]
        assert (s4, e4, s2, e2, sp, ep) == (60, 156, 196, 276, 316, 396) and len(q0) == len(q1) == 497
        assert q0[s4:e4] == b"ACGT" * 24 and q0[s2:e2] == b"AT" * 40 and _rc(q0[sp:ep]) == q0[sp:ep] and q0[sp:sp + 40] != q0[sp + 40:ep]
        assert q0[e4:e4 + 1] != b"A" and q0[e2:e2 + 1] != b"A"
        assert q0[:436] == q1[:436] and (q0[436:437], q1[436:437]) == (b"A", b"C") and q0[437:] == q1[437:]
        named = list(zip(before.names, before.reads))
        more = _more_reads(np.random.default_rng(42), T, spans)
        named += [more[i] for i in np.random.default_rng(43).permutation(len(more))]
        batch = _of_reads("record shapes", [r for _, r in named])
        assert batch.n == before.batch.n + len(more) < 4000
        _CASE["case"] = (RecordsShapes(index, batch, [n for n, _ in named]), paths, T, spans)
    return _CASE["case"]


def five_pieces(c):
    """the five pieces of rescue_sets_shapes_case.five_pieces -- the long reads in a piece of their own, in the middle -- as
    [(batch, the reads' places in the whole batch)]"""
    long = [i for i, n in enumerate(c.names) if n.startswith("long")]
    rest = [i for i, n in enumerate(c.names) if not n.startswith("long")]
    cuts = [0, len(rest) // 4, len(rest) // 2, 3 * len(rest) // 4, len(rest)]
    idx = [rest[a:b] for a, b in zip(cuts, cuts[1:])]
    idx.insert(2, long)
    pieces = [(c.pick(i), np.array(i)) for i in idx]
    assert len(pieces) == 5 and min(len(c.reads[i]) for i in long) >= 159 and sum(p.n for p, _ in pieces) == c.batch.n
    # (a read's records do not depend on its batch: the pieces' candidates are the batch's)
    assert all(np.array_equal(_has_record(p, c.index), c.has[i]) for p, i in pieces)
    return pieces


def redone_piece(c):
    """a sixth piece for GROOT_TEST_SMALL_BUFFERS, whose record buffers start with room for 64: every read of the batch that has a record
    and the batch's first 150 reads -> (batch, the reads' places).  A mapped read has a record at least, so its pass is redone for certain"""
    idx = np.r_[np.flatnonzero(c.has), np.arange(150)]
    p = c.pick(idx)
    assert np.array_equal(_has_record(p, c.index), c.has[idx]) and int(c.has.sum()) > 2 * 64 and len(np.unique(c.records_of(2, 0, 150)["read"])) >= 20
    return p, idx


def sort_by(rec, order):
    return np.sort(rec, order=list(order))


def order_sensitive(rec):
    """the reads whose records come out differently under (read, path, pos, strand) order"""
    other = sort_by(rec, ("read", "path", "pos", "strand"))
    return np.unique(rec["read"][(rec["pos"] != other["pos"]) | (rec["strand"] != other["strand"])])


def classes(c, paths, M):
    """the number of records (of reads, of (read, path) pairs, where the name says so) of every input class under M"""
    rec = c.records(M)
    assert rec.dtype == RECORD_DTYPE and np.array_equal(rec, sort_by(rec, ("read", "path", "strand", "pos")))
    read, path, pos, strand = (rec[k].astype(np.int64) for k in ("read", "path", "pos", "strand"))
    L = np.array([len(r) for r in c.reads], dtype=np.int64)[read]
    plen = c.index.arrays["path_len"].astype(np.int64)
    mm = np.where(np.arange(3) < rec["d"][:, None], rec["mm"].astype(np.int64), -1)
    per_read = c.per_read(M)
    # per (read, path): the sets of pos of the two strands
    pos_of = {}
    for r, p, s, x in zip(read.tolist(), path.tolist(), strand.tolist(), pos.tolist()):
        pos_of.setdefault((r, p), (set(), set()))[s].add(x)
    both = {k: v for k, v in pos_of.items() if v[0] and v[1]}
    paths_of = np.unique(np.stack([read, path], axis=1), axis=0)
    long_path = plen[path] > 256
    p46 = path == paths["p46"]
    out = {"records": len(rec), "reads": int((per_read > 0).sum()), "most_of_one_read": int(per_read.max()),
           "order_sensitive_reads": len(order_sensitive(rec)),
           "both_strands": len(both),
           "both_strands_other_pos": sum(v[0] != v[1] for v in both.values()),
           "both_strands_one_pos": sum(len(v[0] & v[1]) for v in both.values()),
           "reads_64_records": int((per_read >= 64).sum()), "reads_100_records": int((per_read >= 100).sum()),
           "reads_on_4_paths": int((np.bincount(paths_of[:, 0]) >= 4).sum()),
           "of_long_reads": int((L > 256).sum()),
           "offset_256_up": int((mm >= 256).any(axis=1).sum()),
           "d": np.bincount(rec["d"], minlength=4).tolist(),
           "pos_0_long_path": int(((pos == 0) & long_path).sum()), "last_base_long_path": int(((pos + L == plen[path]) & long_path).sum()),
           "pos_0_p46": int(((pos == 0) & p46).sum()), "last_base_p46": int(((pos + L == plen[path]) & p46).sum()),
           "on_textless_or_p11": int(np.isin(path, [paths["gap"], paths["p11"]]).sum())}
    for at in OFFSETS:
        out["offset_%d" % at] = int((mm == at).any(axis=1).sum())
    for s in (0, 1):
        out["offset_0_strand_%d" % s] = int(((mm == 0).any(axis=1) & (strand == s)).sum())
        out["offset_last_strand_%d" % s] = int(((mm == (L - 1)[:, None]).any(axis=1) & (strand == s)).sum())
    by_class = {}
    for r in order_sensitive(rec).tolist():
        by_class[c.names[r]] = by_class.get(c.names[r], 0) + 1
    out["order_sensitive_by_class"] = by_class
    other = {}
    for (r, p), v in both.items():
        if v[0] != v[1]:
            other[c.names[r]] = other.get(c.names[r], 0) + 1
    out["both_strands_other_pos_by_class"] = other
    return out
