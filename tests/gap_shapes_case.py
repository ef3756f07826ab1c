"""The index and the reads of tests/test_gap_shapes.py: gapped rescue (kernels_gap.hpp) at the shapes tests/gap_case.py does not reach,
small enough for the brute force of tests/gap_def.py.

Five graphs, about 4 900 bases of text in thirteen paths.  The first four are those of tests/test_rescue_shapes.py (r0, r1 | gap, full |
main, p11, p46 | l0, l1: tandem repeats and homopolymer runs, a text-less path, two short paths, two long ones), the fifth is built here:

    m300 = 10 . 30 . 260 bases
    p72  = 10 . 30 . 32      the 32 differ from m300's next 32 in every base: an INS read of 72 + g bases, or a DEL read of 72 - g, fills it
    p81  = 10 . 30 . 41      the same with 41 bases, by another substitution of the bases
    rep  = 10 . 30 . 20 u . W16 x 8 . 40 u . W20 x 7 . 40 u . (ACG) x 30 . 60 u      repeats longer than a read of 100 bases; rep is the
                             last path of the index

A Position is the running length over the path's own nodes (create_groot_graph), so the first Position of every path a GFA file gives is 0:
a text that starts elsewhere cannot be built with _gfa, and there is none here."""
import numpy as np

from gap_case import gapped
from groot_amd import host
from rescue_def import A, _rc, path_texts
from test_path_pass import _gfa, _seq
from test_rescue import _mut
from test_rescue_shapes import LONG, _long_graph, _no_text_graph, _repeat_graph, _short_graph

DEL, INS = 0, 1
PATHS = ("r0", "r1", "gap", "full", "main", "p11", "p46", "l0", "l1", "m300", "p72", "p81", "rep")
REP_LENGTHS = (80, 96, 100)
INS_WORDS = ((129, 1), (131, 3), (257, 1), (264, 8), (481, 1), (488, 8))      # len - g = 128, 256, 480
_SWAPS = [bytes.maketrans(b"ACGT", x) for x in (b"CATG", b"GTAC", b"TGCA")]     # three ways of every base to another one, no two alike


def _fifth_graph(rng, path):
    """-> (file, {class: (first base in rep, behind the last, period)})"""
    c = _seq(rng, 260)
    w16, w20 = _seq(rng, 16), _seq(rng, 20)
    sw = lambda s, i: s.encode().translate(_SWAPS[i]).decode()
    parts = [(None, sw(c[0], 2) + _seq(rng, 19)), ("rep16", w16 * 8), (None, _seq(rng, 40, w16[0])), ("rep20", w20 * 7), (None, _seq(rng, 40, w20[0])),
             ("period3", "ACG" * 30), (None, _seq(rng, 60, "A"))]
    spans, at = {}, 40
    for name, s in parts:
        if name:
            spans[name] = (at, at + len(s), {"rep16": 16, "rep20": 20, "period3": 3}[name])
        at += len(s)
    nodes = {1: _seq(rng, 10), 2: _seq(rng, 30), 3: c, 4: sw(c[:32], 0), 5: sw(c[:41], 1), 6: "".join(s for _, s in parts)}
    f = _gfa(path, nodes, [(1, 2), (2, 3), (2, 4), (2, 5), (2, 6)], [("m300", [1, 2, 3]), ("p72", [1, 2, 4]), ("p81", [1, 2, 5]), ("rep", [1, 2, 6])])
    return f, spans


def build_index(tmp):
    """-> (index, texts by path name, spans of the fifth graph's repeats, spans of r0's repeats, the text-less path's spelling, its landmarks)"""
    rng = np.random.default_rng(41)
    f0, spans0 = _repeat_graph(rng, tmp / "g0.gfa")
    f1, gap, gap_at = _no_text_graph(rng, tmp / "g1.gfa")
    f4, spans = _fifth_graph(rng, tmp / "g4.gfa")
    files = [f0, f1, _short_graph(rng, tmp / "g2.gfa"), _long_graph(rng, tmp / "g3.gfa"), f4]
    index = host.Index.from_gfa_files(files, host.index_params(k=7, s=10, w=64))
    return index, spans, spans0, gap, gap_at


def make_reads(rng, T, spans, spans0, gap, gap_at, M=2):
    """T: {path name: text} -> [(class name, read)]"""
    out = []
    clean = [T["full"], T["main"][40:], T["l0"], T["m300"][40:]]                # unique sequence

    def put(name, r):
        out.append((name, _rc(r) if len(out) & 1 else r))                      # both strands, in turn

    def away(L, k, g, n, lo=2):
        """n substitutions at least 3 bases away from the gap and from the ends"""
        ok = [i for i in range(lo, L - 2) if i < k - 3 or i > k + g + 3]
        return rng.choice(ok, n, replace=False).tolist()

    def pinned(t, L, typ, g, k, x=None, subs=(), tries=200):
        """the read with its gap at k exactly: one that could move a base to the left is drawn again (other x, other inserted bases)"""
        wlen = L + g if typ == DEL else L - g
        for _ in range(tries):
            at = int(rng.integers(0, len(t) - wlen + 1)) if x is None else x
            r = gapped(rng, t, at, L, typ, g, k)
            if (t[at + k - 1] != t[at + k + g - 1]) if typ == DEL else (r[k + g - 1] != r[k - 1]):
                return _mut(rng, r, subs)
        raise AssertionError(("no pinned gap", L, typ, g, k, x))

    # repeats longer than the read: a substitution in every block before `keep`, the gap behind block `keep`
    rep = T["rep"]
    for name in ("rep16", "rep20"):
        s, e, per = spans[name]
        for L in REP_LENGTHS:
            for typ in (DEL, INS):
                for g in (1, 2, 3):
                    for keep in range(4):
                        kmax = (L if typ == DEL else L - g) - A
                        if A * (keep + 1) > kmax:
                            continue
                        wlen = L + g if typ == DEL else L - g
                        x = int(rng.integers(s - 30, e - wlen + 31)) if (g + keep) & 1 else int(rng.integers(s, e - wlen + 1))      # over one edge | inside
                        k = int(rng.integers(A * (keep + 1), kmax + 1))
                        subs = [A * b + int(rng.integers(A)) for b in range(keep)]
                        put("%s/keep%d" % (name, keep), gapped(rng, rep, x, L, typ, g, k, subs))
    s, e, _ = spans["rep16"]
    for i in range(16):                                                        # four copies one period apart: the window starts in the repeat's first bases
        g, keep = 1 + i % 3, i % 3
        put("rep16/many", gapped(rng, rep, s + int(rng.integers(0, g + 1)), 80, INS, g, int(rng.integers(A * (keep + 1), 80 - g - A + 1)),
                                 [A * b + int(rng.integers(A)) for b in range(keep)]))
    # a gap of one whole period, the read hanging out of both ends of the repeat: k* is the repeat's start, or A when that is nearer to the read's start
    s, e, _ = spans["period3"]
    for i in range(24):
        off, typ = (5, 9, 12, 15, 16, 17, 20, 25)[i % 8], i & 1
        L = (129, 150)[i >> 1 & 1]
        put("whole period/ACG", gapped(rng, rep, s - off, L, typ, 3, off + 3 * (i % 7), fill=b"ACG"))
    (sa, ea, _), = [x for x in spans0["homopolymer"] if x[1] - x[0] == 72]
    for i in range(24):
        off, typ, g = (8, 10, 12, 14, 15, 16, 17, 18)[i % 8], i & 1, 1 + i % 3
        put("whole period/A", gapped(rng, T["r0"], sa - off, 96, typ, g, off + i % 40, fill=b"A" * g))
    # poly-A, poly-T and poly-G blocks as the only clean block of an 80-base read: block 1 lies in the run, the inserted bases spoil blocks
    # 2 and 3, a substitution each spoils blocks 0 and 4
    for run, base in ((0, b"A"), (1, b"T"), (2, b"G")):
        s, e, _ = spans0["homopolymer"][run]
        assert T["r0"][s:e] == base * 40
        for i in range(12):
            x = s - int(rng.integers(1, 9))                                     # the run covers read bases 1..8 to 41..48
            g = 2 + i % 2                                                       # the inserted bases lie on both sides of read base 48
            subs = [int(rng.integers(0, s - x)), 64 + int(rng.integers(0, A))]
            put("poly" + base.decode(), pinned(T["r0"], 80, INS, g, 47 - (i >> 1) % (g - 1), x=x, subs=subs))
    # the short paths: filled exactly, and one base too long on either side
    for name in ("p72", "p81"):
        t = T[name]
        for typ in (DEL, INS):
            for g in range(1, 9):
                L = len(t) - g if typ == DEL else len(t) + g
                k = int(rng.integers(A + 2, (L if typ == DEL else L - g) - A - 1))
                put("fit/" + "DI"[typ], gapped(rng, t, 0, L, typ, g, k, away(L, k, g, g & 1)))
                ext = (_seq(rng, 1).encode() + t) if g & 1 else (t + _seq(rng, 1).encode())
                put("over/" + "DI"[typ], gapped(rng, ext, 0, L + 1, typ, g, k + (g & 1)))
    for i in range(48):                                                        # reads of a main path that begin where the short paths still run beside it
        t, first = ((T["m300"], 72), (T["main"], 46))[i % 3 == 2]
        L, typ, g = (64, 80, 96)[i % 3], i >> 1 & 1, 1 + i % 3
        x = int(rng.integers(0, first))
        k = int(rng.integers(A, (L if typ == DEL else L - g) - A + 1))
        put("short/main", gapped(rng, t, x, L, typ, g, k, away(L, k, g, i % 2)))
    # the text-less path: its own spelling over the missing junction and through the node it alone holds, with a gap elsewhere; its neighbour
    j13, s5, e5 = gap_at
    for i in range(20):
        L, typ, g = (80, 96, 100)[i % 3], i & 1, 1 + i % 3
        lo, hi = (j13 - L + 24, j13 - 24) if i < 10 else (max(s5 + 24 - L, j13), min(e5 - 24, len(gap) - L - g))
        x = int(rng.integers(max(lo, 0), hi + 1))
        cut = (j13 if i < 10 else s5 + 12) - x                                  # read base of the junction / inside the lone node
        k = int(rng.integers(A, cut - 4)) if cut - 4 > A + 2 and i & 2 else int(rng.integers(min(cut + 8, L - g - A), L - g - A + 1))
        put("gap", gapped(rng, gap, x, L, typ, g, k))
    full = T["full"]
    for i in range(36):
        L, typ, g = (64, 80, 96, 100)[i % 4], i & 1, 1 + i % 8
        wlen = L + g if typ == DEL else L - g
        k = int(rng.integers(A, wlen - g - A + 1)) if typ == INS else int(rng.integers(A, L - A + 1))
        put("full", gapped(rng, full, int(rng.integers(0, len(full) - wlen + 1)), L, typ, g, k, away(L, k, g, int(i % 3 == 0))))
    # long reads: the cut on and beside word edges, at kmax and at A
    for L in LONG:
        n = 0
        for rnd in range(2):
            for ki in range(8):
                typ, g = (ki + rnd) & 1, (1, 8)[((ki >> 1) + rnd) & 1]
                ls = L if typ == DEL else L - g
                kmax = ls - A
                mid, last = 32 * max(1, round(ls / 64)), 32 * (kmax // 32)
                k = (mid - 1, mid, mid + 1, last - 1, last, last + 1, kmax, A)[ki]
                if not A <= k <= kmax:
                    k = kmax - ki
                edges = [w for w in range(32, L - 2, 32) if abs(w - k) > 12 and abs(w - k - g) > 12]
                subs = []
                for j in range((n + rnd) % (M + 1)):                             # 0 .. M substitutions, on the last base before / the first behind a word edge
                    w = edges[int(rng.integers(len(edges)))]
                    subs.append(w - 1 if j & 1 else w)
                put("long", pinned((T["l0"], T["l1"])[n & 1], L, typ, g, k, subs=sorted(set(subs))))
                n += 1
    for i, (L, g) in enumerate(INS_WORDS * 2):                                 # INS with len - g a multiple of 32
        ls = L - g
        k = (ls - A, 32 * ((ls - A) // 32))[i >= len(INS_WORDS)]
        put("long/ins words", pinned(T["l0"], L, INS, g, k, subs=[ls // 2][:i & 1]))
    for i in range(12):                                                        # the inserted bases over a 64-bit word edge of the read
        L, g = (160, 257, 300, 512)[i % 4], (2, 3, 8)[i % 3]
        w = 32 * int(rng.integers(1, (L - g - A) // 32 + 1))
        put("long/ins straddle", pinned(T["l1"], L, INS, g, w - g // 2 - (g & 1)))
    # M = 3: 96 bases are six blocks
    for i in range(28):                                                        # (an inserted base that equals the text's leaves a second block clean: some do)
        t = clean[i % 4]
        g, edge = 2 + i % 2, A * (2 + i % 3)                                    # the inserted bases across the edge of blocks 1|2, 2|3, 3|4
        spoilt = {edge // A - 1, edge // A}
        free = [b for b in range(6) if b not in spoilt]
        keep = free[i % 4]
        subs = [A * b + int(rng.integers(2, A - 2)) for b in free if b != keep]
        put("m3/ins", pinned(t, 96, INS, g, edge - 1, subs=subs))
    for i in range(12):
        t, typ, g = clean[i % 4], DEL, 1 + i % 3
        k = int(rng.integers(A + 4, 96 - A - 4))
        put("m3/del", gapped(rng, t, int(rng.integers(1, len(t) - 110)), 96, typ, g, k, away(96, k, g, 3)))
    for i in range(12):
        t, typ, g = clean[i % 4], i & 1, 1 + i % 3
        k = int(rng.integers(A + 4, 95 - g - A - 4))
        put("m3/len95", gapped(rng, t, int(rng.integers(1, len(t) - 110)), 95, typ, g, k, away(95, k, g, i % 3)))
    for i in range(12):
        t, typ, g = clean[i % 4], i & 1, 1 + i % 3
        L = (96, 100, 160)[i % 3]
        k = int(rng.integers(A + 4, L - g - A - 4))
        put("m3/d4", gapped(rng, t, int(rng.integers(1, len(t) - L - 10)), L, typ, g, k, away(L, k, g, 4)))
    # the window flush with the start of the first path of the index, and with the end of the last
    for i in range(7):
        L = (159, 160, 192, 256, 300, 480, 500)[i]
        put("flush first", gapped(rng, T["r0"], 0, L, DEL, 8, int(rng.integers(A, 50))))
        put("flush last", gapped(rng, rep, len(rep) - L - 8, L, DEL, 8, L - int(rng.integers(A, 28))))
    # controls
    for i, L in enumerate((64, 80, 96, 100, 150) + LONG):
        put("random", _seq(rng, L).encode())
        put("random", _seq(rng, L).encode())
    for i in range(24):                                                        # error-free: the aligner takes them
        t, L = clean[i % 4], (64, 66, 70)[i % 3]                                # (about as long as the index's window)
        x = int(rng.integers(1, len(t) - L))
        put("clean", t[x:x + L])
    for i in range(24):                                                        # one substitution: mismatch rescue takes them, gapped rescue never looks
        t, L = clean[i % 4], (64, 100, 160)[i % 3]
        x = int(rng.integers(1, len(t) - L))
        put("ungapped", _mut(rng, t[x:x + L], [int(rng.integers(4, L - 4))]))
    return out


_CASE = {}


def case(tmp_path_factory):
    """(index, batch, class names, has_record, Brute for M <= 3, {path name: global path}): built once per session"""
    if not _CASE:
        import gap_def
        from test_counter_edges import _of_reads
        from test_rescue import _has_record
        index, spans, spans0, gap, gap_at = build_index(tmp_path_factory.mktemp("gap_shapes"))
        texts = path_texts(index)
        paths = dict(zip(PATHS, range(len(PATHS))))
        assert index.view.n_paths == len(PATHS)
        T = {n: texts[p][0] for n, p in paths.items() if texts[p] is not None}
        named = make_reads(np.random.default_rng(42), T, spans, spans0, gap, gap_at)
        named = [named[i] for i in np.random.default_rng(43).permutation(len(named))]
        batch = _of_reads("gap shapes", [r for _, r in named])
        _CASE["case"] = (index, batch, [n for n, _ in named], _has_record(batch, index), gap_def.Brute(index, 3), paths)
    return _CASE["case"]
