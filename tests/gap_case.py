"""The index and the reads of the gapped-rescue tests (tests/test_gap_def.py on the CPU, tests/test_gap_rescue.py on the device): small
enough for the brute force of tests/gap_def.py, with every input class the definition (include/groot_hip.h, "gapped rescue") tells apart.

Three graphs, about 2 800 bases of text in seven paths:
    graph 0   the eighth graph of test_rescue.py (_extra_graph): an 'N' at a node start (text base 60) and inside a node (120), a 64-base
              reverse-complement palindrome (150 .. 214), a one-base bubble (274); paths q0, q1
    graph 1   four near-identical alleles  U1 . (A | C) . U2 . ("GT" | nothing) . U3:  a0, a1 hold the two bases, a2, a3 do not
    graph 2   one path  U . A x 10 . U . (CAG) x 6 . U . A . AAAAAACCCCCCGGGGG:  a homopolymer run, a 3-mer tandem repeat, and a tail that
              differs from itself shifted by one base in two places only (a read with one base deleted in front of it lies ungapped
              with two substitutions, and gapped with none)"""
import numpy as np

from groot_amd import host
from rescue_def import A, _rc, path_texts
from test_path_pass import _gfa, _seq
from test_rescue import _extra_graph, _mut

LENGTHS = (80, 96, 100, 129, 150)
GAPS = (1, 2, 3, 4, 8, 9)                   # G and G + 1 for G = 1, 3 and 8
TAIL = b"AAAAAACCCCCCGGGGG"
DEL, INS = 0, 1


def build_graphs(rng, tmp):
    """-> the three GFA files"""
    u1, u2, u3 = _seq(rng, 150), _seq(rng, 100), _seq(rng, 150)
    alleles = _gfa(tmp / "alleles.gfa", {1: u1, 2: "A", 3: "C", 4: u2, 5: "GT", 6: u3},
                   [(1, 2), (1, 3), (2, 4), (3, 4), (4, 5), (5, 6), (4, 6)],
                   [("a0", [1, 2, 4, 5, 6]), ("a1", [1, 3, 4, 5, 6]), ("a2", [1, 2, 4, 6]), ("a3", [1, 3, 4, 6])])
    rep = _gfa(tmp / "repeats.gfa", {1: _seq(rng, 109) + "C" + "A" * 10 + "G" + _seq(rng, 89), 2: "T" + "CAG" * 6 + "T" + _seq(rng, 88), 3: _seq(rng, 59) + "TA" + TAIL.decode()},
               [(1, 2), (2, 3)], [("h0", [1, 2, 3])])
    return [_extra_graph(rng, tmp / "g7.gfa"), alleles, rep]


def gapped(rng, t, x, L, typ, g, k, subs=(), fill=None):
    """the read of L bases that lies on text t at x with a gap of g bases behind its first k bases, then substitutions at `subs` (read
    coordinates); an 'N' of the text becomes a random base"""
    if typ == DEL:
        r = t[x:x + k] + t[x + k + g:x + L + g]
    else:
        ins = fill if fill is not None else bytes(rng.choice(list(b"ACGT"), g).tolist())
        r = t[x:x + k] + ins + t[x + k:x + L - g]
    assert len(r) == L, (len(r), L, x, k, g, len(t))
    r = bytes(c if c in b"ACGT" else b"ACGT"[int(rng.integers(4))] for c in r)
    return _mut(rng, r, subs)


def make_reads(rng, texts, M=2):
    """-> [(class name, read)]"""
    out = []
    q0, a0, a2, h0 = texts[0][0], texts[2][0], texts[4][0], texts[6][0]
    clean = [q0[121:], a0, a2, h0[:200]]                                   # stretches without an 'N' and without the repeats

    def put(name, r):
        out.append((name, _rc(r) if len(out) & 1 else r))                  # both strands, in turn

    def place(t, L, typ, g):
        """(x, k) at random with both flanks inside the text"""
        x = int(rng.integers(1, len(t) - L - g - 1))
        return x, int(rng.integers(A + 4, (L if typ == DEL else L - g) - A - 4))

    def away(L, k, g, n):
        """n substitutions at least 3 bases away from the gap and from the ends"""
        ok = [i for i in range(2, L - 2) if i < k - 3 or i > k + g + 3]
        return rng.choice(ok, n, replace=False).tolist()

    n = 0
    for g in GAPS:                                                         # every g up to G, and G + 1
        for typ in (DEL, INS):
            for i in range(10):
                t, L = clean[n % 4], LENGTHS[n % 5]
                n += 1
                x, k = place(t, L, typ, g)
                put("%s%d" % ("DI"[typ], g), gapped(rng, t, x, L, typ, g, k))
    for nm in (M, M + 1):                                                  # M and M + 1 substitutions beside the gap
        for i in range(12):
            t, L, typ, g = clean[i % 4], LENGTHS[i % 5], i & 1, 1 + i % 3
            x, k = place(t, L, typ, g)
            put("subs%d" % nm, gapped(rng, t, x, L, typ, g, k, away(L, k, g, nm)))
    for i in range(40):                                                    # the gap at the first and the last allowed k, and one base outside either
        t, L, typ, g = clean[i % 3], LENGTHS[i % 5], (i >> 2) & 1, 1 + i % 2
        last = (L if typ == DEL else L - g) - A
        name, k = (("k=A", A), ("k=last", last), ("k=A-1", A - 1), ("k=last+1", last + 1))[i % 4]
        while True:                                                        # (a gap that could move one base to the left would be left-aligned away from k)
            x = place(t, L, typ, g)[0]
            r = gapped(rng, t, x, L, typ, g, k)
            if (t[x + k - 1] != t[x + k + g - 1]) if typ == DEL else (r[k + g - 1] != r[k - 1]):
                break
        put(name, r)
    for i in range(72):                                                    # the gap, or the inserted bases, across bases 15/16, 31/32 and 63/64
        t, L, typ, edge = clean[i % 3], LENGTHS[1 + i % 4], i & 1, (16, 32, 64)[(i >> 1) % 3]
        g = 2 + i % 2
        put("edge%d%s" % (edge, "DI"[typ]), gapped(rng, t, place(t, L, typ, g)[0], L, typ, g, edge - typ))
    for i in range(12):                                                    # an INS across the edge of blocks 1 and 2 of an 80-base read, a substitution in all others but one
        keep = (0, 3, 4)[i % 3]
        subs = [A * b + int(rng.integers(1, A - 1)) for b in (0, 3, 4) if b != keep]
        put("straddle", gapped(rng, a0, int(rng.integers(1, 300)), 80, INS, 3, 30, subs))
    for i in range(40):                                                    # W flush with an end of the path, and hanging over it by one base
        t, L, typ, g = (q0[121:], a0, h0)[i % 3], LENGTHS[i % 5], (i >> 2) & 1, 1 + i % 3
        wlen = L + g if typ == DEL else L - g
        ext = _seq(rng, 4).encode() + t + _seq(rng, 4).encode()
        name, x = (("flush0", 4), ("flushend", 4 + len(t) - wlen), ("over0", 3), ("overend", 5 + len(t) - wlen))[i % 4]
        if t is not a0 and name in ("flush0", "over0"):                    # (q0 is cut at 121 and h0's start is what it is: a0 for the left end)
            t, ext = a0, _seq(rng, 4).encode() + a0 + _seq(rng, 4).encode()
        put(name, gapped(rng, ext, x, L, typ, g, place(t, L, typ, g)[1]))
    for i in range(20):                                                    # an 'N' of the path among the deleted bases, and in a flank
        L, g = LENGTHS[i % 4], 1 + i % 3
        if i & 1:
            x = int(rng.integers(121 - L + A, 100))
            put("N flank", gapped(rng, q0, x, L, i >> 1 & 1, g, int(rng.integers(A, L - g - A))))
        else:
            at = (60, 120)[i >> 1 & 1]
            k = int(rng.integers(A + 2, 40))
            put("N deleted", gapped(rng, q0, at - k - int(rng.integers(g)), L, DEL, g, k))
    for i in range(10):                                                    # a gap inside the palindrome
        g = 1 + i % 3
        put("palindrome", gapped(rng, q0, 130, 129, i & 1, g, int(rng.integers(30, 70))))
    run, rep = h0.index(b"A" * 10), h0.index(b"CAG" * 6)
    for i in range(20):                                                    # repeats, where the gap left-aligns
        L, g = LENGTHS[i % 5], 1 + i % 3
        if i & 1:
            put("homopolymer", gapped(rng, h0, run - 30 - i, L, i >> 1 & 1, g, 30 + i + 2 + i % 5, fill=b"A" * g))
        else:
            put("tandem", gapped(rng, h0, rep - 40 - i, L, i >> 1 & 1, 3, 40 + i + 3 * (i % 4), fill=b"CAG"))
    for i in range(10):                                                    # ties over alleles: in front of the bubble base, all four alleles alike
        L = 80 + 4 * i
        put("tie alleles", gapped(rng, a0, 2 + i, L, i & 1, 1 + i % 3, int(rng.integers(A + 4, L - A - 8))))
    for i in range(10):                                                    # ties over types: one of the two bases that a0 has and a2 lacks
        L = LENGTHS[i % 5]
        x = 251 - int(rng.integers(30, L - 30))
        put("tie types", a2[x:251] + (b"G", b"T")[i & 1] + a2[251:x + L - 1])
    for i in range(10):                                                    # ungapped with two substitutions, gapped with none: stays mismatch-rescued
        L = LENGTHS[i % 5]
        end = len(h0)
        put("cheaper gapped", h0[end - 18 - (L - 17):end - 18] + TAIL)
    for i in range(10):                                                    # one base short of A (M + 3) for M = 2
        x, k = place(a0, 79, i & 1, 1)
        put("len79", gapped(rng, a0, x, 79, i & 1, 1, k))
    for i in range(30):                                                    # error-free, and about as long as the index's window: the aligner takes them
        t, L = clean[i % 4], (96, 100)[i >> 2 & 1]
        x = int(rng.integers(1, len(t) - L))
        put("clean", t[x:x + L])
    for i in range(20):
        put("random", _seq(rng, LENGTHS[i % 5]).encode())
    return out


_CASE = {}


def case(tmp_path_factory):
    """(index, batch, class names, has_record, Brute for M <= 2): built once per session, for both test modules"""
    if not _CASE:
        import gap_def
        from test_counter_edges import _of_reads
        from test_rescue import _has_record
        tmp = tmp_path_factory.mktemp("gap")
        # (windows of 100 bases: the aligner takes the error-free reads of 96 and 100 bases, so that the batch holds reads with a record)
        index = host.Index.from_gfa_files(build_graphs(np.random.default_rng(21), tmp), host.index_params(k=7, s=10, w=100))
        texts = path_texts(index)
        assert index.view.n_paths == 7 and all(t is not None and t[1] == 0 for t in texts) and sum(len(t[0]) for t in texts) <= 6000
        named = make_reads(np.random.default_rng(22), texts)
        named = [named[i] for i in np.random.default_rng(23).permutation(len(named))]
        batch = _of_reads("gap classes", [r for _, r in named])
        _CASE["case"] = (index, batch, [n for n, _ in named], _has_record(batch, index), gap_def.Brute(index, 2))
    return _CASE["case"]
