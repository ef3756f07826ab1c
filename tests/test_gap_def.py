"""The brute force of gapped rescue (tests/gap_def.py) on cases worked by hand, and the inputs of tests/test_gap_rescue.py: every class
the definition tells apart is there.  No GPU.

The definition (include/groot_hip.h, "gapped rescue"), restated:

    M, A = 16, texts, path coordinates, 'N', CANDIDATE, oriented read, strand: exactly mismatch rescue's (tests/test_rescue.py).
    G = max gap length, 1 <= G <= 8.
    A GAP CANDIDATE is a candidate of mismatch rescue that is NOT rescued (no ungapped placement with d <= M) and has len >= A * (M + 3).
    A GAPPED PLACEMENT of r is (p, strand, x, type, g, k), 1 <= g <= G, with the oriented read R (len bases) and T = text_p:
       type DEL:   R[0,k) on T[x, x+k),  R[k,len) on T[x+k+g, x+len+g);   A <= k <= len - A;       W = T[x, x+len+g)
       type INS:   R[0,k) on T[x, x+k),  R[k+g,len) on T[x+k, x+len-g);   A <= k <= len - g - A;   W = T[x, x+len-g);  R[k,k+g) is inserted
       W lies inside the text's bases inside path_len and holds no 'N'.   d(k) = the mismatching bases of the two aligned parts.
    For fixed (p, strand, x, type, g):  d = min over the allowed k of d(k);  k* = the SMALLEST k with d(k) = d;  the placement exists when
       d <= M; its cost is e = d + g.
    e*(r) = the smallest e over r's gapped placements; the KEPT ones are all those with e = e*, each (p, strand, x, type, g) once.
    Per kept placement (X = first Position of the path + x):  gdepth += 1 on DEL: [X, X+k*) and [X+k*+g, X+len+g);  INS: [X, X+len-g);
       event (p, pos = X + k* - 1, type, g, seq) += 1,  seq = R[k*, k*+g) at 2 bits per base (A C G T = 0 1 2 3) for INS, 0 for DEL.
    Stats: gap candidates, gap-rescued, kept placements, kept DEL, kept INS, too short for a gap, distinct events, events dropped."""
import numpy as np
import pytest

import gap_case
from gap_def import DEL, INS, Brute, GapTables, event_of, keep
from rescue_def import A, _rc
from test_rescue import _reads_of

L20 = b"CTGACCATGGTCAAGTCGTC"         # ends with C
R20 = b"GGATCCTTAGCAGTCTAGGT"         # starts with G
B16, C16 = L20[:16], R20[:16]         # B16 ends with T


def _brute(*texts, m_max=2):
    return Brute(None, m_max, [(t, 0) for t in texts])


def test_del_in_a_homopolymer_is_left_aligned():
    """T = L20 AAAAA R20, the read lacks one A: every cut k = 20 .. 24 inside the run gives d = 0, k* = 20 is the smallest.
    d = 0, e = 1, event (path 0, pos 19, DEL, 1)"""
    read = L20 + b"AAAA" + R20
    pl = _brute(L20 + b"AAAAA" + R20).placements(read)
    e, kept = keep(pl, 2, 3)
    assert (e, kept) == (1, [(0, 0, 0, DEL, 1, 0, 20)])
    assert event_of(kept[0], read) == (0, 19, DEL, 1, 0)


def test_ins_in_a_dinucleotide_repeat_left_aligns_onto_k_A():
    """T = B16 ACACAC R20, the read has one AC more: every k = 16 .. 22 gives d = 0 (k = 17 inserts CA), k* = 16 = A, the first allowed cut.
    W is the whole text.  d = 0, e = 2, event (path 0, pos 15, INS, 2, seq "AC" = 0 | 1 << 2)"""
    read = B16 + b"ACACACAC" + R20
    e, kept = keep(_brute(B16 + b"ACACAC" + R20).placements(read), 2, 3)
    assert (e, kept) == (2, [(0, 0, 0, INS, 2, 0, A)])
    assert event_of(kept[0], read) == (0, 15, INS, 2, 4)
    assert event_of((0, 1, 0, INS, 2, 0, A), _rc(read)) == (0, 15, INS, 2, 4)      # (the other strand's read: seq is in path strand)


def test_minimal_flank_on_each_side():
    """T = T B16 A C16 T with the A deleted.  B16 C16 T from x = 1: k* = 16 = A.  T B16 C16 from x = 0: k* = 17 = len - A.  Either: d = 0, pos 16.
    With a flank of 15 bases (B16[1:] C16 T from x = 2) the cut at 15 is not allowed: the placement is the one at k = 16 with the base
    before it as a substitution, d = 1.  A read of 31 bases has no allowed k at all."""
    t = b"T" + B16 + b"A" + C16 + b"T"
    b = _brute(t)
    left, right, short = B16 + C16 + b"T", b"T" + B16 + C16, B16[1:] + C16 + b"T"
    assert keep(b.placements(left), 2, 3) == (1, [(0, 0, 1, DEL, 1, 0, 16)]) and event_of((0, 0, 1, DEL, 1, 0, 16), left) == (0, 16, DEL, 1, 0)
    assert keep(b.placements(right), 2, 3) == (1, [(0, 0, 0, DEL, 1, 0, 17)]) and len(right) - A == 17
    assert keep(b.placements(short), 2, 3) == (2, [(0, 0, 2, DEL, 1, 1, 16)])
    assert b.placements(B16[1:] + C16) == []


def test_tie_of_a_del_and_an_ins():
    """path 0 = L20 GT R20, path 1 = L20 R20, the read L20 G R20: on path 0 the T is deleted (k* = 21: at k = 20 the G would be, with one
    mismatch), on path 1 the G is inserted (k* = 20).  Both e = 1, both kept: events (0, 20, DEL, 1, 0) and (1, 19, INS, 1, G = 2)"""
    read = L20 + b"G" + R20
    e, kept = keep(_brute(L20 + b"GT" + R20, L20 + R20).placements(read), 2, 3)
    assert e == 1 and sorted(kept) == [(0, 0, 0, DEL, 1, 0, 21), (1, 0, 0, INS, 1, 0, 20)]
    assert [event_of(x, read) for x in sorted(kept)] == [(0, 20, DEL, 1, 0), (1, 19, INS, 1, 2)]


def test_cost_at_and_above_the_threshold():
    """T = L20 CAT R20, the read lacks CAT.  With two substitutions (read bases 5 and 30): d = 2 = M, g = 3, e = M + g = 5: kept under
    M = 2, G = 3, nothing under G = 2 or M = 1.  With a third (base 12): d = 3 = M + 1: no placement under M = 2."""
    t = L20 + b"CAT" + R20
    sub = lambda s, at: bytes(b"ACGT"[(b"ACGT".index(c) + 1) % 4] if i in at else c for i, c in enumerate(s))
    two, three = sub(L20 + R20, (5, 30)), sub(L20 + R20, (5, 12, 30))
    b = _brute(t, m_max=3)
    assert keep(b.placements(two), 2, 3) == (5, [(0, 0, 0, DEL, 3, 2, 20)])
    assert keep(b.placements(two), 2, 2) == (None, []) and keep(b.placements(two), 1, 3) == (None, [])
    assert keep(b.placements(three), 3, 3) == (6, [(0, 0, 0, DEL, 3, 3, 20)])
    assert keep(b.placements(three), 2, 3) == (None, [])


def test_window_with_an_N_and_window_over_the_end():
    """the deleted base is an 'N': no placement (W holds it); W one base longer than the text: none either"""
    read = L20 + R20
    assert _brute(L20 + b"N" + R20).placements(read) == []
    assert keep(_brute(L20 + b"A" + R20).placements(read), 2, 3)[0] == 1
    assert _brute(L20 + b"A" + R20[:19]).placements(read) == []


P72 = b"TGGTGTTAACCTTACTATACTCCCGCTCCGGGGTTTGGCTCATATGAACAAGTCTTTGCGCCCATAAATGTA"
U100 = b"GCCAGTGAGCTTAGTTGGAGCAAGGGGTGCGGAAGCGCAACTCCGTCGCGCGGGTAGCCAACTACTTAAGACCTAGGATTCTGTTGCAGATTAGAACTTG"
W16 = b"ACGTCAGTGCATGACT"             # no base twice in a row, around the period's end neither: a one-base gap in it does not move


def test_read_that_fills_a_short_path_exactly():
    """a path of 72 bases.  An 80-base read with 8 inserted bases behind its first 40 has W = the whole path: x = 0, d = 0, e = 8, k* = 40 (the
    last inserted base G is not the T in front of the cut, so the gap does not move left), event (0, 39, INS, 8, GATTACAG).  A 64-base
    read that lacks bases 40 .. 47 fills it as well.  On the path's first 71 bases, or on its last 71, neither has a placement: every
    window of a read of 80 bases is at least 72 long, and the DEL read's only window with d <= 3 is the 72"""
    ins, dele = P72[:40] + b"GATTACAG" + P72[40:], P72[:40] + P72[48:]
    assert (len(P72), len(ins), len(dele)) == (72, 80, 64)
    b = _brute(P72, m_max=3)
    assert keep(b.placements(ins), 1, 8) == (8, [(0, 0, 0, INS, 8, 0, 40)]) and keep(b.placements(ins), 3, 7) == (None, [])
    assert event_of((0, 0, 0, INS, 8, 0, 40), ins) == (0, 39, INS, 8, 2 | 3 << 4 | 3 << 6 | 1 << 10 | 2 << 14)
    assert keep(b.placements(dele), 1, 8) == (8, [(0, 0, 0, DEL, 8, 0, 40)])
    for short in (P72[:71], P72[1:]):
        assert _brute(short, m_max=3).placements(ins) == [] and _brute(short, m_max=3).placements(dele) == []


def test_shifted_copies_in_a_repeat_longer_than_the_read():
    """T = L20 (W16 x 8) R20.  The read is T[24, 125) without base 74: 100 bases inside the repeat.  One period to the right the repeat
    spells the same 101 bases (40 + 101 <= 148), two periods to the right the window would run into R20, one to the left into L20: x = 24
    and x = 40 are kept, each d = 0, e = 1, k* = 50, events at pos 73 and 89"""
    t = L20 + W16 * 8 + R20
    read = t[24:74] + t[75:125]
    e, kept = keep(_brute(t, m_max=3).placements(read), 2, 3)
    assert e == 1 and sorted(kept) == [(0, 0, 24, DEL, 1, 0, 50), (0, 0, 40, DEL, 1, 0, 50)]
    assert [event_of(x, read) for x in sorted(kept)] == [(0, 73, DEL, 1, 0), (0, 89, DEL, 1, 0)]


def test_three_mismatches_and_one_clean_block():
    """M = 3: a read of 96 bases is six blocks.  TT inserted behind base 47 lies in blocks 2 and 3, substitutions at 5, 20 and 70 spoil
    blocks 0, 1 and 4: block 5 alone is clean.  d = 3, e = 3 + 2 under M = 3; nothing under M = 2, whatever G"""
    sub = lambda s, at: bytes(b"ACGT"[(b"ACGT".index(c) + 1) % 4] if i in at else c for i, c in enumerate(s))
    read = sub(U100[:47] + b"TT" + U100[47:94], (5, 20, 70))
    b = _brute(U100, m_max=3)
    assert len(read) == 96 and keep(b.placements(read), 3, 3) == (5, [(0, 0, 0, INS, 2, 3, 47)])
    assert keep(b.placements(read), 2, 8) == (None, []) and keep(b.placements(read), 3, 1) == (None, [])
    assert event_of((0, 0, 0, INS, 2, 3, 47), read) == (0, 46, INS, 2, 3 | 3 << 2)
    blocks = [read[16 * i:16 * i + 16] for i in range(6)]
    assert [blocks[i] == U100[16 * i:16 * i + 16] for i in range(3)] == [False] * 3            # in front of the gap
    assert [blocks[i] == U100[16 * i - 2:16 * i + 14] for i in range(3, 6)] == [False, False, True]      # behind it


# ---- the inputs of tests/test_gap_rescue.py ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return gap_case.case(tmp_path_factory)


def test_inputs_hold_every_class(case):
    index, batch, names, has, brute = case
    reads = _reads_of(batch)
    t = GapTables(index, 2, 3, brute)
    t.add(reads, has)
    cand = {i: (e, kept) for i, e, kept in t.per_read}
    print(t.stats, "reads", batch.n, "with a record", int(has.sum()), "events", len(t.events))
    assert batch.n <= 460 and len(cand) <= 420
    count = lambda f: sum(1 for i in range(batch.n) if f(i))
    rescued = lambda i: i in cand and cand[i][0] is not None
    floor = 10
    for cls in sorted(set(names) - {"clean", "cheaper gapped", "len79"}):      # every class is there as gap candidates
        assert count(lambda i: names[i] == cls and i in cand) >= floor, cls
    for g in (1, 2, 3):                                                        # up to G: rescued; G + 1 and more: not as such
        for typ in "DI":
            assert count(lambda i: names[i] == "%s%d" % (typ, g) and rescued(i) and cand[i][0] == g) >= floor, (typ, g)
    for cls in ("D4", "D8", "D9", "I8", "I9", "subs3", "over0", "overend", "N deleted", "N flank", "random"):
        assert count(lambda i: names[i] == cls and i in cand and not rescued(i)) >= floor, cls
    for cls in ("subs2", "k=A", "k=last", "edge16D", "edge16I", "edge32D", "edge32I", "edge64D", "edge64I", "straddle", "flush0", "flushend", "palindrome",
                "homopolymer", "tandem", "tie alleles", "tie types"):
        assert count(lambda i: names[i] == cls and rescued(i)) >= floor, cls
    assert count(lambda i: names[i] == "subs2" and rescued(i) and any(x[5] == 2 for x in cand[i][1])) >= floor            # d = M
    assert count(lambda i: names[i] == "k=A" and rescued(i) and any(x[6] == A for x in cand[i][1])) >= floor
    assert count(lambda i: names[i] == "k=last" and rescued(i) and any(x[6] == len(reads[i]) - (x[4] if x[3] == INS else 0) - A for x in cand[i][1])) >= floor
    assert count(lambda i: names[i] == "tie alleles" and rescued(i) and len({x[0] for x in cand[i][1]}) == 4) >= floor     # a0 .. a3
    assert count(lambda i: names[i] == "tie types" and rescued(i) and {x[3] for x in cand[i][1]} == {DEL, INS}) >= floor
    assert count(lambda i: names[i] in ("homopolymer", "tandem") and rescued(i)) >= 2 * floor
    assert count(lambda i: rescued(i) and any(x[1] == 0 for x in cand[i][1])) >= 100 and count(lambda i: rescued(i) and any(x[1] == 1 for x in cand[i][1])) >= 100      # both strands
    assert count(lambda i: names[i] == "clean" and has[i]) >= floor                                                        # reads with a record
    assert count(lambda i: names[i] == "cheaper gapped" and not has[i] and i not in cand and keep(brute.placements(reads[i]), 2, 3)[0] == 1) >= floor
    assert t.stats["too_short"] >= floor and count(lambda i: names[i] == "len79" and i not in cand) >= floor
    assert t.stats["del_placements"] >= 100 and t.stats["ins_placements"] >= 100
    t1 = GapTables(index, 1, 3, brute)                                                                                     # under M = 1 the "cheaper gapped" reads are not rescued ungapped
    t1.add(reads, has)
    c1 = {i for i, e, kept in t1.per_read if e == 1}
    assert count(lambda i: names[i] == "cheaper gapped" and i in c1) >= floor and t1.stats["too_short"] == 0
