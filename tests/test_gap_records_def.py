"""The brute force of the gapped records (tests/gap_records_def.py; include/groot_hip.h, "gapped records") on four hand-worked cases with
every field written out, and the floor of every class of record on the case of tests/test_gap_records.py (tests/gap_records_case.py):
checked against the brute force alone, so that the device tests cannot pass by leaving a class out.  CPU only."""
import numpy as np
import pytest

from gap_def import DEL, INS, Brute, keep
from gap_records_case import CLASSES, the_case
from gap_records_def import NONE, RECORD_DTYPE, rows_of
from rescue_def import _rc

#      0         10        20        30        40        50        60        70        80        90        100       110       120       130
T0 = b"TGGTGTTAACCTTACTATACTCCCGCTCCGGGGTTTGGCTCATATGAACAAGTCTTTGCGCCCATAAATGTAGCCAGTGAGCTTAGTTGGAGCAAGGGGTGCGGAAGCGCAACTCCGTCGCGCGGGTAGCCAACTACTTA"
T1 = T0[:120] + b"G" + T0[121:]           # a second path: the same but for base 120 (C -> G)
N3 = (NONE, NONE, NONE)


def _rows(read, texts, M=2, G=3):
    """(e*, [(path, strand, pos, type, g, d, k, mm)]) of one read"""
    b = Brute(None, 3, texts=[(t, 0) for t in texts])
    e, kept = keep(b.placements(read), M, G)
    return e, rows_of(b, read, kept)


def test_a_deletion_with_a_mismatch_right_behind_it():
    """31 bases of T0 from 10, T0[41:44] = ATA left out, then T0[44:112] with its first base T -> G: G differs from the T it lies on and
    from the A a cut one base later would put it on, so k* stays 31 and the mismatch is the first aligned base behind the gap"""
    assert T0[41:44] == b"ATA" and T0[44:45] == b"T" and T0[40:41] != T0[43:44]
    read = T0[10:41] + b"G" + T0[45:112]
    assert len(read) == 99
    assert _rows(read, [T0]) == (4, [(0, 0, 10, DEL, 3, 1, 31, (31, NONE, NONE))])


def test_an_insertion_with_the_matching_run_across_it():
    """50 bases of T0 from 5, a C that is not there, 49 bases more: no mismatch, the aligned bases are T0[5:104]"""
    assert T0[54:55] == b"T" and T0[55:56] == b"T"
    read = T0[5:55] + b"C" + T0[55:104]
    assert len(read) == 100
    assert _rows(read, [T0]) == (1, [(0, 0, 5, INS, 1, 0, 50, N3)])
    # ... and left-aligned: an inserted T behind T0[54] = T is an inserted T in front of it
    assert _rows(T0[5:55] + b"T" + T0[55:104], [T0]) == (1, [(0, 0, 5, INS, 1, 0, 49, N3)])


def test_the_reverse_strand():
    """the oriented read: 40 bases of T0 from 20, two left out, 50 more, base 5 substituted; the read is its reverse complement.  pos, k and
    mm are the oriented read's"""
    oriented = T0[20:25] + {b"T": b"A", b"C": b"G", b"G": b"T", b"A": b"C"}[T0[25:26]] + T0[26:60] + T0[62:112]
    assert len(oriented) == 90 and T0[59:60] != T0[61:62]
    assert _rows(_rc(oriented), [T0]) == (3, [(0, 1, 20, DEL, 2, 1, 40, (5, NONE, NONE))])


def test_a_read_tied_over_two_paths():
    """T1 is T0 but for base 120, behind the window: one record per path, in path order; with M = 0 substitutions nothing changes"""
    read = T0[12:42] + b"GT" + T0[42:110]
    assert len(read) == 100
    want = [(0, 0, 12, INS, 2, 0, 30, N3), (1, 0, 12, INS, 2, 0, 30, N3)]
    assert _rows(read, [T0, T1]) == (2, want)
    assert _rows(read, [T0, T1], G=1) == (None, [])                  # G below the gap: not gap-rescued
    # a window that reaches base 120 tells the paths apart: T0 at e = 2, T1 at e = 3 is not kept
    read = T0[30:60] + b"GT" + T0[60:128]
    assert _rows(read, [T0, T1]) == (2, [(0, 0, 30, INS, 2, 0, 30, N3)])


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return the_case(tmp_path_factory)


def test_the_case_holds_every_class(case):
    """ten records at least of every class under (M, G) = (2, 8), over the parts of the case; the list is sorted and every record is
    well-formed"""
    n = dict.fromkeys(CLASSES, 0)
    for part in case.values():
        rec = part.records(2, 8)
        assert rec.dtype == RECORD_DTYPE and len(rec)
        assert np.array_equal(rec, np.sort(rec, order=["read", "path", "strand", "pos", "type", "g"]))
        L = np.array([len(r) for r in part.reads])[rec["read"]]
        assert (rec["k"] >= 16).all() and (rec["k"] + 16 <= L - np.where(rec["type"] == INS, rec["g"], 0)).all() and (rec["d"] <= 2).all()
        for name in CLASSES:
            n[name] += len(part.in_class(name))
    print(n)
    assert all(v >= 10 for v in n.values()), n
    # the parts' own: reads up to 512 bases in "shapes", both strands of the palindromes in "pal"
    assert len(case["shapes"].in_class("offset above 255")) >= 10 and len(case["pal"].in_class("both strands")) >= 10
    assert len(case["pal"].in_class("two x on one path")) >= 10 and len(case["classes"].in_class("two paths")) >= 10
