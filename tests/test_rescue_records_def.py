"""The brute force of the rescued records (tests/rescue_records_def.py; the definition is in include/groot_hip.h, "rescued records") on
hand-worked cases with every record written out, and the floor of every class of record in the batch that tests/test_rescue_records.py
feeds the device (tests/rescue_records_case.py: the eight graphs and the batch of tests/test_rescue.py).  CPU only."""
import numpy as np
import pytest

from rescue_def import Tables, _rc
from rescue_records_case import the_case
from rescue_records_def import NONE as F, plain, records

FLOOR = 10


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return the_case(tmp_path_factory)


def _hand(case, texts, lens, reads, M):
    t = Tables(case.index, M)
    t.texts = texts + [None] * (len(t.texts) - len(texts))
    t.plen = np.array(lens + [0] * (len(t.plen) - len(lens)), dtype=np.int64)
    t.base = np.r_[0, np.cumsum(t.plen)]
    return plain(records(case.index, M, reads, np.zeros(len(reads), dtype=bool), t))


A40 = b"ACGTTGCAAGGCTTAACCGGATCAGGTTACAGTCATGCAA"


def test_strand_0_by_hand(case):
    """path 0 = the 40 bases, first Position 0; path 1 = the same with base 36 changed, first Position 3.  M = 1.
    read 0: bases 0 .. 31 with base 5 changed: distance 1 at x = 0 on both paths, X = 0 and 3.
    read 1: bases 8 .. 39 with its FIRST base changed: distance 1 on path 0 (on path 1 base 36 differs too: 2, not a placement).
    read 2: bases 8 .. 39 with its LAST base changed: likewise, and the record ends at the path's last base."""
    assert A40[5:6] == b"G" and A40[8:9] == b"A" and A40[39:40] == b"A" and A40[36:37] == b"G"
    texts = [(A40, 0), (A40[:36] + b"T" + A40[37:], 3)]
    reads = [A40[:5] + b"A" + A40[6:32], b"C" + A40[9:40], A40[8:39] + b"C"]
    assert _hand(case, texts, [40, 43], reads, 1) == [
        (0, 0, 0, 0, 1, (5, F, F)),
        (0, 1, 3, 0, 1, (5, F, F)),
        (1, 0, 8, 0, 1, (0, F, F)),
        (2, 0, 8, 0, 1, (31, F, F)),
    ]


def test_strand_1_by_hand(case):
    """the two paths 16 bases longer (M = 2 takes reads of 48 bases and more), path 1 again with base 36 changed and first Position 3.
    read 0: the reverse complement of bases 8 .. 55 with base 19 changed: strand 1, distance 1 on path 0 at offset 11 of the ORIENTED read;
            2 on path 1 -- within M, but above d*: not kept.
    read 1: the same with base 36 changed as well, to a base neither path has: distance 2 on both, offsets 11 and 28, X = 8 and 3 + 8."""
    b56 = A40 + b"TTGACCGTAAGCATCG"
    assert b56[19:20] == b"G" and b56[36:37] == b"G"
    texts = [(b56, 0), (b56[:36] + b"T" + b56[37:], 3)]
    reads = [_rc(b56[8:19] + b"C" + b56[20:56]), _rc(b56[8:19] + b"C" + b56[20:36] + b"A" + b56[37:56])]
    assert _hand(case, texts, [56, 59], reads, 2) == [
        (0, 0, 8, 1, 1, (11, F, F)),
        (1, 0, 8, 1, 2, (11, 28, F)),
        (1, 1, 11, 1, 2, (11, 28, F)),
    ]


def test_a_palindrome_on_both_strands_by_hand(case):
    """a 32-base reverse-complement palindrome P at offset 14 of path 0; the read is P with base 5 changed.  Strand 0: offset 5.  Strand 1:
    the oriented read is the reverse complement, the changed base lies at 31 - 5 = 26.  Two records of one read on one path at one pos,
    strand 0 first.  A second read that is P itself: d = 0 on both strands, no offsets.  M = 1."""
    half = b"ACGTTGCAAGGCTTAC"
    pal = half + _rc(half)
    assert _rc(pal) == pal and pal[5:6] == b"G"
    t0 = b"GGATCCTTAGGCAT" + pal + b"TTGACCGTAAGCAA"
    assert _hand(case, [(t0, 0)], [60], [pal[:5] + b"A" + pal[6:], pal], 1) == [
        (0, 0, 14, 0, 1, (5, F, F)),
        (0, 0, 14, 1, 1, (26, F, F)),
        (1, 0, 14, 0, 0, (F, F, F)),
        (1, 0, 14, 1, 0, (F, F, F)),
    ]


def test_a_palindromic_repeat_by_hand(case):
    """path 0 = U . (ACGT) x 16 . V, first Position 3: the repeat is its own reverse complement, so a read from it lies on both strands.  M = 1.
    read 0: (ACGT) x 12 with base 5 changed.  Strand 0: the repeat has room for it at s, s + 4 .. s + 16 (s = 3 + 20), offset 5.  Strand 1:
            the oriented read is (ACGT) x 12 with base 47 - 5 changed, at the same five pos.  ALL of strand 0 comes before strand 1: in
            (path, pos, strand) order the ten records would alternate.
    read 1: (CGTA) x 12 with its first base changed.  Strand 0 at s + 1, s + 5, s + 9, s + 13; its reverse complement is (TACG) x 12 with its
            LAST base changed, at s + 3 .. s + 15: the strands interleave in pos, and the list does not."""
    u, v = b"GGATCCTTAGGCATTGACCG", b"TTGACCGTAAGC"
    text = u + b"ACGT" * 16 + v
    w0, w1 = b"ACGT" * 12, b"CGTA" * 12
    assert len(text) == 96 and w0[5:6] == b"C" and _rc(b"ACGT" * 16) == b"ACGT" * 16 and _rc(w1) == b"TACG" * 12
    reads = [w0[:5] + b"A" + w0[6:], b"T" + w1[1:]]
    assert _rc(reads[0]) == w0[:42] + b"T" + w0[43:] and _rc(reads[1]) == _rc(w1)[:47] + b"A"
    assert _hand(case, [(text, 3)], [99], reads, 1) == [
        (0, 0, 23, 0, 1, (5, F, F)),
        (0, 0, 27, 0, 1, (5, F, F)),
        (0, 0, 31, 0, 1, (5, F, F)),
        (0, 0, 35, 0, 1, (5, F, F)),
        (0, 0, 39, 0, 1, (5, F, F)),
        (0, 0, 23, 1, 1, (42, F, F)),
        (0, 0, 27, 1, 1, (42, F, F)),
        (0, 0, 31, 1, 1, (42, F, F)),
        (0, 0, 35, 1, 1, (42, F, F)),
        (0, 0, 39, 1, 1, (42, F, F)),
        (1, 0, 24, 0, 1, (0, F, F)),
        (1, 0, 28, 0, 1, (0, F, F)),
        (1, 0, 32, 0, 1, (0, F, F)),
        (1, 0, 36, 0, 1, (0, F, F)),
        (1, 0, 26, 1, 1, (47, F, F)),
        (1, 0, 30, 1, 1, (47, F, F)),
        (1, 0, 34, 1, 1, (47, F, F)),
        (1, 0, 38, 1, 1, (47, F, F)),
    ]


def test_records_hold_every_class(case):
    """every class of record the device test relies on occurs at least FLOOR times in the batch"""
    rec = case.records(2)
    L = np.array([len(r) for r in case.reads], dtype=np.int64)[rec["read"]]
    mm = rec["mm"].astype(np.int64)
    print("records", len(rec), "reads", len(np.unique(rec["read"])))
    assert np.array_equal(rec, np.sort(rec, order=["read", "path", "strand", "pos"]))
    # this batch cannot tell that order from (read, path, pos, strand): where one read has both strands on one path -- the palindrome of
    # graph 7 -- they lie at the same pos.  tests/test_rescue_records_shapes.py has the reads that can, and the floor for them
    other = np.sort(rec, order=["read", "path", "pos", "strand"])
    print("reads whose records differ under (read, path, pos, strand) order", len(np.unique(rec["read"][rec != other])))
    for d in (0, 1, 2):
        assert int((rec["d"] == d).sum()) >= FLOOR, d
    assert int((case.records(3)["d"] == 3).sum()) >= FLOOR
    for at in (0, 31, 32, 63, 64):
        assert int((mm == at).any(axis=1).sum()) >= FLOOR, at
    assert int((mm == (L - 1)[:, None]).any(axis=1).sum()) >= FLOOR
    per_read = np.unique(rec["read"], return_counts=True)[1]
    assert int((per_read > 64).sum()) >= FLOOR, per_read.max()
    print("most records of one read", int(per_read.max()), "mean", float(per_read.mean()))
    on_path = np.unique(np.stack([rec["read"], rec["path"]], axis=1), axis=0, return_counts=True)[1]
    assert int((on_path >= 2).sum()) >= FLOOR
    plen = case.index.arrays["path_len"].astype(np.int64)
    first = np.array([t[1] for t in case.texts], dtype=np.int64)
    end = np.array([t[1] + min(len(t[0]), int(plen[p]) - t[1]) for p, t in enumerate(case.texts)], dtype=np.int64)
    assert int((rec["pos"] == first[rec["path"]]).sum()) >= FLOOR
    assert int((rec["pos"] + L == end[rec["path"]]).sum()) >= FLOOR
    # M = 1 and M = 3 give other lists: a read rescued at d = 2 has no record under M = 1, one below 64 bases has none under M = 3
    n = {M: len(case.records(M)) for M in (1, 2, 3)}
    assert len(set(n.values())) == 3, n
