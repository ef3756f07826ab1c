"""groot_bam_write_rescued_gapped (include/groot_host.h, "Gapped records") against a plain-Python restatement of the writer: on the
hand-made records of tools/rescued_gapped_bam_check.c, which runs the writer as a stand-alone program under AddressSanitizer + UBSan, and
through the library on random records over the index of tests/rescue_records_case.py.

The writer, restated: the two lists of a batch merged by read; a rescued record as tests/test_rescued_bam.py restates it; a gapped record
with CIGAR <k>M<g>D<len-k>M or <k>M<g>I<len-k-g>M, bin over the reference span (len + g, len - g), NM = d + g as a uint8, and MD over the
aligned bases: runs, the path's base at every mismatch, ^ and the deleted path bases between the flanks of a deletion (a run of 0 in
front of them after a mismatch, and behind them before one), nothing at an insertion: the run goes on across it."""
import os
import struct
import subprocess

import numpy as np
import pytest

from bamread import read_bam
from groot_amd import device, host
from rescue_records_case import the_case
from test_rescued_bam import _COMP, _NT16, _random_records, _reg2bin, aux_of, record_py, split_bam

F = 0xFFFF
DEL, INS = 0, 1


def md_py(L, path, pos, k, d, typ, g, mm, ref_base):
    """MD of a gapped record, from the aligned pairs (read offset, path coordinate) one by one"""
    pairs = [(i, pos + i) for i in range(k)]
    pairs += [(i, pos + g + i) for i in range(k, L)] if typ == DEL else [(i, pos + i - g) for i in range(k + g, L)]
    out, run = b"", 0
    for i, y in pairs:
        if typ == DEL and i == k:
            out += b"%d^" % run + bytes(ref_base(path, pos + k + q) for q in range(g))
            run = 0
        if i in mm[:d]:
            out += b"%d%c" % (run, ref_base(path, y))
            run = 0
        else:
            run += 1
    return out + b"%d" % run


def gapped_py(name, seq, qual, rec, secondary, ref_base):
    """the bytes of one gapped record; rec = (path, pos, k, strand, d, type, g, mm)"""
    path, pos, k, strand, d, typ, g, mm = rec
    n = len(seq)
    qual = (qual + b"!" * n)[:n]
    if strand:
        seq, qual = seq.translate(_COMP)[::-1], qual[::-1]
    cigar = [(k, 0), (g, 2), (n - k, 0)] if typ == DEL else [(k, 0), (g, 1), (n - k - g, 0)]
    span = n + g if typ == DEL else n - g
    flag = (0x10 if strand else 0) | (0x100 if secondary else 0)
    packed = bytes((_NT16[seq[j]] << 4) | (_NT16[seq[j + 1]] if j + 1 < n else 0) for j in range(0, n, 2))
    body = struct.pack("<iiBBHHHiiii", path, pos, len(name) + 1, 30, _reg2bin(pos, pos + span), 3, flag, n, -1, -1, 0)
    body += name + b"\0" + b"".join(struct.pack("<I", c << 4 | op) for c, op in cigar) + packed + qual
    body += b"NMC" + bytes([d + g]) + b"MDZ" + md_py(n, path, pos, k, d, typ, g, list(mm), ref_base) + b"\0"
    return struct.pack("<i", len(body)) + body


def merged_py(names, seqs, quals, recs, grecs, ref_base):
    """recs: [(read, path, pos, strand, d, mm)], grecs: [(read, path, pos, k, strand, d, type, g, mm)], both ascending by read"""
    tagged = sorted([(r[0], 0, i) for i, r in enumerate(recs)] + [(r[0], 1, i) for i, r in enumerate(grecs)])
    out, prev = b"", None
    for read, kind, i in tagged:
        r = (grecs if kind else recs)[i]
        out += (gapped_py if kind else record_py)(names[read], seqs[read], quals[read], r[1:], read == prev, ref_base)
        prev = read
    return out


# the tables of tools/rescued_gapped_bam_check.c
_PATHS = [(b"alpha", b"TGGTGTTAACCTTACTATACTCCCGCTCCGGGGTTTGGCTCATATGAACAAGTCTTTGCGCCCATAAATGTAGCCAGTGA"), (b"beta", b"GCTTAGTTGGAGCAAGGGGTGCGGAAGCGCAACTCCGTCGCGCGGGTA")]
_NAMES = [b"d0", b"ins/1", b"u", b"two", b"last"]
_SEQS = [b"ACGT" * 10, b"C" * 20 + b"A" + b"G" * 20, b"CATGAATG", b"T" * 16 + b"A" * 8 + b"C" * 16, b"GATTACA" * 5]
_QUALS = [b"I" * 10 + b"H" * 10 + b"G" * 10 + b"F" * 10, b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmno", b"JJJ", b"!!##%%", b"01234567890123456789012345678901234"]
_PLAIN = [(2, 1, 40, 0, 1, (4, F, F))]
_GOOD = [(0, 0, 2, 16, 0, 1, DEL, 3, (16, F, F)), (0, 0, 5, 24, 1, 1, DEL, 8, (15, F, F)), (1, 0, 10, 20, 0, 0, INS, 1, (F, F, F)), (1, 1, 0, 16, 1, 3, INS, 8, (0, 15, 40)),
         (3, 0, 37, 24, 0, 2, DEL, 3, (24, 25, F)), (3, 1, 2, 16, 1, 1, INS, 8, (24, F, F)), (4, 1, 3, 19, 0, 0, DEL, 1, (F, F, F))]
_CALLS = [(_PLAIN, _GOOD[:4]), ([], _GOOD[4:])]
_REF = lambda p, y: _PATHS[p][1][y]


def test_restatement_by_hand():
    """the MD strings of the issue's two examples, and of the program's records, written out"""
    t = b"A" * 31 + b"ACG" + b"T" + b"A" * 67                      # 31 matches, ACG deleted, a mismatch on the T, 67 matches
    assert md_py(99, 0, 0, 31, 1, DEL, 3, [31], lambda p, y: t[y]) == b"31^ACG0T67"
    assert md_py(100, 0, 0, 50, 0, INS, 1, [], lambda p, y: 65) == b"99"     # 50M1I49M without a mismatch
    got = b"".join(merged_py(_NAMES, _SEQS, _QUALS, r, g, _REF) for r, g in _CALLS)
    aux = aux_of(got)
    assert aux == [("d0", 0, 2, 0, {"NM": 4, "MD": "16^ACT0C23"}), ("d0", 0, 5, 0x110, {"NM": 9, "MD": "15T8^GGGGTTTG16"}),
                   ("ins/1", 0, 10, 0, {"NM": 1, "MD": "40"}), ("ins/1", 1, 0, 0x110, {"NM": 11, "MD": "0G14G16C0"}),
                   ("u", 1, 40, 0, {"NM": 1, "MD": "4G3"}),
                   ("two", 0, 37, 0, {"NM": 5, "MD": "24^CCA0T0A14"}), ("two", 1, 2, 0x110, {"NM": 9, "MD": "16G15"}), ("last", 1, 3, 0, {"NM": 1, "MD": "19^G16"})], aux


def _check_fields(path, names, seqs, merged):
    """CIGAR, bin, NM, MD's total and the flags of every record of the file, from the records' fields alone; merged: [(kind, record)]"""
    import re
    _, _, recs = read_bam(path)
    aux = aux_of(split_bam(path)[2])
    assert len(recs) == len(aux) == len(merged)
    prev = None
    for b, a, (kind, r) in zip(recs, aux, merged):
        L = len(seqs[r[0]])
        if kind:
            read, p, pos, k, strand, d, typ, g, mm = r
            cigar, span, nm = ("%dM%dD%dM" % (k, g, L - k), L + g, d + g) if typ == DEL else ("%dM%dI%dM" % (k, g, L - k - g), L - g, d + g)
        else:
            read, p, pos, strand, d, mm = r
            cigar, span, nm = "%dM" % L, L, d
        assert b["name"] == names[read].decode() and (b["ref_id"], b["pos"], b["mapq"], b["cigar"]) == (p, pos, 30, cigar), (b, r)
        assert b["bin"] == _reg2bin(pos, pos + span) and b["flag"] == (0x10 if strand else 0) | (0x100 if read == prev else 0), (b, r)
        assert a[4]["NM"] == nm
        md = a[4]["MD"]
        # MD covers the reference span: runs + one per mismatch base + the deleted bases
        n_del = sum(len(x) for x in re.findall(r"\^([ACGTN]+)", md))
        rest = re.sub(r"\^[ACGTN]+", "|", md)
        assert sum(int(x) for x in re.findall(r"\d+", rest)) + len(re.findall(r"[ACGTN]", rest)) + n_del == span, (md, r)
        assert len(re.findall(r"[ACGTN]", rest)) == d and n_del == (g if kind and typ == DEL else 0), (md, r)
        prev = read


def test_stand_alone_program_under_sanitizers(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(repo, "include")]
    obj, exe, bam = str(tmp_path / "check.o"), str(tmp_path / "rescued_gapped_bam_check"), str(tmp_path / "gapped.bam")
    subprocess.run(["gcc", "-std=c11"] + san + ["-c", os.path.join(repo, "tools", "rescued_gapped_bam_check.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17"] + san + ["-o", exe, obj, os.path.join(repo, "tools", "rescued_bam_check_stubs.cpp"),
                                                 os.path.join(repo, "groot_amd", "csrc", "host", "bam.cpp"), "-lpthread", "-lz"], check=True)
    r = subprocess.run([exe, bam], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"ok\n", (r.stdout, r.stderr[-2000:])
    text, refs, records = split_bam(bam)
    assert refs == [(n, len(s)) for n, s in _PATHS]
    want = b"".join(merged_py(_NAMES, _SEQS, _QUALS, rr, g, _REF) for rr, g in _CALLS)
    assert records == want, (aux_of(records), aux_of(want))
    order = [(1, _GOOD[0]), (1, _GOOD[1]), (1, _GOOD[2]), (1, _GOOD[3]), (0, _PLAIN[0]), (1, _GOOD[4]), (1, _GOOD[5]), (1, _GOOD[6])]
    _check_fields(bam, _NAMES, _SEQS, order)
    assert [b["cigar"] for b in read_bam(bam)[2]] == ["16M3D24M", "24M8D16M", "20M1I20M", "16M8I17M", "8M", "24M3D16M", "16M8I16M", "19M1D16M"]


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return the_case(tmp_path_factory)


def _random_gapped(case, rng, n_reads, per_read):
    """reads of 40 .. 150 bases; the even ones get rescued records (test_rescued_bam's), the odd ones gapped records: any path, any pos up
    to the path's last base, both strands and types, g = 1 .. 8, k from 16 to its largest, d = 0 .. 3 with offsets at either end and on
    either side of the gap"""
    plen = case.index.arrays["path_len"].astype(np.int64)
    names, seqs, quals, recs = _random_records(case, rng, n_reads, per_read)
    recs = [r for r in recs if not r[0] & 1]
    grecs = []
    for r in range(1, n_reads, 2):
        L = len(seqs[r])
        if L < 40:
            continue
        for _ in range(int(rng.integers(0, per_read + 1))):
            typ, g = int(rng.integers(2)), int(rng.integers(1, 9))
            aligned, span = (L, L + g) if typ == DEL else (L - g, L - g)
            k = int(rng.choice([16, aligned - 16, int(rng.integers(16, aligned - 15))]))
            ok = [i for i in range(L) if typ == DEL or not k <= i < k + g]
            d = int(rng.integers(0, 4))
            mm = sorted(rng.choice(ok, d, replace=False).tolist())
            if d and rng.integers(2) == 0:
                mm = sorted(set(mm[1:-1] + [int(rng.choice([0, k - 1])), int(rng.choice([k + (g if typ == INS else 0), L - 1]))]))
                d = len(mm)
            p = int(rng.choice(np.flatnonzero(plen >= span)))
            pos = int(rng.integers(0, plen[p] - span + 1)) if rng.integers(4) else int(plen[p]) - span
            grecs.append((r, p, pos, k, int(rng.integers(2)), d, typ, g, tuple(mm + [F] * (3 - d))))
    return names, seqs, quals, recs, grecs


def _arrays(recs, grecs):
    a = np.zeros(len(recs), dtype=device.RESCUE_RECORD_DTYPE)
    for i, (r, p, pos, strand, d, mm) in enumerate(recs):
        a[i] = (r, p, pos, mm, strand, d)
    b = np.zeros(len(grecs), dtype=device.GAP_RECORD_DTYPE)
    for i, (r, p, pos, k, strand, d, typ, g, mm) in enumerate(grecs):
        b[i] = (r, p, pos, k, mm, strand, d, typ, g)
    return a, b


def _ref_base(case):
    def ref_base(p, y):
        t, first = case.texts[p]
        return t[y - first] if first <= y < first + len(t) else ord("N")
    return ref_base


def test_library_on_random_records(case, tmp_path):
    """the library's writer on a few hundred random records of both kinds over the eight graphs, in two calls: byte for byte the
    restatement after inflation, and CIGAR, bin, NM, MD and the flags per record from the fields alone"""
    rng = np.random.default_rng(29)
    out = str(tmp_path / "gapped.bam")
    w = host.BamWriter(out, case.index, date="2020-01-01T00:00:00Z")
    want, merged, all_names, all_seqs = b"", [], [], []
    for call in range(2):
        names, seqs, quals, recs, grecs = _random_gapped(case, rng, 80, 4)
        a, b = _arrays(recs, grecs)
        assert host.bam_write_rescued_gapped(w, a, b, names, seqs, quals) == len(recs) + len(grecs) and len(recs) > 40 and len(grecs) > 40
        want += merged_py(names, seqs, quals, recs, grecs, _ref_base(case))
        base = len(all_names)
        tagged = sorted([(r[0], 0, i) for i, r in enumerate(recs)] + [(r[0], 1, i) for i, r in enumerate(grecs)])
        merged += [(kind, ((grecs if kind else recs)[i][0] + base,) + (grecs if kind else recs)[i][1:]) for _, kind, i in tagged]
        all_names += names
        all_seqs += seqs
    w.close()
    assert split_bam(out)[2] == want
    _check_fields(out, all_names, all_seqs, merged)
    aux = aux_of(want)
    assert any("^" in a[4]["MD"] and "0^" in a[4]["MD"] for a in aux) and any(__import__("re").search(r"\^[ACGTN]+0[ACGTN]", a[4]["MD"]) for a in aux)
    assert {b["cigar"][-1] for b in read_bam(out)[2]} == {"M"} and any("I" in b["cigar"] for b in read_bam(out)[2]) and any("D" in b["cigar"] for b in read_bam(out)[2])


def test_no_gapped_record_is_the_rescued_writer(case, tmp_path):
    """ng = 0: the bytes of groot_bam_write_rescued, file for file"""
    files = []
    for gapped in (False, True):
        rng = np.random.default_rng(23)
        out = str(tmp_path / ("g%d.bam" % gapped))
        w = host.BamWriter(out, case.index, date="2020-01-01T00:00:00Z")
        for call in range(2):
            names, seqs, quals, recs = _random_records(case, rng, 60, 4)
            a, b = _arrays(recs, [])
            n = host.bam_write_rescued_gapped(w, a, b, names, seqs, quals) if gapped else w.write_rescued(a, names, seqs, quals)
            assert n == len(recs) > 60
        w.close()
        files.append(open(out, "rb").read())
    assert files[0] == files[1] and len(files[0]) > 1000


def test_library_refuses_what_the_program_refuses(case, tmp_path):
    w = host.BamWriter(str(tmp_path / "x.bam"), case.index, date="2020-01-01T00:00:00Z")
    L = 40
    plen = case.index.arrays["path_len"].astype(np.int64)
    names, seqs, quals = [b"a", b"b"], [b"A" * L, b"C" * 8], [b"I" * L, b"I" * 8]
    N3 = (F, F, F)
    good = (0, 0, 2, 16, N3, 0, 0, DEL, 3)
    none = np.zeros(0, dtype=device.RESCUE_RECORD_DTYPE)
    for bad in [(2, 0, 2, 16, N3, 0, 0, DEL, 3), (0, len(plen), 2, 16, N3, 0, 0, DEL, 3), (0, 0, int(plen[0]) - L - 3 + 1, 16, N3, 0, 0, DEL, 3),
                (0, 0, int(plen[0]) - L + 1 + 1, 16, N3, 0, 0, INS, 1), (0, 0, 2, 16, N3, 2, 0, DEL, 3), (0, 0, 2, 16, (1, 2, 3), 0, 4, DEL, 3),
                (0, 0, 2, 16, N3, 0, 0, 2, 3), (0, 0, 2, 16, N3, 0, 0, DEL, 0), (0, 0, 2, 16, N3, 0, 0, DEL, 9), (0, 0, 2, 15, N3, 0, 0, DEL, 3),
                (0, 0, 2, 25, N3, 0, 0, DEL, 3), (0, 0, 2, 17, N3, 0, 0, INS, 8), (1, 0, 2, 4, N3, 0, 0, INS, 8), (0, 0, 2, 16, (L, F, F), 0, 1, DEL, 3),
                (0, 0, 2, 16, N3, 0, 1, DEL, 3), (0, 0, 2, 16, (3, 3, F), 0, 2, DEL, 3), (0, 0, 2, 16, (1, F, 2), 0, 1, DEL, 3),
                (0, 0, 2, 16, (16, F, F), 0, 1, INS, 3), (0, 0, 2, 16, (18, F, F), 0, 1, INS, 3)]:
        arr = np.zeros(2, dtype=device.GAP_RECORD_DTYPE)
        arr[0], arr[1] = good, bad
        with pytest.raises(host.GrootError) as e:
            host.bam_write_rescued_gapped(w, none, arr, names, seqs, quals)
        assert e.value.code == -1, bad
    arr = np.zeros(1, dtype=device.GAP_RECORD_DTYPE)
    arr[0] = good
    both = np.zeros(1, dtype=device.RESCUE_RECORD_DTYPE)
    both[0] = (0, 0, 0, N3, 0, 0)
    with pytest.raises(host.GrootError) as e:                    # a read in both lists
        host.bam_write_rescued_gapped(w, both, arr, names, seqs, quals)
    assert e.value.code == -1 and "rescued records and gapped records" in str(e.value), e.value
    both[0] = (0, 0, int(plen[0]), N3, 0, 0)                     # what the rescued writer refuses
    with pytest.raises(host.GrootError) as e:
        host.bam_write_rescued_gapped(w, both, np.zeros(0, dtype=device.GAP_RECORD_DTYPE), names, seqs, quals)
    assert e.value.code == -1
    with pytest.raises(host.GrootError) as e:
        host.bam_write_rescued_gapped(w, none, arr, [b"n" * 255, b"b"], seqs, quals)
    assert e.value.code == -3
    w.close()
    assert split_bam(str(tmp_path / "x.bam"))[2] == b""
