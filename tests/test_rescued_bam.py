"""groot_bam_write_rescued (include/groot_host.h, "Rescued records") against a plain-Python restatement of the writer: on the hand-made
records of tools/rescued_bam_check.c, which runs the writer as a stand-alone program under AddressSanitizer + UBSan, and through the
library on random records over the index of tests/rescue_records_case.py.

The writer, restated: one BAM record per rescued record, in list order -- QNAME the read's name; FLAG 0x10 for strand 1, 0x100 on every
record of a read but its first in the list; MAPQ 30; CIGAR <len>M; SEQ / QUAL reverse-complemented / reversed for strand 1 (a short
quality line padded with '!'); no mate; NM as a uint8; MD the run of matches, then per mismatch the path's base and the next run."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from groot_amd import device, host
from rescue_records_case import the_case

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_NT16 = {c: i for i, c in enumerate(b"=ACMGRSVTWYHKDBN")}


def _reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def record_py(name, seq, qual, rec, secondary, ref_base):
    """the bytes of one record; rec = (path, pos, strand, d, mm), ref_base(path, y) the path's base at coordinate y"""
    path, pos, strand, d, mm = rec
    n = len(seq)
    qual = (qual + b"!" * n)[:n]
    if strand:
        seq, qual = seq.translate(_COMP)[::-1], qual[::-1]
    md, at = b"", 0
    for k in range(d):
        md += b"%d%c" % (mm[k] - at, ref_base(path, pos + mm[k]))
        at = mm[k] + 1
    md += b"%d" % (n - at)
    flag = (0x10 if strand else 0) | (0x100 if secondary else 0)
    packed = bytes((_NT16[seq[j]] << 4) | (_NT16[seq[j + 1]] if j + 1 < n else 0) for j in range(0, n, 2))
    body = struct.pack("<iiBBHHHiiii", path, pos, len(name) + 1, 30, _reg2bin(pos, pos + n), 1, flag, n, -1, -1, 0)
    body += name + b"\0" + struct.pack("<I", n << 4) + packed + qual + b"NMC" + bytes([d]) + b"MDZ" + md + b"\0"
    return struct.pack("<i", len(body)) + body


def records_py(names, seqs, quals, recs, ref_base):
    """... of a list of (read, path, pos, strand, d, mm) in list order"""
    out, prev = b"", None
    for r in recs:
        out += record_py(names[r[0]], seqs[r[0]], quals[r[0]], r[1:], r[0] == prev, ref_base)
        prev = r[0]
    return out


def split_bam(path):
    """(header text, [(name, length)], the bytes of all records) of a BAM file"""
    data = gzip.open(path, "rb").read()
    assert data[:4] == b"BAM\x01"
    (l_text,) = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", data, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", data, p)
        refs.append((data[p + 4:p + 4 + l_name - 1], struct.unpack_from("<i", data, p + 4 + l_name)[0]))
        p += 8 + l_name
    return data[8:8 + l_text], refs, data[p:]


def aux_of(records):
    """per record of the bytes: (name, ref_id, pos, flag, {tag: value}) with the aux fields 'C' and 'Z' this writer uses"""
    out, p = [], 0
    while p < len(records):
        (bs,) = struct.unpack_from("<i", records, p)
        ref_id, pos, l_rn, mapq, bin_, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", records, p + 4)
        q = p + 36 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        tags = {}
        while q < p + 4 + bs:
            tag, ty = records[q:q + 2].decode(), records[q + 2:q + 3]
            if ty == b"C":
                tags[tag], q = records[q + 3], q + 4
            else:
                assert ty == b"Z"
                e = records.index(b"\0", q + 3)
                tags[tag], q = records[q + 3:e].decode(), e + 1
        assert q == p + 4 + bs
        out.append((records[p + 36:p + 36 + l_rn - 1].decode(), ref_id, pos, flag, tags))
        p += 4 + bs
    return out


# the tables of tools/rescued_bam_check.c
_PATHS = [(b"*alpha", b"ACGTACGTTGCAGGATCC"), (b"beta", b"ACGTACGTTGCATTTAAA"), (b"gamma", b"CATGCATG")]
_NAMES, _SEQS, _QUALS = [b"r0", b"read/1", b"q", b"r3"], [b"ACGTACGTTG", b"CGATACTT", b"CATGAATG", b"ACTGTG"], [b"IIIIIHHHHH", b"ABCDEFGH", b"JJJ", b"!!##%%"]
F = 0xFFFF
_CALLS = [[(0, 0, 0, 0, 0, (F, F, F)), (0, 1, 0, 0, 0, (F, F, F)), (1, 0, 10, 1, 3, (0, 3, 7))],
          [(2, 2, 0, 0, 1, (4, F, F)), (3, 1, 4, 0, 2, (2, 3, F)), (3, 1, 4, 1, 2, (2, 3, F))]]


def test_restatement_by_hand():
    ref = lambda p, y: _PATHS[p][1][y]
    got = aux_of(b"".join(records_py(_NAMES, _SEQS, _QUALS, c, ref) for c in _CALLS))
    assert got == [("r0", 0, 0, 0, {"NM": 0, "MD": "10"}), ("r0", 1, 0, 0x100, {"NM": 0, "MD": "10"}),
                   ("read/1", 0, 10, 0x10, {"NM": 3, "MD": "0C2G3C0"}),
                   ("q", 2, 0, 0, {"NM": 1, "MD": "4C3"}), ("r3", 1, 4, 0, {"NM": 2, "MD": "2G0T2"}), ("r3", 1, 4, 0x110, {"NM": 2, "MD": "2G0T2"})]
    one = record_py(b"read/1", b"CGATACTT", b"ABCDEFGH", (0, 10, 1, 3, (0, 3, 7)), False, ref)
    assert one[36 + 7 + 4:36 + 7 + 4 + 4 + 8] == bytes([0x11, 0x48, 0x18, 0x24]) + b"HGFEDCBA"      # AAGTATCG, the quality line reversed
    short = record_py(b"q", b"CATGAATG", b"JJJ", (2, 0, 0, 1, (4, F, F)), False, ref)
    assert short[36 + 2 + 4 + 4:36 + 2 + 4 + 4 + 8] == b"JJJ!!!!!"


def test_stand_alone_program_under_sanitizers(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(repo, "include")]
    obj, exe, bam = str(tmp_path / "check.o"), str(tmp_path / "rescued_bam_check"), str(tmp_path / "rescued.bam")
    subprocess.run(["gcc", "-std=c11"] + san + ["-c", os.path.join(repo, "tools", "rescued_bam_check.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17"] + san + ["-o", exe, obj, os.path.join(repo, "tools", "rescued_bam_check_stubs.cpp"),
                                                 os.path.join(repo, "groot_amd", "csrc", "host", "bam.cpp"), "-lpthread", "-lz"], check=True)
    r = subprocess.run([exe, bam], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == b"ok\n", (r.stdout, r.stderr[-2000:])
    text, refs, records = split_bam(bam)
    assert refs == [(n, len(s)) for n, s in _PATHS] and text.startswith(b"@HD\tVN:1.5\tSO:unknown\n@SQ\tSN:*alpha\tLN:18\n") and b"DT:2020-01-01T00:00:00Z" in text
    want = b"".join(records_py(_NAMES, _SEQS, _QUALS, c, lambda p, y: _PATHS[p][1][y]) for c in _CALLS)
    assert records == want, (aux_of(records), aux_of(want))


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return the_case(tmp_path_factory)


def _random_records(case, rng, n_reads, per_read):
    plen = case.index.arrays["path_len"].astype(np.int64)
    names, seqs, quals, recs = [], [], [], []
    for r in range(n_reads):
        L = int(rng.integers(17, 151))
        names.append(b"read%d/%d" % (r, r & 1) if r != 3 else b"n" * 254)
        seqs.append(bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), L)))
        quals.append(bytes(rng.integers(33, 74, L if r % 5 else L // 2).astype(np.uint8)))
        for _ in range(int(rng.integers(0, per_read + 1))):
            p = int(rng.choice(np.flatnonzero(plen >= L)))
            d = int(rng.integers(0, 4))
            mm = sorted(rng.choice(L, d, replace=False).tolist())
            if d and rng.integers(3) == 0:
                mm[0], mm[-1] = 0, L - 1
                mm = sorted(set(mm))
                d = len(mm)
            pos = int(rng.integers(0, plen[p] - L + 1)) if rng.integers(4) else int(plen[p]) - L
            recs.append((r, p, pos, int(rng.integers(2)), d, tuple(mm + [F] * (3 - d))))
    return names, seqs, quals, recs


def test_library_on_random_records(case, tmp_path):
    """the library's writer on a few hundred random records over the eight graphs -- any path, any pos up to the path's last base, both
    strands, d = 0 .. 3 with offsets at either end -- in two calls, byte for byte the restatement after inflation"""
    rng = np.random.default_rng(23)
    texts = case.texts

    def ref_base(p, y):
        t, first = texts[p]
        return t[y - first] if first <= y < first + len(t) else ord("N")

    out = str(tmp_path / "rescued.bam")
    w = host.BamWriter(out, case.index, date="2020-01-01T00:00:00Z")
    want = b""
    for call in range(2):
        names, seqs, quals, recs = _random_records(case, rng, 60, 4)
        arr = np.zeros(len(recs), dtype=device.RESCUE_RECORD_DTYPE)
        for i, (r, p, pos, strand, d, mm) in enumerate(recs):
            arr[i] = (r, p, pos, mm, strand, d)
        assert w.write_rescued(arr, names, seqs, quals) == len(recs) > 60
        want += records_py(names, seqs, quals, recs, ref_base)
    w.close()
    text, refs, records = split_bam(out)
    assert len(refs) == case.index.view.n_paths
    assert records == want
    aux = aux_of(records)
    assert {a[4]["NM"] for a in aux} == {0, 1, 2, 3} and any(a[4]["MD"].startswith("0") and a[4]["NM"] for a in aux) and any(a[4]["MD"].endswith("0") and a[4]["NM"] for a in aux)
    assert any(a[3] & 0x100 for a in aux) and any(a[3] & 0x10 for a in aux)


def test_library_on_long_and_palindromic_records(tmp_path_factory, native_libs, tmp_path):
    """the definition's records of tests/rescue_records_shapes_case.py (M = 2) with their own reads through the library's writer, in two
    calls split at a read boundary: byte for byte the restatement -- MD runs of three digits, SEQ / QUAL of 512 bases reversed, a hundred
    records of one read of which one is primary, and both strands of one read at one (path, pos)"""
    import re

    import rescue_records_shapes_case as shapes
    from rescue_def import path_texts
    from rescue_records_def import plain

    c = shapes.build(tmp_path_factory)[0]
    rec = c.records(2)
    texts = path_texts(c.index)
    rng = np.random.default_rng(24)
    names = [b"%s:%d" % (n.encode(), i) for i, n in enumerate(c.names)]
    quals = [bytes(rng.integers(33, 74, len(r) if i % 5 else len(r) // 2).astype(np.uint8)) for i, r in enumerate(c.reads)]
    cut = int(np.searchsorted(rec["read"], rec["read"][len(rec) // 2]))
    assert 0 < cut < len(rec) and rec["read"][cut - 1] != rec["read"][cut]
    out = str(tmp_path / "shapes.bam")
    w = host.BamWriter(out, c.index, date="2020-01-01T00:00:00Z")
    want = b""
    for part in (rec[:cut], rec[cut:]):
        assert w.write_rescued(part, names, c.reads, quals) == len(part)
        want += records_py(names, c.reads, quals, plain(part), lambda p, y: texts[p][0][y - texts[p][1]])
    w.close()
    records = split_bam(out)[2]
    assert records == want
    aux = aux_of(records)
    assert len(aux) == len(rec)
    length = {n.decode(): len(r) for n, r in zip(names, c.reads)}
    assert max(int(x) for a in aux for x in re.findall(r"\d+", a[4]["MD"])) >= 256
    assert any(a[3] & 0x10 and length[a[0]] == 512 and a[4]["NM"] for a in aux)
    flags = {}
    for a in aux:
        flags.setdefault(a[0], []).append(a[3])
    most = max(flags.values(), key=len)
    assert len(most) >= 100 and all(sum(not f & 0x100 for f in v) == 1 and not v[0] & 0x100 for v in flags.values())
    at = {}
    for a in aux:
        at.setdefault(a[:3], set()).add(a[3] & 0x10)
    assert sum(len(v) == 2 for v in at.values()) >= 10


def test_library_refuses_what_the_program_refuses(case, tmp_path):
    w = host.BamWriter(str(tmp_path / "x.bam"), case.index, date="2020-01-01T00:00:00Z")
    L = 40
    plen = case.index.arrays["path_len"].astype(np.int64)
    names, seqs, quals = [b"a"], [b"A" * L], [b"I" * L]
    for bad in [(1, 0, 0, (F, F, F), 0, 0), (0, len(plen), 0, (F, F, F), 0, 0), (0, 0, int(plen[0]) - L + 1, (F, F, F), 0, 0), (0, 0, 0, (F, F, F), 2, 0),
                (0, 0, 0, (0, 1, 2), 0, 4), (0, 0, 0, (L, F, F), 0, 1), (0, 0, 0, (65534, F, F), 0, 1), (0, 0, 0, (2, 1, F), 0, 2), (0, 0, 0, (1, 2, F), 0, 1)]:
        arr = np.zeros(1, dtype=device.RESCUE_RECORD_DTYPE)
        arr[0] = bad
        with pytest.raises(host.GrootError) as e:
            w.write_rescued(arr, names, seqs, quals)
        assert e.value.code == -1, bad
    arr = np.zeros(1, dtype=device.RESCUE_RECORD_DTYPE)
    arr[0] = (0, 0, 0, (F, F, F), 0, 0)
    with pytest.raises(host.GrootError) as e:
        w.write_rescued(arr, [b"n" * 255], seqs, quals)
    assert e.value.code == -3
    w.close()
    assert split_bam(str(tmp_path / "x.bam"))[2] == b""
