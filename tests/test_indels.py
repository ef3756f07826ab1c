"""groot_host_indels_write (include/groot_host.h, "Indels") against a plain-Python restatement of the writer: on the hand-made tables of
tools/indels_check.c, which runs the writer as a stand-alone program under AddressSanitizer + UBSan, and through the library on random
events over a fixture index.

The writer, restated: one line  name \\t pos (1-based, the base before the gap) \\t DEL|INS \\t len \\t seq \\t reads \\t gap_depth \\t
rescued_depth \\t exact_depth \\t share  per event with reads >= max(min_reads, 1) and share = reads / (gap_depth + rescued_depth +
exact_depth) >= min_share, the depths at pos, one division in double printed %.4f, in the order given; seq = the deleted bases of the
path for a DEL, the inserted bases (2 bits each, A C G T = 0 1 2 3) for an INS; the name without its leading '*'."""
import os
import subprocess

import numpy as np

from groot_amd import host
from rescue_def import path_texts

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
DEL, INS = 0, 1


def indels_py(names, refs, events, gdepth, rescued, exact, min_reads, min_share):
    """names / refs: per path its name and its bases by path coordinate (bytes); events: (path, pos, type, len, seq, reads); the three
    depths flat in global path order"""
    base = np.r_[0, np.cumsum([len(r) for r in refs])]
    out = []
    for p, pos, typ, g, seq, reads in events:
        at = int(base[p]) + pos
        gd, rd, ed = int(gdepth[at]), int(rescued[at]), int(exact[at])
        if reads >= max(min_reads, 1) and reads / (gd + rd + ed) >= min_share:
            s = refs[p][pos + 1:pos + 1 + g] if typ == DEL else bytes(b"ACGT"[(seq >> (2 * j)) & 3] for j in range(g))
            name = names[p][1:] if names[p][:1] == b"*" else names[p]
            out.append(b"%s\t%d\t%s\t%d\t%s\t%d\t%d\t%d\t%d\t%s\n" % (name, pos + 1, (b"DEL", b"INS")[typ], g, s, reads, gd, rd, ed, b"%.4f" % (reads / (gd + rd + ed))))
    return b"".join(out)


# the tables of tools/indels_check.c
_NAMES, _REFS = [b"*alpha", b"beta", b"gamma"], [b"ACGTNGGA", b"ACGTNTTT", b"CAT"]
_GDEPTH = [0, 5, 0, 2, 0, 9, 1, 0, 0, 10, 0, 0, 0, 0, 0, 0, 5, 0, 2]
_RESCUED = [0, 1, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 6]
_EXACT = [0, 4, 0, 16, 0, 0, 0, 0, 0, 30, 0, 0, 0, 0, 0, 0, 5, 0, 0]
_EVENTS = [(0, 1, DEL, 2, 0, 3), (0, 3, DEL, 1, 0, 2), (0, 5, INS, 3, 11, 4), (0, 6, DEL, 1, 0, 1), (1, 1, INS, 1, 1, 4), (1, 1, INS, 8, 58596, 6), (2, 0, DEL, 2, 0, 5),
           (2, 2, INS, 1, 3, 2)]
_CASES = [(1, 0.0), (0, 0.0), (2, 0.1), (3, 0.5), (1, 0.1), (1, 1.0), (100, 0.0)]


def test_restatement_on_the_hand_made_tables():
    """by hand: the two bases behind base 2 of alpha (3 of 5 + 1 + 4), the 'N' as the deleted base, the path's last base deleted, TGA = 3 | 2 << 2 |
    0 << 4 = 11 inserted, the share 0.1 met exactly (4 of 10 + 0 + 30), eight bases inserted, an INS behind gamma's last base"""
    full = indels_py(_NAMES, _REFS, _EVENTS, _GDEPTH, _RESCUED, _EXACT, 1, 0.0).split(b"\n")
    assert full == [b"alpha\t2\tDEL\t2\tGT\t3\t5\t1\t4\t0.3000", b"alpha\t4\tDEL\t1\tN\t2\t2\t0\t16\t0.1111", b"alpha\t6\tINS\t3\tTGA\t4\t9\t3\t0\t0.3333",
                    b"alpha\t7\tDEL\t1\tA\t1\t1\t0\t0\t1.0000", b"beta\t2\tINS\t1\tC\t4\t10\t0\t30\t0.1000", b"beta\t2\tINS\t8\tACGTACGT\t6\t10\t0\t30\t0.1500",
                    b"gamma\t1\tDEL\t2\tAT\t5\t5\t0\t5\t0.5000", b"gamma\t3\tINS\t1\tT\t2\t2\t6\t0\t0.2500", b""]
    at = lambda mr, ms: [l.split(b"\t")[:2] for l in indels_py(_NAMES, _REFS, _EVENTS, _GDEPTH, _RESCUED, _EXACT, mr, ms).split(b"\n")[:-1]]
    assert at(2, 0.1) == [[b"alpha", b"2"], [b"alpha", b"4"], [b"alpha", b"6"], [b"beta", b"2"], [b"beta", b"2"], [b"gamma", b"1"], [b"gamma", b"3"]]
    assert at(3, 0.5) == [[b"gamma", b"1"]] and at(1, 1.0) == [[b"alpha", b"7"]] and at(100, 0.0) == []


def test_stand_alone_program_under_sanitizers(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(repo, "include")]
    obj, exe = str(tmp_path / "check.o"), str(tmp_path / "indels_check")
    subprocess.run(["gcc", "-std=c11"] + san + ["-c", os.path.join(repo, "tools", "indels_check.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17"] + san + ["-o", exe, obj, os.path.join(repo, "tools", "call_support_check_err.cpp"),
                                                 os.path.join(repo, "groot_amd", "csrc", "host", "report.cpp"), "-lpthread", "-lz"], check=True)
    r = subprocess.run([exe], capture_output=True)
    want = b""
    for mr, ms in _CASES:
        body = indels_py(_NAMES, _REFS, _EVENTS, _GDEPTH, _RESCUED, _EXACT, mr, ms)
        want += b"== case %d %s\n" % (mr, b"%.4f" % ms) + body + b"== %d lines\n" % body.count(b"\n")
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == want + b"ok\n", (r.stdout, want, r.stderr[-2000:])


def test_library_on_random_events(tmp_path):
    """test.gfa: random events, every line against the restatement; the refs are the texts of rescue_def.path_texts"""
    index = host.Index.from_gfa_files([os.path.join(DATA, "test.gfa")], host.index_params(k=7, s=10, w=30))
    texts = path_texts(index)
    plen = index.arrays["path_len"].astype(np.int64)
    assert all(t is not None and t[1] == 0 and len(t[0]) == n for t, n in zip(texts, plen))
    off = index.arrays["path_name_off"].astype(np.int64)
    names = [index.arrays["path_names"].tobytes()[a:b] for a, b in zip(off, off[1:])]
    rng = np.random.default_rng(5)
    base = np.r_[0, np.cumsum(plen)]
    n = int(plen.sum())
    keys = set()
    while len(keys) < 300:
        p, typ, g = int(rng.integers(len(plen))), int(rng.integers(2)), int(rng.integers(1, 9))
        keys.add((p, int(rng.integers(15, plen[p] - 16 - g)), typ, g, int(rng.integers(1 << (2 * g))) if typ == INS else 0))
    events = [k + (int(rng.integers(1, 9)),) for k in sorted(keys)]
    gdepth = np.zeros(n, dtype=np.uint64)
    for p, pos, typ, g, seq, reads in events:
        gdepth[base[p] + pos] += reads
    gdepth += rng.integers(0, 4, n).astype(np.uint64)
    rescued = (rng.integers(0, 10, n) * (rng.random(n) < 0.5)).astype(np.uint64)
    exact = (rng.integers(0, 40, n) * (rng.random(n) < 0.5)).astype(np.uint64)
    ev = np.zeros(len(events), dtype=host.GAP_EVENT_DTYPE)
    for f, col in zip(("path", "pos", "type", "len", "seq", "reads"), zip(*events)):
        ev[f] = col
    for mr, ms in ((2, 0.1), (1, 0.0), (3, 0.25)):
        out = tmp_path / ("i%d.tsv" % mr)
        lines = host.indels_write(index, ev, gdepth, rescued, exact, str(out), mr, ms)
        want = indels_py(names, [t[0] for t in texts], events, gdepth, rescued, exact, mr, ms)
        assert out.read_bytes() == want and lines == want.count(b"\n") > 10
    ev["reads"][7] = gdepth[base[ev["path"][7]] + ev["pos"][7]] + 1         # more reads than the gap depth there: refused, nothing written
    out = tmp_path / "bad.tsv"
    try:
        host.indels_write(index, ev, gdepth, rescued, exact, str(out))
        raise AssertionError("taken")
    except host.GrootError as e:
        assert e.code == -1 and not out.exists()
