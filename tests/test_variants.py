"""groot_host_variants_write (include/groot_host.h, "Variants") against a plain-Python restatement of the writer: on the hand-made tables
of tools/variants_check.c, which runs the writer as a stand-alone program under AddressSanitizer + UBSan, and through the library on
random tables over a fixture index.

The writer, restated: one line  name \\t pos (1-based) \\t ref \\t alt \\t alt_reads \\t rescued_depth \\t exact_depth \\t share  per (path,
position, alt base) with alt_reads >= max(min_reads, 1) and share = alt_reads / (rescued_depth + exact_depth) >= min_share, one division in
double printed %.4f, ascending by global path, position and A, C, G, T; the name without its leading '*'."""
import os
import subprocess

import numpy as np

from groot_amd import host
from rescue_def import path_texts

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


def variants_py(names, refs, rescued, alt, exact, min_reads, min_share):
    """names / refs: per path its name and its bases by path coordinate (bytes); the three tables flat in global path order"""
    out, at = [], 0
    for name, ref in zip(names, refs):
        for y in range(len(ref)):
            for b in range(4):
                n, rd, ed = int(alt[4 * (at + y) + b]), int(rescued[at + y]), int(exact[at + y])
                if n >= max(min_reads, 1) and n / (rd + ed) >= min_share:
                    out.append(b"%s\t%d\t%c\t%c\t%d\t%d\t%d\t%s\n" % (name[1:] if name[:1] == b"*" else name, y + 1, ref[y], b"ACGT"[b], n, rd, ed, b"%.4f" % (n / (rd + ed))))
        at += len(ref)
    return b"".join(out)


# the tables of tools/variants_check.c
_NAMES, _REFS = [b"*alpha", b"beta", b"gamma"], [b"ACGTNGGA", b"ACGTNTTT", b"CAT"]
_RESCUED = [3, 0, 4, 4, 9, 2, 0, 5, 0, 10, 0, 0, 1, 0, 0, 20, 6, 0, 7]
_EXACT = [0, 7, 0, 16, 1, 0, 0, 5, 0, 30, 0, 0, 0, 0, 0, 0, 0, 0, 3]
_ALT = [0, 3, 0, 0, 0, 0, 0, 0, 1, 0, 0, 3, 2, 0, 2, 0, 4, 0, 5, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 1,
        0, 0, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 18, 0, 0,
        0, 0, 6, 0, 0, 0, 0, 0, 0, 1, 0, 6]
_CASES = [(1, 0.0), (0, 0.0), (2, 0.1), (3, 0.5), (1, 0.1), (1, 1.0), (100, 0.0)]


def test_restatement_on_the_hand_made_tables():
    """by hand: base 1 of alpha (3 C of 3 + 0), the 'N' at base 5, the share 0.1 met exactly at base 2 of beta (4 of 10 + 30)"""
    full = variants_py(_NAMES, _REFS, _RESCUED, _ALT, _EXACT, 1, 0.0).split(b"\n")
    assert full[0] == b"alpha\t1\tA\tC\t3\t3\t0\t1.0000" and b"alpha\t5\tN\tA\t4\t9\t1\t0.4000" in full and len(full) == 16 + 1      # (the sixteen non-zero alt counts: 9 on alpha, 4 on beta, 3 on gamma)
    assert b"beta\t2\tC\tA\t4\t10\t30\t0.1000" in variants_py(_NAMES, _REFS, _RESCUED, _ALT, _EXACT, 2, 0.1).split(b"\n")
    assert variants_py(_NAMES, _REFS, _RESCUED, _ALT, _EXACT, 1, 1.0) == b"alpha\t1\tA\tC\t3\t3\t0\t1.0000\nalpha\t6\tG\tT\t2\t2\t0\t1.0000\nbeta\t5\tN\tC\t1\t1\t0\t1.0000\ngamma\t1\tC\tG\t6\t6\t0\t1.0000\n"
    assert variants_py(_NAMES, _REFS, _RESCUED, _ALT, _EXACT, 100, 0.0) == b""


def test_stand_alone_program_under_sanitizers(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = ["-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(repo, "include")]
    obj, exe = str(tmp_path / "check.o"), str(tmp_path / "variants_check")
    subprocess.run(["gcc", "-std=c11"] + san + ["-c", os.path.join(repo, "tools", "variants_check.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17"] + san + ["-o", exe, obj, os.path.join(repo, "tools", "call_support_check_err.cpp"),
                                                 os.path.join(repo, "groot_amd", "csrc", "host", "report.cpp"), "-lpthread", "-lz"], check=True)
    r = subprocess.run([exe], capture_output=True)
    want = b""
    for mr, ms in _CASES:
        body = variants_py(_NAMES, _REFS, _RESCUED, _ALT, _EXACT, mr, ms)
        want += b"== case %d %s\n" % (mr, b"%.4f" % ms) + body + b"== %d lines\n" % body.count(b"\n")
    assert r.returncode == 0 and r.stderr == b"" and r.stdout == want + b"ok\n", (r.stdout, want, r.stderr[-2000:])


def test_library_on_random_tables(tmp_path):
    """test.gfa: sparse random counts, every line against the restatement; the refs are the texts of test_rescue.path_texts"""
    index = host.Index.from_gfa_files([os.path.join(DATA, "test.gfa")], host.index_params(k=7, s=10, w=30))
    texts = path_texts(index)
    plen = index.arrays["path_len"].astype(np.int64)
    assert all(t is not None and t[1] == 0 and len(t[0]) == n for t, n in zip(texts, plen))
    off = index.arrays["path_name_off"].astype(np.int64)
    names = [index.arrays["path_names"].tobytes()[a:b] for a, b in zip(off, off[1:])]
    rng = np.random.default_rng(3)
    n = int(plen.sum())
    alt = (rng.integers(0, 6, (n, 4)) * (rng.random((n, 4)) < 0.02)).astype(np.uint64)
    rescued = alt.sum(axis=1) + rng.integers(0, 5, n).astype(np.uint64)
    exact = (rng.integers(0, 40, n) * (rng.random(n) < 0.5)).astype(np.uint64)
    for mr, ms in ((2, 0.1), (1, 0.0), (3, 0.25)):
        out = tmp_path / ("v%d.tsv" % mr)
        lines = host.variants_write(index, rescued, alt, exact, str(out), mr, ms)
        want = variants_py(names, [t[0] for t in texts], rescued, alt.reshape(-1), exact, mr, ms)
        assert out.read_bytes() == want and lines == want.count(b"\n") > 10
