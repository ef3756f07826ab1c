"""The tables of mismatch rescue as a plain host function (build_rescue_tables, groot_amd/csrc/hip/index_tables.hpp), on a CPU:
tools/rescue_tables_check.cpp is compiled with the host library's sources under AddressSanitizer + UBSan and run as a child process.  It
builds an index from test.gfa, test2.gfa, test-genes.msa and the first 24 clusters of arg-annot.90 and one hand-made view (a path without
a text, an 'N', a 16-mer in three paths, a path shorter than 16 bases), runs the builder on each and checks it against a restatement from
the view alone: the texts, the 'N' tags, and that every 16-mer of every text finds exactly its occurrences.

The hand-made line is pinned from the view itself: texts of 56, 48, 28 and 6 bases (the path through the empty node has none); 41 + 33 +
13 + 0 windows of 16 bases, six of them over the 'N' at base 50 of the first text: 81 occurrences; node 0's thirteen 16-mers are in three
texts each: 13 + (35 - 13) + (33 - 13) = 55 distinct, in a table of 128 slots (the power of two from 2 x 55)."""
import os
import subprocess
import tarfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(REPO, "tests", "golden", "data")
HOST_SRC = ["index.cpp", "gob.cpp", "graphs.cpp", "fastq.cpp", "reads.cpp", "bam.cpp", "report.cpp"]


def test_rescue_table_builder_under_sanitizers(tmp_path):
    flags = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
             "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "groot_amd", "csrc", "hip")]
    src = [os.path.join(REPO, "tools", "rescue_tables_check.cpp")] + [os.path.join(REPO, "groot_amd", "csrc", "host", f) for f in HOST_SRC]
    objs = [str(tmp_path / (os.path.basename(s) + ".o")) for s in src]
    jobs = [subprocess.Popen(flags + ["-c", s, "-o", o], stderr=subprocess.PIPE, text=True) for s, o in zip(src, objs)]
    for s, j in zip(src, jobs):
        err = j.communicate()[1]
        assert j.returncode == 0, (s, err[-3000:])
    exe = str(tmp_path / "rescue_tables_check")
    subprocess.run(flags + ["-o", exe] + objs + ["-lpthread", "-lz"], check=True)
    with tarfile.open(os.path.join(DATA, "arg-annot.90.tar.gz")) as tf:
        names = sorted(n for n in tf.getnames() if os.path.basename(n).startswith("cluster") and n.endswith(".msa"))[:24]
        tf.extractall(tmp_path, members=[tf.getmember(n) for n in names])
    args = [os.path.join(DATA, f) for f in ("test.gfa", "test2.gfa", "test-genes.msa")] + [str(tmp_path / n) for n in names]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-3000:])
    got = r.stdout.splitlines()
    assert got[-1] == "ok" and len(got) == 6, got
    assert [g.split("/rescue")[0] for g in got[:5]] == ["test.gfa", "test2.gfa", "test-genes.msa", "arg-annot.90[:24]", "hand-made"]
    # every path of the four fixture indices has a text (test_open_tables.py pins the same counts for the first pass)
    assert [g.split("  ")[1].split(" bases")[0] for g in got[:4]] == ["6 of 6 paths, 4484", "2 of 2 paths, 1650", "81 of 81 paths, 66774", "29 of 29 paths, 21729"]
    assert got[4] == "hand-made/rescue  4 of 5 paths, 138 bases, 81 occurrences of 55 16-mers, 128 slots"
