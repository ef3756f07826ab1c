"""`groot-hip align --abundance a --calls c [--callDepth 1.0] [--covCutoff 0.97] [--noBam]`: per line of the abundance file the pileup of
the reads the EM assigns to the ARG, from the table of (class, ARG, interval) tuples counted on the GPU -- byte for byte what
`groot-hip report --bamFile b --abundance a2 --calls c2` writes for the BAM of the same run (read names are unique in these inputs).
Line format: name \\t em_reads (%.2f) \\t length \\t depth (%.2f) \\t breadth (%.4f) \\t cigar \\t called."""
import os

import pytest

from conftest import DATA
from test_abundance_cli import _idx
from test_coverage_cli import _mixed_fastq, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


def test_calls_equal_the_calls_of_the_bam(cli, argannot_index, tmp_path):
    idx_dir = _idx(argannot_index, tmp_path)
    fqs = ",".join(os.path.join(DATA, f) for f in ("full-argannot-perfect-reads-small.fq.gz", "full-argannot-perfect-reads-small-variable-rl.fq.gz",
                                                   "argannot-150bp-10000-reads.fq.gz"))
    base = [cli, "align", "-i", idx_dir, "-f", fqs, "--batch", "1500", "-p", "4", "-t", "0.97"]
    bam, a0 = str(tmp_path / "x.bam"), str(tmp_path / "a0.tsv")
    # the abundance file without --calls: what --calls must leave as it is
    r = run(base + ["--bam", bam, "--abundance", a0, "--log", str(tmp_path / "a0.log"), "-g", str(tmp_path / "g0")])
    assert r.returncode == 0, r.stderr
    r = run([cli, "report", "--bamFile", bam, "--abundance", str(tmp_path / "b.tsv"), "--calls", str(tmp_path / "bc.tsv"), "--log", str(tmp_path / "r.log")])
    assert r.returncode == 0, r.stderr
    assert "calls: " in open(tmp_path / "r.log").read()
    want_a, want = open(a0, "rb").read(), open(tmp_path / "bc.tsv", "rb").read()
    assert open(tmp_path / "b.tsv", "rb").read() == want_a
    print(want.decode())
    rows = [ln.split(b"\t") for ln in want.splitlines()]
    assert len(rows) == want_a.count(b"\n") > 5 and all(len(x) == 7 for x in rows)
    assert [x[0] for x in rows] == [ln.split(b"\t")[0] for ln in want_a.splitlines()]                     # a line per line of the abundance file
    assert [x[1] for x in rows] == [ln.split(b"\t")[2] for ln in want_a.splitlines()]                     # em_reads
    assert all(0.0 <= float(x[4]) <= 1.0 and x[6] == (b"1" if float(x[4]) >= 0.97 else b"0") for x in rows if abs(float(x[4]) - 0.97) > 1e-3)
    # (these inputs are thin: a few reads per ARG, no line reaches 0.97 at depth 1.0; both values of `called` are met below)
    for tag, extra in (("bam", ["--bam", str(tmp_path / "y.bam")]), ("nobam", ["--noBam"]),
                       ("ctx2", ["--ctxPerGpu", "2", "--batch", "1001", "--noBam"]),
                       ("all", ["--noBam", "--report", str(tmp_path / "rep.tsv"), "--sharedReads", str(tmp_path / "sh.tsv"), "--bootstraps", "3"])):
        ab, c, log = str(tmp_path / f"{tag}.a.tsv"), str(tmp_path / f"{tag}.c.tsv"), str(tmp_path / f"{tag}.log")
        r = run(base + ["--abundance", ab, "--calls", c, "--log", log, "-g", str(tmp_path / f"g{tag}")] + extra)
        assert r.returncode == 0, r.stderr
        assert open(c, "rb").read() == want, tag
        got_a = open(ab, "rb").read()
        if tag == "all":             # the bootstrap columns behind the same four
            assert [b"\t".join(ln.split(b"\t")[:4]) for ln in got_a.splitlines()] == want_a.splitlines()
        else:
            assert got_a == want_a, tag
        assert "calls: " in open(log).read() and " tuple(s) of (class, ARG, interval)" in open(log).read()
    # the report and the shared-reads file beside --calls are the files without it
    r = run(base + ["--noBam", "--abundance", str(tmp_path / "n.a.tsv"), "--report", str(tmp_path / "rep0.tsv"), "--sharedReads", str(tmp_path / "sh0.tsv"),
                    "--log", str(tmp_path / "n.log"), "-g", str(tmp_path / "gn")])
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "rep0.tsv", "rb").read() == open(tmp_path / "rep.tsv", "rb").read() != b""
    assert open(tmp_path / "sh0.tsv", "rb").read() == open(tmp_path / "sh.tsv", "rb").read() != b""
    # --callDepth and --covCutoff reach the writer on both sides
    opts = ["--callDepth", "0.5", "--covCutoff", "0.5", "--abundanceMin", "5"]
    r = run(base + ["--noBam", "--abundance", str(tmp_path / "o.a.tsv"), "--calls", str(tmp_path / "o.c.tsv"), "--log", str(tmp_path / "o.log"),
                    "-g", str(tmp_path / "go")] + opts)
    assert r.returncode == 0, r.stderr
    r = run([cli, "report", "--bamFile", bam, "--abundance", str(tmp_path / "p.a.tsv"), "--calls", str(tmp_path / "p.c.tsv"), "--log", str(tmp_path / "p.log")] + opts)
    assert r.returncode == 0, r.stderr
    got = open(tmp_path / "o.c.tsv", "rb").read()
    print(got.decode())
    assert got == open(tmp_path / "p.c.tsv", "rb").read() and got != want and 0 < got.count(b"\n") < want.count(b"\n")
    rows = [ln.split(b"\t") for ln in got.splitlines()]
    assert all(float(x[1]) >= 5.0 for x in rows) and {x[6] for x in rows} == {b"0", b"1"}
    assert all(x[6] == (b"1" if float(x[4]) >= 0.5 else b"0") for x in rows if abs(float(x[4]) - 0.5) > 1e-3)


def test_calls_through_the_reopen(cli, argannot_index, tmp_path):
    """a read longer than --maxReadLen reopens its context mid-run: its table is harvested before it closes and merged"""
    idx_dir = _idx(argannot_index, tmp_path)
    fq = str(tmp_path / "mixed.fq")
    _mixed_fastq(argannot_index, fq)
    bam = str(tmp_path / "big.bam")
    r = run([cli, "align", "-i", idx_dir, "-f", fq, "--batch", "128", "--maxReadLen", "1024", "--bam", bam, "--log", str(tmp_path / "big.log"),
             "-g", str(tmp_path / "gb"), "-p", "2"])
    assert r.returncode == 0, r.stderr
    r = run([cli, "report", "--bamFile", bam, "--abundance", str(tmp_path / "want.a.tsv"), "--calls", str(tmp_path / "want.c.tsv"), "--log", str(tmp_path / "r.log")])
    assert r.returncode == 0, r.stderr
    want = open(tmp_path / "want.c.tsv", "rb").read()
    assert want.count(b"\n") > 5
    for tag, extra in (("grow", []), ("grow2", ["--ctxPerGpu", "2", "--depth", "2"])):
        ab, c, log = str(tmp_path / f"{tag}.a.tsv"), str(tmp_path / f"{tag}.c.tsv"), str(tmp_path / f"{tag}.log")
        r = run([cli, "align", "-i", idx_dir, "-f", fq, "--batch", "128", "--maxReadLen", "160", "--abundance", ab, "--calls", c, "--noBam", "--log", log,
                 "-g", str(tmp_path / f"g{tag}"), "-p", "2"] + extra)
        assert r.returncode == 0, r.stderr
        assert "reopening the GPU context" in open(log).read()
        assert open(c, "rb").read() == want, tag
        assert open(ab, "rb").read() == open(tmp_path / "want.a.tsv", "rb").read(), tag


def test_calls_flag_errors(cli, argannot_index, tmp_path):
    idx_dir = _idx(argannot_index, tmp_path)
    fq = os.path.join(DATA, "full-argannot-perfect-reads-small.fq.gz")
    base = [cli, "align", "-i", idx_dir, "-f", fq, "--log", str(tmp_path / "x.log"), "-g", str(tmp_path / "gx")]
    c, a = str(tmp_path / "c.tsv"), str(tmp_path / "a.tsv")
    r = run(base + ["--calls", c, "--noBam"])
    assert r.returncode != 0 and b"--calls" in r.stderr and b"--abundance" in r.stderr
    r = run(base + ["--calls", c, "--abundance", a, "--noAlign", "--bam", str(tmp_path / "x.bam")])
    assert r.returncode != 0 and b"--noAlign" in r.stderr
    for flag, files in (("--paired", fq + "," + fq), ("--interleaved", fq)):
        r = run([cli, "align", "-i", idx_dir, "-f", files, "--log", str(tmp_path / "x.log"), "-g", str(tmp_path / "gx"), "--calls", c, "--abundance", a, "--noBam", flag])
        assert r.returncode != 0 and b"--calls cannot be combined with --paired / --interleaved" in r.stderr, r.stderr
    r = run(base + ["--calls", c, "--abundance", a, "--noBam", "--covCutoff", "1.5"])
    assert r.returncode != 0 and b"exceeds 1.0" in r.stderr
    assert not os.path.exists(c) and not os.path.exists(a)
    r = run([cli, "report", "--bamFile", str(tmp_path / "none.bam"), "--calls", c, "--log", str(tmp_path / "r.log")])
    assert r.returncode != 0 and not os.path.exists(c)
