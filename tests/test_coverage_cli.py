"""`groot-hip align --report`: the lines of `groot report` for the run, counted on the GPU, with or without a BAM -- byte for byte what
`groot-hip report --bamFile` writes for the BAM of the same run (testing/run_travis_tests.sh:36-56 for the one-gene assertion)."""
import os
import subprocess

import pytest

from conftest import DATA, REPO, read_fastq
from groot_amd import host

pytestmark = pytest.mark.gpu

B7 = "argannot~~~(Bla)B-7~~~AF189304:1-747"


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


def run(cmd):
    return subprocess.run(cmd, cwd=REPO, capture_output=True, timeout=600)


def test_travis_flow_report_without_a_bam(cli, msa_dir, tmp_path):
    idx_dir = str(tmp_path / "idx")
    assert run([cli, "index", "-m", msa_dir, "-i", idx_dir, "-w", "150", "-k", "31", "-s", "20", "--log", str(tmp_path / "i.log"), "-p", "8"]).returncode == 0
    fq = os.path.join(DATA, "bla-b7-150bp-5x.fq")
    rep = str(tmp_path / "r.tsv")
    r = run([cli, "align", "-i", idx_dir, "-f", fq, "-t", "0.99", "--report", rep, "--noBam", "-g", str(tmp_path / "g"), "--log", str(tmp_path / "a.log")])
    assert r.returncode == 0, r.stderr
    assert r.stdout == b""                                                     # no BAM on stdout either
    lines = open(rep).read().splitlines()
    assert len(lines) == 1 and lines[0].split("\t")[0] == B7
    # refusals: --report with --noAlign, a cutoff above 1.0 (cmd/report.go:95-97), --noBam alone
    for extra in (["--report", rep, "--noAlign"], ["--report", rep, "--covCutoff", "1.5"], ["--noBam"]):
        r = run([cli, "align", "-i", idx_dir, "-f", fq, "--log", str(tmp_path / "x.log"), "-g", str(tmp_path / "gx")] + extra)
        assert r.returncode != 0


def _mixed_fastq(index, path):
    """the two small fixtures + one read longer than --maxReadLen 160 in the middle (forces the reopen of its context)"""
    reads = read_fastq(os.path.join(DATA, "full-argannot-perfect-reads-small.fq.gz")) + \
        read_fastq(os.path.join(DATA, "full-argannot-perfect-reads-small-variable-rl.fq.gz"))
    gene = index.path_sequence(5, 0)
    long_read = bytes(gene[:600])
    with open(path, "wb") as f:
        for i, (n, s, q) in enumerate(reads):
            f.write(b"@" + n + b"\n" + s + b"\n+\n" + q + b"\n")
            if i == 1100:
                f.write(b"@long\n" + long_read + b"\n+\n" + b"I" * len(long_read) + b"\n")


@pytest.mark.parametrize("cutoff,low", [("0.97", False), ("0.5", False), ("0.5", True)])
def test_report_equals_report_of_the_bam(cli, argannot_index, tmp_path, cutoff, low):
    idx_dir = tmp_path / "idx"
    idx_dir.mkdir()
    argannot_index.save(str(idx_dir / "groot.gidx"))
    fqs = ",".join(os.path.join(DATA, f) for f in ("full-argannot-perfect-reads-small.fq.gz", "full-argannot-perfect-reads-small-variable-rl.fq.gz",
                                                   "argannot-150bp-10000-reads.fq.gz"))
    lc = ["--lowCov"] if low else []
    base = [cli, "align", "-i", str(idx_dir), "-f", fqs, "--batch", "1500", "-p", "4", "-t", "0.97"]
    bam = str(tmp_path / "x.bam")
    r = run(base + ["--bam", bam, "--report", str(tmp_path / "a.tsv"), "--covCutoff", cutoff, "--log", str(tmp_path / "a.log"), "-g", str(tmp_path / "ga")] + lc)
    assert r.returncode == 0, r.stderr
    r = run([cli, "report", "--bamFile", bam, "-c", cutoff, "--log", str(tmp_path / "r.log")] + lc)
    assert r.returncode == 0, r.stderr
    want = r.stdout
    assert want.count(b"\n") > (0 if low else 5)
    assert open(tmp_path / "a.tsv", "rb").read() == want
    for tag, extra in (("nobam", ["--noBam"]), ("ctx2", ["--ctxPerGpu", "2", "--depth", "2", "--bam", str(tmp_path / "y.bam")])):
        r = run(base + ["--report", str(tmp_path / f"{tag}.tsv"), "--covCutoff", cutoff, "--log", str(tmp_path / f"{tag}.log"), "-g", str(tmp_path / f"g{tag}")]
                + extra + lc)
        assert r.returncode == 0, r.stderr
        assert open(tmp_path / f"{tag}.tsv", "rb").read() == want, tag


def test_report_through_the_reopen(cli, argannot_index, tmp_path):
    """a read longer than --maxReadLen: its context is reopened mid-run (coverage carried over), and with two contexts the other one is
    reopened before the call counts are summed"""
    idx_dir = tmp_path / "idx"
    idx_dir.mkdir()
    argannot_index.save(str(idx_dir / "groot.gidx"))
    fq = str(tmp_path / "mixed.fq")
    _mixed_fastq(argannot_index, fq)
    bam = str(tmp_path / "big.bam")
    r = run([cli, "align", "-i", str(idx_dir), "-f", fq, "--batch", "128", "--maxReadLen", "1024", "--bam", bam, "--log", str(tmp_path / "big.log"),
             "-g", str(tmp_path / "gb"), "-p", "2"])
    assert r.returncode == 0, r.stderr
    r = run([cli, "report", "--bamFile", bam, "-c", "0.5", "--log", str(tmp_path / "r.log")])
    assert r.returncode == 0, r.stderr
    want = r.stdout
    assert want.count(b"\n") > 5
    for tag, extra in (("grow", []), ("grow2", ["--ctxPerGpu", "2", "--depth", "2"])):
        rep, log = str(tmp_path / f"{tag}.tsv"), str(tmp_path / f"{tag}.log")
        r = run([cli, "align", "-i", str(idx_dir), "-f", fq, "--batch", "128", "--maxReadLen", "160", "--report", rep, "--covCutoff", "0.5", "--noBam",
                 "--log", log, "-g", str(tmp_path / f"g{tag}"), "-p", "2"] + extra)
        assert r.returncode == 0, r.stderr
        assert "reopening the GPU context" in open(log).read()
        assert open(rep, "rb").read() == want, tag
