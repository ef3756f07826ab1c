"""`groot-hip align --report r --sharedReads s [--noBam]`: for every pair of reported ARGs the reads with records on both, counted on
the GPU -- byte for byte what `groot-hip report --bamFile b --sharedReads s2` writes for the BAM of the same run (read names are
unique in these inputs)."""
import os

import pytest

from conftest import DATA
from test_coverage_cli import _mixed_fastq, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


def _idx(argannot_index, tmp_path):
    idx_dir = tmp_path / "idx"
    idx_dir.mkdir()
    argannot_index.save(str(idx_dir / "groot.gidx"))
    return str(idx_dir)


@pytest.mark.parametrize("cutoff,low", [("0.97", False), ("0.5", True)])
def test_shared_equals_shared_of_the_bam(cli, argannot_index, tmp_path, cutoff, low):
    idx_dir = _idx(argannot_index, tmp_path)
    fqs = ",".join(os.path.join(DATA, f) for f in ("full-argannot-perfect-reads-small.fq.gz", "full-argannot-perfect-reads-small-variable-rl.fq.gz",
                                                   "argannot-150bp-10000-reads.fq.gz"))
    lc = ["--lowCov"] if low else []
    base = [cli, "align", "-i", idx_dir, "-f", fqs, "--batch", "1500", "-p", "4", "-t", "0.97"]
    bam = str(tmp_path / "x.bam")
    r = run(base + ["--bam", bam, "--log", str(tmp_path / "b.log"), "-g", str(tmp_path / "gb")])
    assert r.returncode == 0, r.stderr
    r = run([cli, "report", "--bamFile", bam, "-c", cutoff, "--sharedReads", str(tmp_path / "want.tsv"), "--log", str(tmp_path / "r.log")] + lc)
    assert r.returncode == 0, r.stderr
    want_report, want = r.stdout, open(tmp_path / "want.tsv", "rb").read()
    assert want.count(b"\n") > (0 if low else 5)
    assert any(ln.split(b"\t")[0] != ln.split(b"\t")[1] for ln in want.splitlines()) or low
    for tag, extra in (("nobam", ["--noBam"]), ("ctx2", ["--ctxPerGpu", "2", "--depth", "2", "--bam", str(tmp_path / "y.bam")])):
        rep, sh = str(tmp_path / f"{tag}.rep"), str(tmp_path / f"{tag}.tsv")
        r = run(base + ["--report", rep, "--sharedReads", sh, "--covCutoff", cutoff, "--log", str(tmp_path / f"{tag}.log"), "-g", str(tmp_path / f"g{tag}")]
                + extra + lc)
        assert r.returncode == 0, r.stderr
        assert open(rep, "rb").read() == want_report, tag
        assert open(sh, "rb").read() == want, tag


def test_shared_through_the_reopen(cli, argannot_index, tmp_path):
    """a read longer than --maxReadLen reopens its context mid-run: what it counted before is harvested and summed"""
    idx_dir = _idx(argannot_index, tmp_path)
    fq = str(tmp_path / "mixed.fq")
    _mixed_fastq(argannot_index, fq)
    bam = str(tmp_path / "big.bam")
    r = run([cli, "align", "-i", idx_dir, "-f", fq, "--batch", "128", "--maxReadLen", "1024", "--bam", bam, "--log", str(tmp_path / "big.log"),
             "-g", str(tmp_path / "gb"), "-p", "2"])
    assert r.returncode == 0, r.stderr
    r = run([cli, "report", "--bamFile", bam, "-c", "0.5", "--sharedReads", str(tmp_path / "want.tsv"), "--log", str(tmp_path / "r.log")])
    assert r.returncode == 0, r.stderr
    want = open(tmp_path / "want.tsv", "rb").read()
    assert want.count(b"\n") > 5
    for tag, extra in (("grow", []), ("grow2", ["--ctxPerGpu", "2", "--depth", "2"])):
        rep, sh, log = str(tmp_path / f"{tag}.rep"), str(tmp_path / f"{tag}.tsv"), str(tmp_path / f"{tag}.log")
        r = run([cli, "align", "-i", idx_dir, "-f", fq, "--batch", "128", "--maxReadLen", "160", "--report", rep, "--sharedReads", sh, "--covCutoff", "0.5",
                 "--noBam", "--log", log, "-g", str(tmp_path / f"g{tag}"), "-p", "2"] + extra)
        assert r.returncode == 0, r.stderr
        assert "reopening the GPU context" in open(log).read()
        assert open(sh, "rb").read() == want, tag


def test_shared_reads_needs_report(cli, argannot_index, tmp_path):
    idx_dir = _idx(argannot_index, tmp_path)
    fq = os.path.join(DATA, "full-argannot-perfect-reads-small.fq.gz")
    r = run([cli, "align", "-i", idx_dir, "-f", fq, "--sharedReads", str(tmp_path / "s.tsv"), "--bam", str(tmp_path / "x.bam"),
             "--log", str(tmp_path / "x.log"), "-g", str(tmp_path / "gx")])
    assert r.returncode != 0
    assert b"--sharedReads" in r.stderr and not os.path.exists(tmp_path / "s.tsv")
