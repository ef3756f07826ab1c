"""`groot-hip align --abundance a [--noBam]`: per ARG the reads an EM over equivalence classes counted on the GPU assigns to it --
byte for byte what `groot-hip report --bamFile b --abundance a2` writes for the BAM of the same run (read names are unique in these
inputs).  Line format: name \\t reads \\t em_reads (%.2f) \\t fraction (%.6f), for every path with em_reads >= --abundanceMin."""
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


def test_abundance_equals_abundance_of_the_bam(cli, argannot_index, tmp_path):
    idx_dir = _idx(argannot_index, tmp_path)
    fqs = ",".join(os.path.join(DATA, f) for f in ("full-argannot-perfect-reads-small.fq.gz", "full-argannot-perfect-reads-small-variable-rl.fq.gz",
                                                   "argannot-150bp-10000-reads.fq.gz"))
    base = [cli, "align", "-i", idx_dir, "-f", fqs, "--batch", "1500", "-p", "4", "-t", "0.97"]
    bam, a = str(tmp_path / "x.bam"), str(tmp_path / "a.tsv")
    r = run(base + ["--bam", bam, "--abundance", a, "--log", str(tmp_path / "a.log"), "-g", str(tmp_path / "ga")])
    assert r.returncode == 0, r.stderr
    log = open(tmp_path / "a.log").read()
    assert "equivalence class(es), EM of" in log
    r = run([cli, "report", "--bamFile", bam, "--abundance", str(tmp_path / "b.tsv"), "--log", str(tmp_path / "r.log")])
    assert r.returncode == 0, r.stderr
    want = open(tmp_path / "b.tsv", "rb").read()
    assert want.count(b"\n") > 5
    assert open(a, "rb").read() == want
    rows = [ln.split(b"\t") for ln in want.splitlines()]
    assert all(float(x[2]) >= 1.0 and 0 < float(x[3]) <= 1.0 for x in rows)
    # the same BAM on stdin
    with open(bam, "rb") as f:
        import subprocess
        r = subprocess.run([cli, "report", "--abundance", str(tmp_path / "c.tsv"), "--log", str(tmp_path / "c.log")], stdin=f, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "c.tsv", "rb").read() == want
    for tag, extra in (("nobam", ["--noBam"]), ("ctx2", ["--ctxPerGpu", "2", "--depth", "2", "--bam", str(tmp_path / "y.bam")]),
                       ("all", ["--noBam", "--report", str(tmp_path / "rep.tsv"), "--sharedReads", str(tmp_path / "sh.tsv")])):
        ab = str(tmp_path / f"{tag}.tsv")
        r = run(base + ["--abundance", ab, "--log", str(tmp_path / f"{tag}.log"), "-g", str(tmp_path / f"g{tag}")] + extra)
        assert r.returncode == 0, r.stderr
        assert open(ab, "rb").read() == want, tag
    # --abundanceMin: the paths above it, the same lines
    r = run(base + ["--abundance", str(tmp_path / "m.tsv"), "--abundanceMin", "50", "--noBam", "--log", str(tmp_path / "m.log"), "-g", str(tmp_path / "gm")])
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "m.tsv", "rb").read().splitlines() == [x for x in want.splitlines() if float(x.split(b"\t")[2]) >= 50]


def test_abundance_through_the_reopen(cli, argannot_index, tmp_path):
    """a read longer than --maxReadLen reopens its context mid-run: what it counted before is harvested and summed"""
    idx_dir = _idx(argannot_index, tmp_path)
    fq = str(tmp_path / "mixed.fq")
    _mixed_fastq(argannot_index, fq)
    bam = str(tmp_path / "big.bam")
    r = run([cli, "align", "-i", idx_dir, "-f", fq, "--batch", "128", "--maxReadLen", "1024", "--bam", bam, "--log", str(tmp_path / "big.log"),
             "-g", str(tmp_path / "gb"), "-p", "2"])
    assert r.returncode == 0, r.stderr
    r = run([cli, "report", "--bamFile", bam, "--abundance", str(tmp_path / "want.tsv"), "--log", str(tmp_path / "r.log")])
    assert r.returncode == 0, r.stderr
    want = open(tmp_path / "want.tsv", "rb").read()
    assert want.count(b"\n") > 5
    for tag, extra in (("grow", []), ("grow2", ["--ctxPerGpu", "2", "--depth", "2"])):
        ab, log = str(tmp_path / f"{tag}.tsv"), str(tmp_path / f"{tag}.log")
        r = run([cli, "align", "-i", idx_dir, "-f", fq, "--batch", "128", "--maxReadLen", "160", "--abundance", ab, "--noBam", "--log", log,
                 "-g", str(tmp_path / f"g{tag}"), "-p", "2"] + extra)
        assert r.returncode == 0, r.stderr
        assert "reopening the GPU context" in open(log).read()
        assert open(ab, "rb").read() == want, tag


def test_abundance_flag_errors(cli, argannot_index, tmp_path):
    idx_dir = _idx(argannot_index, tmp_path)
    fq = os.path.join(DATA, "full-argannot-perfect-reads-small.fq.gz")
    base = [cli, "align", "-i", idx_dir, "-f", fq, "--log", str(tmp_path / "x.log"), "-g", str(tmp_path / "gx")]
    r = run(base + ["--abundance", str(tmp_path / "a.tsv"), "--noAlign", "--bam", str(tmp_path / "x.bam")])
    assert r.returncode != 0
    assert b"--abundance" in r.stderr and b"--noAlign" in r.stderr and not os.path.exists(tmp_path / "a.tsv")
    # refused as before
    r = run(base + ["--noBam"])
    assert r.returncode != 0 and b"--noBam without --report would leave no output of the alignments" in r.stderr
    r = run(base + ["--noBam", "--abundance", str(tmp_path / "a.tsv"), "--bam", str(tmp_path / "x.bam")])
    assert r.returncode != 0 and b"--noBam and --bam contradict each other" in r.stderr
    r = run(base + ["--sharedReads", str(tmp_path / "s.tsv"), "--abundance", str(tmp_path / "a.tsv"), "--noBam"])
    assert r.returncode != 0 and b"--sharedReads lists pairs of reported ARGs: it needs --report" in r.stderr
