"""`--bootstraps B [--bootSeed S]` on `groot-hip align --abundance` and `groot-hip report --abundance`: four more columns per line,
boot_mean / boot_sd / boot_lo / boot_hi ("%.2f") of B replicates of the reads resampled with replacement, each with its own EM
(include/groot_host.h, "bootstrap intervals").  `align` draws and fits the replicates on the GPU, `report` on -p host threads: both write
the same bytes, and without --bootstraps every file is what it was."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, REPO
from groot_amd import host
from test_abundance import csr, ecs_of_alns
from test_coverage import clipped_reads
from test_shared_reads import _oracle_alns


def run(cmd):
    return subprocess.run(cmd, cwd=REPO, capture_output=True, timeout=900)


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as g

    return g.build_cli()


def test_report_bootstraps_equals_the_writer(cli, small_index, tmp_path):
    """`report --bamFile x.bam --abundance a.tsv --bootstraps B` == groot_host_report_abundance_boot == the writer on the records' ECs"""
    b, al = _oracle_alns(small_index, clipped_reads(small_index, 2500, 17))
    al = al[np.random.default_rng(5).permutation(len(al))]
    bam = str(tmp_path / "x.bam")
    w = host.BamWriter(bam, small_index, date="2020-01-01T00:00:00Z")
    w.write(al, b)
    w.close()
    r = run([cli, "report", "--bamFile", bam, "--abundance", str(tmp_path / "plain.tsv"), "--log", str(tmp_path / "p.log")])
    assert r.returncode == 0, r.stderr
    plain = (tmp_path / "plain.tsv").read_bytes()
    assert plain.count(b"\n") > 3
    for B, seed, p in ((20, None, "1"), (41, 7, "4")):
        a = tmp_path / f"a{B}.tsv"
        cmd = [cli, "report", "--bamFile", bam, "--abundance", str(a), "--bootstraps", str(B), "-p", p, "--log", str(tmp_path / "r.log")]
        r = run(cmd + (["--bootSeed", str(seed)] if seed else []))
        assert r.returncode == 0, r.stderr
        assert f"bootstrap: {B} replicate(s)" in open(tmp_path / "r.log").read()
        got = a.read_bytes()
        host.report_abundance_boot(bam, B, seed=seed or 1, threads=3, out_path=str(tmp_path / "w.tsv"))
        assert got == (tmp_path / "w.tsv").read_bytes()
        host.abundance_boot_from_ecs(small_index, *csr(ecs_of_alns(al)), B, seed=seed or 1, out_path=str(tmp_path / "e.tsv"))
        assert got == (tmp_path / "e.tsv").read_bytes()
        rows = [ln.split(b"\t") for ln in got.splitlines()]
        assert all(len(x) == 8 for x in rows) and b"\n".join(b"\t".join(x[:4]) for x in rows) + b"\n" == plain
        assert all(float(x[6]) <= float(x[4]) <= float(x[7]) for x in rows) and any(float(x[5]) > 0 for x in rows)
    assert (tmp_path / "a20.tsv").read_bytes() != (tmp_path / "a41.tsv").read_bytes()
    # --bootstraps without --abundance
    r = run([cli, "report", "--bamFile", bam, "--bootstraps", "5", "--log", str(tmp_path / "x.log")])
    assert r.returncode != 0 and b"--bootstraps" in r.stderr and b"--abundance" in r.stderr


@pytest.mark.gpu
def test_align_bootstraps_equals_report_bootstraps(cli, hip_lib, argannot_index, tmp_path):
    idx_dir = tmp_path / "idx"
    idx_dir.mkdir()
    argannot_index.save(str(idx_dir / "groot.gidx"))
    fqs = ",".join(os.path.join(DATA, f) for f in ("full-argannot-perfect-reads-small.fq.gz", "full-argannot-perfect-reads-small-variable-rl.fq.gz",
                                                   "argannot-150bp-10000-reads.fq.gz"))
    base = [cli, "align", "-i", str(idx_dir), "-f", fqs, "--batch", "1500", "-p", "4", "-t", "0.97"]
    bam, plain = str(tmp_path / "x.bam"), str(tmp_path / "plain.tsv")
    r = run(base + ["--bam", bam, "--abundance", plain, "--log", str(tmp_path / "p.log"), "-g", str(tmp_path / "gp")])
    assert r.returncode == 0, r.stderr
    plain = open(plain, "rb").read()
    assert plain.count(b"\n") > 5
    r = run([cli, "report", "--bamFile", bam, "--abundance", str(tmp_path / "b.tsv"), "--bootstraps", "20", "-p", "8", "--log", str(tmp_path / "r.log")])
    assert r.returncode == 0, r.stderr
    want = open(tmp_path / "b.tsv", "rb").read()
    rows = [ln.split(b"\t") for ln in want.splitlines()]
    assert all(len(x) == 8 for x in rows) and b"\n".join(b"\t".join(x[:4]) for x in rows) + b"\n" == plain
    assert any(float(x[5]) > 0 for x in rows)
    for tag, extra in (("nobam", []), ("ctx2", ["--ctxPerGpu", "2", "--depth", "2"])):
        a, log = str(tmp_path / f"{tag}.tsv"), str(tmp_path / f"{tag}.log")
        r = run(base + ["--abundance", a, "--bootstraps", "20", "--noBam", "--log", log, "-g", str(tmp_path / f"g{tag}")] + extra)
        assert r.returncode == 0, r.stderr
        assert "bootstrap: 20 replicate(s)" in open(log).read()
        assert open(a, "rb").read() == want, tag
    # --bootSeed 7 on both sides
    r = run([cli, "report", "--bamFile", bam, "--abundance", str(tmp_path / "b7.tsv"), "--bootstraps", "20", "--bootSeed", "7", "--log", str(tmp_path / "r7.log")])
    assert r.returncode == 0, r.stderr
    want7 = open(tmp_path / "b7.tsv", "rb").read()
    assert want7 != want
    r = run(base + ["--abundance", str(tmp_path / "a7.tsv"), "--bootstraps", "20", "--bootSeed", "7", "--noBam", "--log", str(tmp_path / "a7.log"), "-g", str(tmp_path / "g7")])
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "a7.tsv", "rb").read() == want7
    # the same align without --bootstraps still writes exactly the first four columns
    r = run(base + ["--abundance", str(tmp_path / "n.tsv"), "--noBam", "--log", str(tmp_path / "n.log"), "-g", str(tmp_path / "gn")])
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "n.tsv", "rb").read() == plain and "bootstrap:" not in open(tmp_path / "n.log").read()
    # --bootstraps needs --abundance
    r = run(base + ["--bootstraps", "5", "--bam", str(tmp_path / "z.bam"), "--log", str(tmp_path / "z.log"), "-g", str(tmp_path / "gz")])
    assert r.returncode != 0 and b"--bootstraps" in r.stderr and b"--abundance" in r.stderr
