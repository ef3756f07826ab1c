"""`groot-hip align --abundance a --rarefy r [--rarefySteps 10] [--rarefyReps 20] [--rarefySeed 1] [--calls c]`: the rarefaction curve of the
run, drawn and fitted on the GPU -- byte for byte what `groot-hip report --bamFile b --abundance a2 --rarefy r2 [--calls c2]` computes on
host threads for the BAM of the same run (read names are unique in these inputs).  Line format: fraction (%.4f) \\t units \\t args_mean (%.2f)
\\t args_lo \\t args_hi, with --calls also \\t called_mean (%.2f) \\t called_lo \\t called_hi; the last line is the point estimate."""
import os

import pytest

from conftest import DATA
from test_abundance_cli import _idx
from test_coverage_cli import run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


def test_rarefy_equals_the_rarefy_of_the_bam(cli, argannot_index, tmp_path):
    idx_dir = _idx(argannot_index, tmp_path)
    fqs = ",".join(os.path.join(DATA, f) for f in ("full-argannot-perfect-reads-small.fq.gz", "full-argannot-perfect-reads-small-variable-rl.fq.gz"))
    base = [cli, "align", "-i", idx_dir, "-f", fqs, "--batch", "1500", "-p", "4", "-t", "0.97"]
    opts = ["--callDepth", "0.5", "--covCutoff", "0.5", "--abundanceMin", "2"]
    rare = ["--rarefyReps", "8", "--rarefySeed", "5"]
    p = lambda name: str(tmp_path / name)                                                                  # noqa: E731
    read = lambda name: open(tmp_path / name, "rb").read()                                                 # noqa: E731
    # the run without the flag: its BAM, and the files --rarefy must leave as they are
    r = run(base + ["--bam", p("x.bam"), "--abundance", p("a0.tsv"), "--calls", p("c0.tsv"), "--log", p("a0.log"), "-g", p("g0")] + opts)
    assert r.returncode == 0, r.stderr
    want_a, want_c = read("a0.tsv"), read("c0.tsv")
    n_ab, n_called = want_a.count(b"\n"), sum(ln.endswith(b"\t1") for ln in want_c.splitlines())
    assert n_ab > 5 and 0 < n_called < n_ab
    # report on host threads: with and without --calls
    r = run([cli, "report", "--bamFile", p("x.bam"), "--abundance", p("b.a.tsv"), "--calls", p("b.c.tsv"), "--rarefy", p("b.r8.tsv"), "-p", "4", "--log", p("b.log")] + opts + rare)
    assert r.returncode == 0, r.stderr
    assert read("b.a.tsv") == want_a and read("b.c.tsv") == want_c and "rarefaction: 10 step(s), 8 replicate(s)" in open(p("b.log")).read()
    r = run([cli, "report", "--bamFile", p("x.bam"), "--abundance", p("b5.a.tsv"), "--rarefy", p("b.r5.tsv"), "-p", "2", "--log", p("b5.log")] + opts[4:] + rare)
    assert r.returncode == 0, r.stderr
    want8, want5 = read("b.r8.tsv"), read("b.r5.tsv")
    print(want8.decode())
    rows = [ln.split(b"\t") for ln in want8.splitlines()]
    assert len(rows) == 10 and all(len(x) == 8 for x in rows) and [x[0] for x in rows] == [b"%.4f" % (s / 10) for s in range(1, 11)]
    assert [b"\t".join(x[:5]) for x in rows] == want5.splitlines()                                         # the first five columns are the file without --calls
    units = int(rows[-1][1])
    assert [int(x[1]) for x in rows] == [(units // 10) * s + ((units % 10) * s) // 10 for s in range(1, 11)]
    assert rows[-1][2:5] == [b"%d.00" % n_ab, b"%d" % n_ab, b"%d" % n_ab]                                    # the last line: the abundance file's line count
    assert rows[-1][5:8] == [b"%d.00" % n_called, b"%d" % n_called, b"%d" % n_called]                       # ... and the calls file's called lines
    assert all(int(x[3]) <= float(x[2]) <= int(x[4]) and int(x[6]) <= float(x[5]) <= int(x[7]) for x in rows)
    assert float(rows[0][2]) < float(rows[-1][2]) and float(rows[0][5]) <= float(rows[-1][5])               # the curve rises over the run
    # align on the GPU: the same bytes, and the abundance and calls files are those of the run without the flag
    for tag, extra, calls in (("calls", ["--noBam"], True), ("ctx2", ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "1001", "--noBam"], True),
                              ("plain", ["--noBam"], False)):
        cmd = base + ["--abundance", p(tag + ".a.tsv"), "--rarefy", p(tag + ".r.tsv"), "--log", p(tag + ".log"), "-g", p("g" + tag)] + extra + rare
        cmd += (["--calls", p(tag + ".c.tsv")] + opts) if calls else opts[4:]
        r = run(cmd)
        assert r.returncode == 0, r.stderr
        assert read(tag + ".r.tsv") == (want8 if calls else want5), tag
        assert read(tag + ".a.tsv") == want_a and (not calls or read(tag + ".c.tsv") == want_c), tag
        log = open(p(tag + ".log")).read()
        assert "rarefaction: 10 step(s), 8 replicate(s) of %d unit(s)" % units in log and " iteration(s), 10 line(s)" in log
    # other steps, replicates and seed reach both sides
    other = ["--rarefySteps", "4", "--rarefyReps", "3", "--rarefySeed", "77"]
    r = run(base + ["--noBam", "--abundance", p("o.a.tsv"), "--rarefy", p("o.r.tsv"), "--log", p("o.log"), "-g", p("go")] + opts[4:] + other)
    assert r.returncode == 0, r.stderr
    r = run([cli, "report", "--bamFile", p("x.bam"), "--abundance", p("q.a.tsv"), "--rarefy", p("q.r.tsv"), "--log", p("q.log")] + opts[4:] + other)
    assert r.returncode == 0, r.stderr
    assert read("o.r.tsv") == read("q.r.tsv") and read("o.r.tsv").count(b"\n") == 4 and read("o.r.tsv").splitlines()[-1] == want5.splitlines()[-1]


def test_refusals(cli, argannot_index, tmp_path):
    idx_dir = _idx(argannot_index, tmp_path)
    fq = os.path.join(DATA, "full-argannot-perfect-reads-small.fq.gz")
    base = [cli, "align", "-i", idx_dir, "-f", fq, "--log", str(tmp_path / "x.log"), "-g", str(tmp_path / "gx")]
    a, rf = str(tmp_path / "a.tsv"), str(tmp_path / "r.tsv")
    r = run(base + ["--rarefy", rf, "--bam", str(tmp_path / "x.bam")])
    assert r.returncode != 0 and b"--rarefy" in r.stderr and b"it needs --abundance" in r.stderr
    open(a, "w").close()
    for extra in (["--rarefy", rf], ["--rarefy", rf, "--abundance", str(tmp_path / "a2.tsv")]):
        r = run(base + ["--assignFrom", a, "--bam", str(tmp_path / "x.bam")] + extra)
        assert r.returncode != 0 and b"--assignFrom cannot be combined with --rarefy" in r.stderr, r.stderr
    r = run([cli, "report", "--bamFile", str(tmp_path / "none.bam"), "--rarefy", rf, "--log", str(tmp_path / "r.log")])
    assert r.returncode != 0 and b"--rarefy" in r.stderr and b"it needs --abundance" in r.stderr
    r = run([cli, "report", "--bamFile", str(tmp_path / "none.bam"), "--rarefy", rf, "--abundance", a, "--paired", "--log", str(tmp_path / "r.log")])
    assert r.returncode != 0 and b"report cannot pair the records of a BAM" in r.stderr
    assert not os.path.exists(rf)
