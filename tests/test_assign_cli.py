"""`groot-hip align --assignFrom a.tsv [--minPosterior P]`: the second pass over the reads of `align --abundance a.tsv --noBam`.  Per read
only the records on the ARG with the largest em_reads are kept, with a MAPQ from the posterior -- the definition quoted in
tests/test_assign.py, whose plain-Python restatement (assign_py) is applied here to the CPU oracle's records with alpha parsed from the
abundance file by Python's float."""
import os

import pytest

from bamread import read_bam
from conftest import DATA, read_fastq
from groot_amd import device
from oracle import oracle_py as O
from test_abundance_cli import _idx
from test_assign import assign_py
from test_coverage_cli import _mixed_fastq, run

pytestmark = pytest.mark.gpu

FQS = [os.path.join(DATA, f) for f in ("full-argannot-perfect-reads-small.fq.gz", "full-argannot-perfect-reads-small-variable-rl.fq.gz")]


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


def _alpha_of(index, path):
    names = [index.path_name(p).lstrip("*") for p in range(index.view.n_paths)]
    alpha = [0.0] * len(names)
    for ln in open(path):
        c = ln.rstrip("\n").split("\t")
        alpha[names.index(c[0])] = float(c[2])
    return alpha


def _want_records(index, reads, alpha, min_post):
    """(name, ref_id, pos, flag, mapq, cigar) of every record the definition keeps, from the oracle's records of the reads"""
    seq, off = O.pack_reads([r[1] for r in reads])
    run_ = O.Run(index, 0.99)
    run_.batch(seq, off)
    alns = run_.alns().astype(device.ALN_DTYPE)
    best, mapq, kept, st = assign_py(alns, alpha, min_post, len(reads))
    out, seen = [], set()
    for a in alns[kept]:
        r = int(a["read_id"])
        m = len(reads[r][1]) - int(a["start_clip"]) - int(a["end_clip"])
        cigar = ("1H" if a["start_clip"] else "") + "%dM" % m + ("1H" if a["end_clip"] else "")
        out.append((reads[r][0].decode(), int(a["ref_id"]), int(a["pos"]), (0x100 if r in seen else 0) | (0x10 if a["rc"] else 0), int(mapq[r]), cigar))
        seen.add(r)
    return out, st, len(alns)


def _records(bam):
    return [(r["name"], r["ref_id"], r["pos"], r["flag"], r["mapq"], r["cigar"]) for r in read_bam(bam)[2]]


def test_assigned_bam_equals_the_definition(cli, argannot_index, tmp_path):
    idx_dir = _idx(argannot_index, tmp_path)
    reads = [r for f in FQS for r in read_fastq(f)]
    base = [cli, "align", "-i", idx_dir, "-f", ",".join(FQS), "--batch", "700", "-p", "4"]
    a = str(tmp_path / "a.tsv")
    r = run(base + ["--abundance", a, "--noBam", "--log", str(tmp_path / "one.log"), "-g", str(tmp_path / "g1")])
    assert r.returncode == 0, r.stderr
    alpha = _alpha_of(argannot_index, a)
    assert sum(1 for x in alpha if x > 0) > 5
    want, st, n_unfiltered = _want_records(argannot_index, reads, alpha, 0.0)
    assert 0 < len(want) < n_unfiltered and st["assigned"] > 1000 and len({w[4] for w in want}) > 1, (len(want), n_unfiltered, st)
    bam, log = str(tmp_path / "assigned.bam"), str(tmp_path / "two.log")
    r = run(base + ["--assignFrom", a, "--bam", bam, "--log", log, "-g", str(tmp_path / "g2")])
    assert r.returncode == 0, r.stderr
    assert _records(bam) == want
    line = next(ln for ln in open(log) if "assignment: " in ln and "read(s) with records" in ln)
    assert "%d read(s) with records: %d assigned (%d on a tie), %d unassigned, %d below" % (st["reads"], st["assigned"], st["ties"], st["unassigned"],
                                                                                           st["below"]) in line
    assert "%d record(s) in, %d kept" % (n_unfiltered, len(want)) in line
    # the report of that BAM == the report counted on the device beside the filter, without a BAM
    rep_bam, rep_dev = str(tmp_path / "rb.tsv"), str(tmp_path / "rd.tsv")
    r = run([cli, "report", "--bamFile", bam, "-c", "0.05", "--log", str(tmp_path / "r.log")])
    assert r.returncode == 0, r.stderr
    open(rep_bam, "wb").write(r.stdout)
    r = run(base + ["--assignFrom", a, "--report", rep_dev, "--covCutoff", "0.05", "--noBam", "--log", str(tmp_path / "three.log"), "-g", str(tmp_path / "g3")])
    assert r.returncode == 0, r.stderr
    assert open(rep_dev, "rb").read() == open(rep_bam, "rb").read() != b""
    # two ctxs on one GPU, another batch size, the structural BAM level
    for tag, extra in (("ctx2", ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "501"]), ("struct", ["--bamLevel", "-2"])):
        b2 = str(tmp_path / (tag + ".bam"))
        r = run(base + ["--assignFrom", a, "--bam", b2, "--log", str(tmp_path / (tag + ".log")), "-g", str(tmp_path / ("g" + tag))] + extra)
        assert r.returncode == 0, r.stderr
        assert _records(b2) == want, tag
    # --minPosterior
    want9, st9, _ = _want_records(argannot_index, reads, alpha, 0.9)
    assert st9["below"] > 0 and len(want9) < len(want)
    b9 = str(tmp_path / "p9.bam")
    r = run(base + ["--assignFrom", a, "--minPosterior", "0.9", "--bam", b9, "--log", str(tmp_path / "p9.log"), "-g", str(tmp_path / "g9")])
    assert r.returncode == 0, r.stderr
    assert _records(b9) == want9


def test_assignment_through_the_reopen(cli, argannot_index, tmp_path):
    """a read longer than --maxReadLen reopens its context mid-run: the new ctx gets alpha and the switch, the stats are harvested first"""
    idx_dir = _idx(argannot_index, tmp_path)
    fq = str(tmp_path / "mixed.fq")
    _mixed_fastq(argannot_index, fq)
    a = str(tmp_path / "a.tsv")
    base = [cli, "align", "-i", idx_dir, "-f", fq, "--batch", "128", "-p", "2"]
    r = run(base + ["--maxReadLen", "1024", "--abundance", a, "--noBam", "--log", str(tmp_path / "a.log"), "-g", str(tmp_path / "ga")])
    assert r.returncode == 0, r.stderr
    recs, lines = [], []
    for tag, mrl in (("big", "1024"), ("grow", "160")):
        bam, log = str(tmp_path / (tag + ".bam")), str(tmp_path / (tag + ".log"))
        r = run(base + ["--maxReadLen", mrl, "--assignFrom", a, "--bam", bam, "--log", log, "-g", str(tmp_path / ("g" + tag))])
        assert r.returncode == 0, r.stderr
        recs.append(_records(bam))
        lines.append(next(ln.split("assignment: ")[1] for ln in open(log) if "read(s) with records" in ln))
    assert "reopening the GPU context" in open(tmp_path / "grow.log").read() and "reopening" not in open(tmp_path / "big.log").read()
    assert recs[0] == recs[1] and len(recs[0]) > 1000 and lines[0] == lines[1]


def test_assign_flag_errors(cli, argannot_index, tmp_path):
    idx_dir = _idx(argannot_index, tmp_path)
    fq = FQS[0]
    a = str(tmp_path / "a.tsv")
    open(a, "w").write("")
    base = [cli, "align", "-i", idx_dir, "-f", fq, "--log", str(tmp_path / "x.log"), "-g", str(tmp_path / "gx"), "--assignFrom", a]
    out = str(tmp_path / "o.tsv")
    for extra, flag in ((["--report", out, "--sharedReads", str(tmp_path / "s.tsv")], b"--sharedReads"), (["--abundance", out], b"--abundance"),
                        (["--abundance", out, "--calls", str(tmp_path / "c.tsv")], b"--abundance"), (["--calls", str(tmp_path / "c.tsv")], b"--calls"),
                        (["--noAlign"], b"--noAlign")):
        r = run(base + ["--bam", str(tmp_path / "x.bam")] + extra)
        assert r.returncode != 0 and b"--assignFrom cannot be combined with " + flag + b": " in r.stderr, r.stderr
    for flag, files in (("--paired", fq + "," + fq), ("--interleaved", fq)):
        r = run([cli, "align", "-i", idx_dir, "-f", files, "--log", str(tmp_path / "x.log"), "-g", str(tmp_path / "gx"), "--assignFrom", a, "--noBam", flag])
        assert r.returncode != 0 and b"--assignFrom cannot be combined with " + flag.encode() + b": " in r.stderr, r.stderr
    r = run(base + ["--noBam"])
    assert r.returncode != 0 and b"--noBam without --report" in r.stderr
    r = run(base + ["--minPosterior", "1.5", "--bam", str(tmp_path / "x.bam")])
    assert r.returncode != 0 and b"--minPosterior" in r.stderr and b"[0, 1]" in r.stderr
    for bad in ("abc", "0.5x", ""):                         # no number: refused, not read as 0
        r = run(base + ["--minPosterior", bad, "--bam", str(tmp_path / "x.bam")])
        assert r.returncode != 0 and b"--minPosterior is a number" in r.stderr, r.stderr
    r = run(base + ["--bootstraps", "10", "--bam", str(tmp_path / "x.bam")])
    assert r.returncode != 0 and b"--bootstraps" in r.stderr
    r = run([cli, "align", "-i", idx_dir, "-f", fq, "--log", str(tmp_path / "x.log"), "-g", str(tmp_path / "gx"), "--minPosterior", "0.5", "--bam", str(tmp_path / "x.bam")])
    assert r.returncode != 0 and b"--minPosterior" in r.stderr and b"--assignFrom" in r.stderr
    r = run([cli, "align", "-i", idx_dir, "-f", fq, "--log", str(tmp_path / "x.log"), "-g", str(tmp_path / "gx"), "--assignFrom", str(tmp_path / "missing.tsv"),
             "--bam", str(tmp_path / "x.bam")])
    assert r.returncode != 0 and b"no file found" in r.stderr
    # a file that names an ARG the index does not have: the run ends before any read is aligned
    open(a, "w").write("nobody\t3\t2.00\t1.000000\n")
    r = run(base + ["--bam", str(tmp_path / "x.bam")])
    assert r.returncode != 0 and b"nobody" in r.stderr
    assert not os.path.exists(out)
