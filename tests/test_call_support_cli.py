"""`groot-hip align --abundance a --bootstraps B --calls c --callSupport`: three more columns of the calls file from the bootstrap replicates,
piled up on the GPU -- byte for byte what `groot-hip report --bamFile b --abundance a2 --bootstraps B --calls c2 --callSupport` computes on
host threads for the BAM of the same run (read names are unique in these inputs).  The definition, quoted from include/groot_host.h:

Inputs: canonical ECs (off, ids, count; count[e] > 0), the assigned-coverage table n(e,p,Pos,last), B >= 1 replicates:
boot_count[b][e] and alpha_b[n_paths] exactly as groot_host_em_bootstrap / groot_hip_em_bootstrap return them, callDepth, covCutoff.
d_e[x] for p in e: the number of records of (e,p,.,.) covering base x of p -- integers, as in §13.
For replicate b, EC e and p in e.  Double precision, no FMA contraction.
    denom_b(e) = 0.0; denom_b(e) = denom_b(e) + alpha_b[q], q over e in ascending ID order
    w_b(e,p)   = alpha_b[p] / denom_b(e);  0.0 when boot_count[b][e] == 0 or denom_b(e) < 2^-52 (the EM's skip)
    s_b(e)     = (double)boot_count[b][e] / (double)count[e]            (one correctly rounded division)
    f_b(e,p)   = s_b(e) * w_b(e,p)                                      (one product)
    D_p^b[x]   = 0.0; D = D + (double)d_e[x] * f_b(e,p), over the ECs that hold p, in canonical EC order
    covered_b[p] = the number of x in [0, path_len(p)) with D_p^b[x] >= callDepth                       (u32: the only thing the device returns)
    called_b[p]  = ((double)covered_b[p] / (double)path_len(p) >= covCutoff), the writer's own expression; path_len 0: breadth 0.0
Per path over b = 0 .. B-1:   support = (double)(number of b with called_b[p]) / (double)B
    v = covered_b[p] sorted ascending (integers), q = (25 * (B - 1)) / 1000 in integers (§11's rule)
    breadth_lo = (double)v[q] / (double)path_len,  breadth_hi = (double)v[B-1-q] / (double)path_len
File: every line of the calls file gets three more tab-separated columns, "support (%.3f) \t breadth_lo (%.4f) \t breadth_hi (%.4f)"; the
lines, their order and their first seven columns are the calls file's, byte for byte.
"""
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


def _seven(text):
    return [b"\t".join(ln.split(b"\t")[:7]) for ln in text.splitlines()]


def test_call_support_equals_the_support_of_the_bam(cli, argannot_index, tmp_path):
    idx_dir = _idx(argannot_index, tmp_path)
    fqs = ",".join(os.path.join(DATA, f) for f in ("full-argannot-perfect-reads-small.fq.gz", "full-argannot-perfect-reads-small-variable-rl.fq.gz",
                                                   "argannot-150bp-10000-reads.fq.gz"))
    base = [cli, "align", "-i", idx_dir, "-f", fqs, "--batch", "1500", "-p", "4", "-t", "0.97"]
    opts = ["--callDepth", "0.5", "--covCutoff", "0.5", "--abundanceMin", "5", "--bootstraps", "16"]
    bam = str(tmp_path / "x.bam")
    # without the switch: the abundance file and the seven columns that must stay as they are
    r = run(base + ["--bam", bam, "--abundance", str(tmp_path / "a0.tsv"), "--calls", str(tmp_path / "c0.tsv"), "--log", str(tmp_path / "a0.log"),
                    "-g", str(tmp_path / "g0")] + opts)
    assert r.returncode == 0, r.stderr
    want_a, seven = open(tmp_path / "a0.tsv", "rb").read(), open(tmp_path / "c0.tsv", "rb").read()
    assert seven.count(b"\n") > 3 and all(len(ln.split(b"\t")) == 7 for ln in seven.splitlines())
    assert "call support" not in open(tmp_path / "a0.log").read()
    r = run([cli, "report", "--bamFile", bam, "--abundance", str(tmp_path / "b.a.tsv"), "--calls", str(tmp_path / "b.c.tsv"), "--callSupport", "-p", "4",
             "--log", str(tmp_path / "r.log")] + opts)
    assert r.returncode == 0, r.stderr
    assert "call support: 16 replicate(s) on 4 host thread(s)" in open(tmp_path / "r.log").read()
    want = open(tmp_path / "b.c.tsv", "rb").read()
    print(want.decode())
    assert open(tmp_path / "b.a.tsv", "rb").read() == want_a
    rows = [ln.split(b"\t") for ln in want.splitlines()]
    assert all(len(x) == 10 for x in rows) and _seven(want) == seven.splitlines()
    for x in rows:
        sup, lo, hi = float(x[7]), float(x[8]), float(x[9])
        assert 0.0 <= sup <= 1.0 and 0.0 <= lo <= hi <= 1.0 and abs(sup * 16 - round(sup * 16)) < 0.01, x
    assert any(float(x[8]) < float(x[9]) for x in rows)                                         # the replicates differ
    for tag, extra in (("nobam", ["--noBam"]), ("ctx2", ["--ctxPerGpu", "2", "--batch", "1001", "--noBam"])):
        ab, c, log = str(tmp_path / f"{tag}.a.tsv"), str(tmp_path / f"{tag}.c.tsv"), str(tmp_path / f"{tag}.log")
        r = run(base + ["--abundance", ab, "--calls", c, "--callSupport", "--log", log, "-g", str(tmp_path / f"g{tag}")] + opts + extra)
        assert r.returncode == 0, r.stderr
        assert open(c, "rb").read() == want, tag
        assert open(ab, "rb").read() == want_a, tag
        text = open(log).read()
        assert "call support: 16 replicate(s), %d path(s), " % len(rows) in text and " row(s) of u32 on GPU " in text
    # another --bootSeed: other support columns behind the same seven
    r = run(base + ["--noBam", "--abundance", str(tmp_path / "s.a.tsv"), "--calls", str(tmp_path / "s.c.tsv"), "--callSupport", "--bootSeed", "77",
                    "--log", str(tmp_path / "s.log"), "-g", str(tmp_path / "gs")] + opts)
    assert r.returncode == 0, r.stderr
    other = open(tmp_path / "s.c.tsv", "rb").read()
    assert other != want and _seven(other) == seven.splitlines()
    r = run([cli, "report", "--bamFile", bam, "--abundance", str(tmp_path / "t.a.tsv"), "--calls", str(tmp_path / "t.c.tsv"), "--callSupport", "--bootSeed", "77",
             "-p", "3", "--log", str(tmp_path / "t.log")] + opts)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "t.c.tsv", "rb").read() == other


def test_call_support_flag_errors(cli, argannot_index, tmp_path):
    idx_dir = _idx(argannot_index, tmp_path)
    fq = os.path.join(DATA, "full-argannot-perfect-reads-small.fq.gz")
    base = [cli, "align", "-i", idx_dir, "-f", fq, "--log", str(tmp_path / "x.log"), "-g", str(tmp_path / "gx"), "--noBam"]
    c, a = str(tmp_path / "c.tsv"), str(tmp_path / "a.tsv")
    r = run(base + ["--abundance", a, "--bootstraps", "4", "--callSupport"])
    assert r.returncode != 0 and b"--callSupport" in r.stderr and b"it needs --calls" in r.stderr
    r = run(base + ["--abundance", a, "--calls", c, "--callSupport"])
    assert r.returncode != 0 and b"--callSupport" in r.stderr and b"it needs --bootstraps" in r.stderr
    assert not os.path.exists(c) and not os.path.exists(a)
    for extra, why in ((["--abundance", a, "--bootstraps", "4"], "--calls"), (["--abundance", a, "--calls", c], "--bootstraps")):
        r = run([cli, "report", "--bamFile", str(tmp_path / "none.bam"), "--callSupport", "--log", str(tmp_path / "r.log")] + extra)
        assert r.returncode != 0 and not os.path.exists(c)
        assert ("it needs " + why) in open(tmp_path / "r.log").read() + r.stderr.decode()
