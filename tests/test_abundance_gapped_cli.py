"""`groot-hip align --abundance a.tsv --abundanceRescued --indels i.tsv --abundanceGapped` against the definition: the abundance file must
be, byte for byte, tests/test_abundance.py's abundance_text over the ECs of the definition -- the oracle's records' sets plus the
brute-forced sets of the rescued reads (tests/rescue_sets_def.py) plus those of the gap-rescued reads (tests/gap_sets_def.py) -- whatever
the number of contexts, the batch size, or a reopen of the context in the middle of the run; with --bootstraps and --rarefy the files are
the host functions' over the same ECs; without the flag the file is what --abundanceRescued alone writes, and the indels and variants files
do not depend on the flag.  The index and the reads are those of tests/gap_ec_case.py."""
import re

import pytest

import gap_ec_case
from gap_sets_def import ecs_plus3
from groot_amd import host
from test_abundance import _names, abundance_text, csr
from test_coverage_cli import run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


@pytest.fixture(scope="module")
def sample(tmp_path_factory, native_libs):
    """(the case, its index directory, its reads as a FASTQ file)"""
    case = gap_ec_case.case(tmp_path_factory)
    tmp = tmp_path_factory.mktemp("abundance_gapped_cli")
    (tmp / "idx").mkdir()
    case.index.save(str(tmp / "idx" / "groot.gidx"))
    fq = tmp / "sample.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(case.reads)))
    return case, str(tmp / "idx"), str(fq)


def _gap_line(log):
    text = open(log).read()
    return text, re.search(r"abundance: (\d+) gap-placed read\(s\) counted in the equivalence classes with them, placed with one deletion or insertion of up to (\d+) "
                           r"base\(s\); (\d+) of them", text)


def test_abundance_file_equals_the_definition(cli, sample, tmp_path):
    case, idx_dir, fq = sample
    index = case.index
    ex, res, gap = case.exact(), case.rescued(2)[0], case.gapped(2, 3)[0]
    ecs, today = sorted(ecs_plus3(ex, res, gap).items()), sorted(ecs_plus3(ex, res, {}).items())
    n_slow = sum(case.graphs_of(g.paths) > 4 for g in gap.values())
    names, P = _names(index), index.view.n_paths
    want, without = abundance_text(names, P, ecs), abundance_text(names, P, today)
    assert len(gap) >= 100 and n_slow >= 3 and want != without and want.count(b"\n") >= without.count(b"\n") > 0
    # (-t 0.9: the threshold the case's records were made with)
    base = [cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.9", "--noBam", "--gapEventSlots", "4096", "--variantMinReads", "1", "--variantMinShare", "0"]
    on = ["--abundanceRescued", "--abundanceGapped"]
    # one ctx, one batch
    a, log, i1, v1 = (str(tmp_path / ("one" + e)) for e in (".tsv", ".log", ".indels", ".variants"))
    r = run(base + on + ["--batch", "4096", "--abundance", a, "--indels", i1, "--variants", v1, "--log", log, "-g", str(tmp_path / "g1")])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == want
    text, m = _gap_line(log)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (len(gap), 3, n_slow), m
    assert "%d rescued read(s) counted in the equivalence classes beside %d read(s)" % (len(res), len(ex)) in text and "reopening" not in text
    # two ctxs, small batches, with the bootstrap and the curve: the host functions over the same ECs
    a, log, rf = str(tmp_path / "ctx2.tsv"), str(tmp_path / "ctx2.log"), str(tmp_path / "ctx2.rarefy")
    r = run(base + on + ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "97", "--abundance", a, "--indels", str(tmp_path / "ctx2.indels"), "--rescueGap", "3", "--bootstraps", "20",
                         "--bootSeed", "3", "--rarefy", rf, "--rarefySteps", "4", "--rarefyReps", "5", "--rarefySeed", "9", "--log", log, "-g", str(tmp_path / "g2")])
    assert r.returncode == 0, r.stderr
    host.abundance_boot_from_ecs(index, *csr(ecs), 20, seed=3, out_path=str(tmp_path / "boot.want"))
    got = open(a, "rb").read()
    assert got == (tmp_path / "boot.want").read_bytes()
    assert b"\n".join(b"\t".join(ln.split(b"\t")[:4]) for ln in got.splitlines()) + b"\n" == want
    host.rarefy_from_ecs(index, *csr(ecs), str(tmp_path / "rarefy.want"), n_rep=5, n_steps=4, seed=9)
    assert open(rf, "rb").read() == (tmp_path / "rarefy.want").read_bytes() != b""
    assert _gap_line(log)[1].group(1) == str(len(gap))
    assert (tmp_path / "ctx2.indels").read_bytes() == open(i1, "rb").read()
    # through a reopen of the ctx
    a, log = str(tmp_path / "grow.tsv"), str(tmp_path / "grow.log")
    r = run(base + on + ["--maxReadLen", "64", "--batch", "128", "--abundance", a, "--indels", str(tmp_path / "grow.indels"), "--log", log, "-g", str(tmp_path / "g3")])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == want
    text, m = _gap_line(log)
    assert "reopening the GPU context" in text and (int(m.group(1)), int(m.group(3))) == (len(gap), n_slow)
    # without the flag: what --abundanceRescued alone writes, and the same indels and variants beside it
    a, log, i0, v0 = (str(tmp_path / ("plain" + e)) for e in (".tsv", ".log", ".indels", ".variants"))
    r = run(base + ["--abundanceRescued", "--batch", "4096", "--abundance", a, "--indels", i0, "--variants", v0, "--log", log, "-g", str(tmp_path / "g4")])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == without and _gap_line(log)[1] is None
    assert open(i1, "rb").read() == open(i0, "rb").read() != b""
    assert open(v1, "rb").read() == open(v0, "rb").read() != b""
