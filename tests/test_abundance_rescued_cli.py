"""`groot-hip align --abundance a.tsv --abundanceRescued [--rescue M]` against the definition: the abundance file must be, byte for byte,
tests/test_abundance.py's abundance_text over the ECs of the definition -- the oracle's records' sets plus the brute-forced sets of the
rescued reads (tests/rescue_sets_def.py) -- whatever the number of contexts, the batch size, or a reopen of the context in the middle of
the run; with --bootstraps and --rarefy the files are the host functions' over the same ECs; without the flag the file is today's.  The
reads are those of tests/test_variants_cli.py: simulated from an allele of arg-annot.90 one substitution away from the indexed one, plus
reads of other ARGs with one to three sequencing errors."""
import re

import numpy as np
import pytest

from groot_amd import device, host
from oracle import oracle_py as O
from rescue_sets_def import ecs_plus, rescued_sets
from test_abundance import _names, abundance_text, csr, ecs_of_alns
from test_coverage_cli import run
from test_variants_cli import cli, sample  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected(sample):
    """(ECs of the definition at M = 2, the ECs of the records alone, reads with a record, rescued reads) as sorted (ids, reads) lists"""
    index, _, _, reads = sample[:4]
    seq, off = O.pack_reads(reads)
    r = O.Run(index, 0.99)
    r.batch(seq, off)
    alns = r.alns().astype(device.ALN_DTYPE)
    exact = {}
    for i, p in zip(alns["read_id"].tolist(), alns["ref_id"].tolist()):
        exact.setdefault(i, set()).add(p)
    exact = {i: tuple(sorted(s)) for i, s in exact.items()}
    res, left = rescued_sets(index, 2, reads, [i in exact for i in range(len(reads))])
    assert len(res) > 100 and len(left) > 0 and len(exact) > 50
    plain = ecs_of_alns(alns)
    assert sorted(ecs_plus(exact, {}).items()) == plain
    return sorted(ecs_plus(exact, res).items()), plain, len(exact), len(res)


def _log_numbers(log):
    """-> (the log, its reads with a seed, the match of the line of the rescued reads: rescued, reads with an exact alignment, M, slow).
    "total number of mapped reads" is the reference's count, the reads with a seed (boss.go:195); a unit of the classes is a read with a
    RECORD, which the new line states."""
    text = open(log).read()
    seeded = int(re.search(r"total number of mapped reads: (\d+)", text).group(1))
    m = re.search(r"abundance: (\d+) rescued read\(s\) counted in the equivalence classes beside (\d+) read\(s\) with an exact alignment, placed with up to (\d+) "
                  r"substitution\(s\); (\d+) of them", text)
    return text, seeded, m


def test_abundance_file_equals_the_definition(cli, sample, expected, tmp_path):
    index, idx_dir, fq = sample[:3]
    ecs, plain, n_exact, n_rescued = expected
    names, P = _names(index), index.view.n_paths
    want, today = abundance_text(names, P, ecs), abundance_text(names, P, plain)
    assert want != today and want.count(b"\n") >= today.count(b"\n") > 0
    base = [cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.99", "--noBam"]
    # one ctx, one batch
    a, log = str(tmp_path / "one.tsv"), str(tmp_path / "one.log")
    r = run(base + ["--batch", "4096", "--abundance", a, "--abundanceRescued", "--log", log, "-g", str(tmp_path / "g1")])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == want
    text, seeded, m = _log_numbers(log)
    assert m and (int(m.group(2)), int(m.group(1)), int(m.group(3))) == (n_exact, n_rescued, 2) and seeded >= n_exact, (seeded, m)
    assert sum(c for _, c in ecs) == int(m.group(2)) + int(m.group(1))   # every unit of the classes is a read with a record or a rescued one
    assert "variants:" not in text and "reopening" not in text
    # two ctxs, small batches, with the bootstrap and the curve: the host functions over the same ECs
    a, log, rf = str(tmp_path / "ctx2.tsv"), str(tmp_path / "ctx2.log"), str(tmp_path / "ctx2.rarefy")
    r = run(base + ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "97", "--abundance", a, "--abundanceRescued", "--rescue", "2", "--bootstraps", "20", "--bootSeed", "3",
                    "--rarefy", rf, "--rarefySteps", "4", "--rarefyReps", "5", "--rarefySeed", "9", "--log", log, "-g", str(tmp_path / "g2")])
    assert r.returncode == 0, r.stderr
    host.abundance_boot_from_ecs(index, *csr(ecs), 20, seed=3, out_path=str(tmp_path / "boot.want"))
    got = open(a, "rb").read()
    assert got == (tmp_path / "boot.want").read_bytes()
    assert b"\n".join(b"\t".join(ln.split(b"\t")[:4]) for ln in got.splitlines()) + b"\n" == want
    host.rarefy_from_ecs(index, *csr(ecs), str(tmp_path / "rarefy.want"), n_rep=5, n_steps=4, seed=9)
    assert open(rf, "rb").read() == (tmp_path / "rarefy.want").read_bytes() != b""
    assert _log_numbers(log)[2].group(1) == str(n_rescued)
    # through a reopen of the ctx, beside --variants and --indels
    a, log, v = str(tmp_path / "grow.tsv"), str(tmp_path / "grow.log"), str(tmp_path / "grow.variants")
    r = run(base + ["--maxReadLen", "64", "--batch", "128", "--abundance", a, "--abundanceRescued", "--variants", v, "--indels", str(tmp_path / "grow.indels"),
                    "--log", log, "-g", str(tmp_path / "g3")])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == want
    text, _, m = _log_numbers(log)
    assert "reopening the GPU context" in text and (int(m.group(2)), int(m.group(1))) == (n_exact, n_rescued)
    # without the flag: today's file, and the same variants and indels beside it
    a, log, v0 = str(tmp_path / "plain.tsv"), str(tmp_path / "plain.log"), str(tmp_path / "plain.variants")
    r = run(base + ["--batch", "4096", "--abundance", a, "--variants", v0, "--indels", str(tmp_path / "plain.indels"), "--log", log, "-g", str(tmp_path / "g4")])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == today and _log_numbers(log)[2] is None
    assert open(v, "rb").read() == open(v0, "rb").read() != b""
    assert (tmp_path / "grow.indels").read_bytes() == (tmp_path / "plain.indels").read_bytes()
