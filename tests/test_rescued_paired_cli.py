"""`groot-hip align (--paired | --interleaved) --abundance a.tsv --abundanceRescued --rescuedPaired` against the rule in plain Python
(tests/rescue_pairs_def.py): the abundance file must be, byte for byte, tests/test_abundance.py's abundance_text over the definition's ECs
-- test_paired.units_of_alns over S+(r), S(r) from the oracle's records, R(r) from the brute force of tests/rescue_sets_def.py -- whatever
the number of contexts, the batch size, or a reopen of the context in the middle of the run; with --bootstraps and --rarefy the files are
the host functions' over the same ECs; without the flag the run is refused in today's words.  The mates are the reads of
tests/test_variants_cli.py, paired from their kinds: reads of one allele, exact and across its SNP, and reads of other ARGs with one to three errors."""
import re

import numpy as np
import pytest

from groot_amd import device, host
from oracle import oracle_py as O
from rescue_pairs_def import expect
from rescue_sets_def import rescued_sets
from test_abundance import _names, abundance_text, csr
from test_coverage_cli import run
from test_variants_cli import cli, sample  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frags(sample, tmp_path_factory):
    """(R1, R2, the interleaved file, the definition at M = 2, the definition over the records alone)"""
    index, _, _, reads = sample[:4]
    # the pairing is chosen from the reads' kinds (never from device output): the first half of the reads with a record, each with one of the
    # first rescued reads -- both lists start with the allele's reads, so those fragments join -- then the rest in file order
    seq, off = O.pack_reads(reads)
    r = O.Run(index, 0.99)
    r.batch(seq, off)
    has = np.bincount(r.alns()["read_id"].astype(np.int64), minlength=len(reads)) > 0
    resc = rescued_sets(index, 2, reads, has)[0]
    E, R = np.flatnonzero(has).tolist(), sorted(resc)
    k = min(len(E), len(R)) // 2
    first = [i for pair in zip(E[:k], R[:k]) for i in pair]
    rest = [i for i in range(len(reads)) if i not in set(first)]
    order = first + rest[:len(rest) & ~1]
    reads = [reads[i] for i in order]
    reads = [reads[n ^ 1] if n & 2 else reads[n] for n in range(len(reads))]      # (every other fragment with the rescued mate first)
    tmp = tmp_path_factory.mktemp("rescued_paired_cli")
    rec = lambda i, m: b"@f%d/%d\n%s\n+\n%s\n" % (i // 2, m, reads[i], b"I" * len(reads[i]))
    (tmp / "r1.fq").write_bytes(b"".join(rec(i, 1) for i in range(0, len(reads), 2)))
    (tmp / "r2.fq").write_bytes(b"".join(rec(i, 2) for i in range(1, len(reads), 2)))
    (tmp / "il.fq").write_bytes(b"".join(rec(i, 1 + (i & 1)) for i in range(len(reads))))
    seq, off = O.pack_reads(reads)
    r = O.Run(index, 0.99)
    r.batch(seq, off)
    alns = r.alns().astype(device.ALN_DTYPE)
    exact = {}
    for i, p in zip(alns["read_id"].tolist(), alns["ref_id"].tolist()):
        exact.setdefault(i, set()).add(p)
    exact = {i: tuple(sorted(s)) for i, s in exact.items()}
    res = {i: v.paths for i, v in rescued_sets(index, 2, reads, [i in exact for i in range(len(reads))])[0].items()}
    gpo = index.arrays["graph_path_off"]
    want, plain = expect(gpo, exact, res, len(reads)), expect(gpo, exact, {}, len(reads))
    print(want.cls, want.kinds, plain.cls)
    assert want.kinds["exact_rescued_joined"] > 20 and want.kinds["rescued_rescued_joined"] > 10 and want.kinds["exact_rescued_split"] > 10 and want.rescued_mates > 100
    assert want.ecs != plain.ecs
    return str(tmp / "r1.fq"), str(tmp / "r2.fq"), str(tmp / "il.fq"), want, plain


def _line(log):
    text = open(log).read()
    m = re.search(r"abundance: (\d+) rescued mate\(s\) counted in their fragments, placed with up to (\d+) substitution\(s\): exact \+ rescued (\d+) joined, (\d+) split; "
                  r"rescued \+ rescued (\d+) joined, (\d+) split; one mate alone (\d+) exact, (\d+) rescued; (\d+) unit\(s\) on ARGs of more than 4 graphs", text)
    return text, m


def _numbers(w, M=2):
    k = w.kinds
    return (w.rescued_mates, M, k["exact_rescued_joined"], k["exact_rescued_split"], k["rescued_rescued_joined"], k["rescued_rescued_split"], k["single_exact"],
            k["single_rescued"], w.bitmap_units)


def test_abundance_file_equals_the_definition(cli, sample, frags, tmp_path):
    index, idx_dir = sample[:2]
    r1, r2, il, want, plain = frags
    names, P = _names(index), index.view.n_paths
    ecs = sorted(want.ecs.items())
    text_want, text_plain = abundance_text(names, P, ecs), abundance_text(names, P, sorted(plain.ecs.items()))
    assert text_want != text_plain
    base = [cli, "align", "-i", idx_dir, "-p", "4", "-t", "0.99", "--noBam", "--abundanceRescued", "--rescuedPaired"]
    # --paired and --interleaved, one ctx, one batch
    for name, how in (("paired", ["--paired", "-f", r1 + "," + r2]), ("inter", ["--interleaved", "-f", il])):
        a, log = str(tmp_path / (name + ".tsv")), str(tmp_path / (name + ".log"))
        r = run(base + how + ["--batch", "4096", "--abundance", a, "--log", log, "-g", str(tmp_path / ("g" + name))])
        assert r.returncode == 0, r.stderr
        assert open(a, "rb").read() == text_want
        text, m = _line(log)
        assert m and tuple(int(x) for x in m.groups()) == _numbers(want), (m and m.groups(), _numbers(want))
        assert "%d joined, %d split, %d single" % (want.cls["joined"], want.cls["split"], want.cls["single"]) in text, text
        assert "rescued read(s) counted in the equivalence classes" not in text and "reopening" not in text
    # two ctxs, small batches, with the bootstrap and the curve: the host functions over the same ECs
    a, log, rf = str(tmp_path / "ctx2.tsv"), str(tmp_path / "ctx2.log"), str(tmp_path / "ctx2.rarefy")
    r = run(base + ["--paired", "-f", r1 + "," + r2, "--gpus", "1", "--ctxPerGpu", "2", "--batch", "98", "--abundance", a, "--rescue", "2", "--bootstraps", "20",
                    "--bootSeed", "3", "--rarefy", rf, "--rarefySteps", "4", "--rarefyReps", "5", "--rarefySeed", "9", "--log", log, "-g", str(tmp_path / "g2")])
    assert r.returncode == 0, r.stderr
    host.abundance_boot_from_ecs(index, *csr(ecs), 20, seed=3, out_path=str(tmp_path / "boot.want"))
    got = open(a, "rb").read()
    assert got == (tmp_path / "boot.want").read_bytes()
    assert b"\n".join(b"\t".join(ln.split(b"\t")[:4]) for ln in got.splitlines()) + b"\n" == text_want
    host.rarefy_from_ecs(index, *csr(ecs), str(tmp_path / "rarefy.want"), n_rep=5, n_steps=4, seed=9)
    assert open(rf, "rb").read() == (tmp_path / "rarefy.want").read_bytes() != b""
    assert tuple(int(x) for x in _line(log)[1].groups()) == _numbers(want)
    # through a reopen of the ctx, beside --variants, --indels and --rescuedBam
    a, log = str(tmp_path / "grow.tsv"), str(tmp_path / "grow.log")
    r = run(base + ["--interleaved", "-f", il, "--maxReadLen", "64", "--batch", "128", "--abundance", a, "--variants", str(tmp_path / "grow.variants"),
                    "--indels", str(tmp_path / "grow.indels"), "--rescuedBam", str(tmp_path / "grow.rescued.bam"), "--log", log, "-g", str(tmp_path / "g3")])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == text_want
    text, m = _line(log)
    assert "reopening the GPU context" in text and tuple(int(x) for x in m.groups()) == _numbers(want)
    # without --abundanceRescued: pairing and the classes alone
    a = str(tmp_path / "plain.tsv")
    r = run([cli, "align", "-i", idx_dir, "-p", "4", "-t", "0.99", "--noBam", "--paired", "-f", r1 + "," + r2, "--batch", "4096", "--abundance", a,
             "--variants", str(tmp_path / "plain.variants"), "--log", str(tmp_path / "plain.log"), "-g", str(tmp_path / "g4")])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == text_plain
    assert (tmp_path / "plain.variants").read_bytes() == (tmp_path / "grow.variants").read_bytes() != b""


def test_without_the_flag_todays_refusal(cli, sample, frags, tmp_path):
    idx_dir = sample[1]
    r = run([cli, "align", "-i", idx_dir, "--noBam", "--paired", "-f", frags[0] + "," + frags[1], "--abundance", str(tmp_path / "a.tsv"), "--abundanceRescued"])
    assert r.returncode == 1
    assert r.stderr == b"--abundanceRescued cannot be combined with --paired yet: mates are rescued one by one, and a fragment's set has no rule for them\n"
