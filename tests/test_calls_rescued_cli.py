"""`groot-hip align --abundance a.tsv --abundanceRescued --calls c.tsv --callsRescued` against the definition: the calls file must be, byte
for byte, groot_host_calls_from_table over the table of the definition -- the oracle's records plus the brute-forced placements of the
rescued reads under S+(r) (tests/rescue_calls_def.py) -- whatever the number of contexts, the batch size, or a reopen of the context in the
middle of the run; with --bootstraps --callSupport and --rarefy the files are the host functions' over the same table; without the flag the
files are today's.  The reads are those of tests/test_variants_cli.py: simulated from an allele of arg-annot.90 one substitution away from
the indexed one, plus reads of other ARGs with one to three sequencing errors.  At --callDepth 5 the planted allele has a hole around the
substitution without the flag, which the rescued reads fill: asserted on the CPU before the device is asked."""
import re

import pytest

from groot_amd import device, host
from oracle import oracle_py as O
from rescue_calls_def import exact_rows, rescued_records, table_of
from rescue_def import Tables
from rescue_sets_def import rescued_sets
from test_abundance import _names, abundance_text
from test_coverage_cli import run
from test_variants_cli import cli, sample  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEPTH = 5.0


@pytest.fixture(scope="module")
def expected(sample):
    """(the table of the definition at M = 2, the table of the records alone, rescued records)"""
    index, _, _, reads = sample[:4]
    seq, off = O.pack_reads(reads)
    r = O.Run(index, 0.99)
    r.batch(seq, off)
    alns = r.alns().astype(device.ALN_DTYPE)
    exact = {}
    for i, p in zip(alns["read_id"].tolist(), alns["ref_id"].tolist()):
        exact.setdefault(i, set()).add(p)
    exact = {i: tuple(sorted(s)) for i, s in exact.items()}
    has = [i in exact for i in range(len(reads))]
    t = Tables(index, 2)
    res, rec = rescued_sets(index, 2, reads, has, t)[0], rescued_records(index, 2, reads, has, t)
    rows = exact_rows(index, alns, off)
    assert len(res) > 100 and len(exact) > 50
    return table_of(exact, rows, res, rec), table_of(exact, rows, {}, {}), sum(len(x) for x in rec.values())


def _covered(index, table, p, tmp, tag):
    """the covered bases of path p in the calls file the host writes for `table`, and the file's bytes"""
    path = tmp / (tag + ".want")
    host.calls_from_table(index, *table.arrays(), out_path=str(path), call_depth=DEPTH)
    name = _names(index)[p].lstrip("*").encode()
    text = path.read_bytes()
    line = next(ln.split(b"\t") for ln in text.splitlines() if ln.split(b"\t")[0] == name)
    return sum(int(n) for n, op in re.findall(rb"(\d+)([MD])", line[5]) if op == b"M"), text


def test_calls_file_equals_the_definition(cli, sample, expected, tmp_path):
    index, idx_dir, fq, _, p0 = sample[:5]
    with_, without, n_rescued = expected
    # the CPU first: the planted allele is covered on more bases with the rescued reads than without them
    cov1, want = _covered(index, with_, p0, tmp_path, "with")
    cov0, today = _covered(index, without, p0, tmp_path, "without")
    plen = int(index.arrays["path_len"][p0])
    print("planted allele: %d of %d bases at depth >= %g without the rescued reads, %d with them" % (cov0, plen, DEPTH, cov1))
    assert cov0 + 20 <= cov1 <= plen and want != today
    names, P = _names(index), index.view.n_paths
    want_a, today_a = abundance_text(names, P, with_.ecs), abundance_text(names, P, without.ecs)
    base = [cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.99", "--noBam", "--callDepth", str(DEPTH)]
    flags = ["--abundanceRescued", "--callsRescued", "--callSlots", str(1 << 18)]
    # one ctx, one batch
    a, c, log = str(tmp_path / "one.a"), str(tmp_path / "one.c"), str(tmp_path / "one.log")
    r = run(base + ["--batch", "4096", "--abundance", a, "--calls", c, "--log", log, "-g", str(tmp_path / "g1")] + flags)
    assert r.returncode == 0, r.stderr
    assert open(c, "rb").read() == want and open(a, "rb").read() == want_a
    text = open(log).read()
    m = re.search(r"calls: (\d+) rescued record\(s\) counted in the pileup", text)
    assert m and int(m.group(1)) == n_rescued and "reopening" not in text, text
    # two ctxs, small batches, with the support columns and the curve: the host functions over the same table
    a, c, rf = str(tmp_path / "ctx2.a"), str(tmp_path / "ctx2.c"), str(tmp_path / "ctx2.r")
    r = run(base + ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "97", "--abundance", a, "--calls", c, "--bootstraps", "20", "--bootSeed", "3", "--callSupport",
                    "--rarefy", rf, "--rarefySteps", "4", "--rarefyReps", "5", "--rarefySeed", "9", "--log", str(tmp_path / "ctx2.log"), "-g", str(tmp_path / "g2")] + flags)
    assert r.returncode == 0, r.stderr
    host.calls_support_from_table(index, *with_.arrays(), out_path=str(tmp_path / "support.want"), n_boot=20, seed=3, call_depth=DEPTH)
    got = open(c, "rb").read()
    assert got == (tmp_path / "support.want").read_bytes()
    assert b"\n".join(b"\t".join(ln.split(b"\t")[:7]) for ln in got.splitlines()) + b"\n" == want
    off, ids, cnt, rows, n = with_.arrays()
    host.rarefy_from_ecs(index, off, ids, cnt, str(tmp_path / "rarefy.want"), n_rep=5, n_steps=4, seed=9, tuples=rows, tn=n, call_depth=DEPTH)
    assert open(rf, "rb").read() == (tmp_path / "rarefy.want").read_bytes() != b""
    # the same bytes without the extras, and through a reopen of the ctx
    for tag, extra in (("small", ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "97"]), ("grow", ["--maxReadLen", "64", "--batch", "128"])):
        a, c, log = str(tmp_path / (tag + ".a")), str(tmp_path / (tag + ".c")), str(tmp_path / (tag + ".log"))
        r = run(base + extra + ["--abundance", a, "--calls", c, "--log", log, "-g", str(tmp_path / ("g" + tag))] + flags)
        assert r.returncode == 0, r.stderr
        assert open(c, "rb").read() == want and open(a, "rb").read() == want_a, tag
        text = open(log).read()
        assert ("reopening the GPU context" in text) == (tag == "grow")
        assert int(re.search(r"calls: (\d+) rescued record\(s\)", text).group(1)) == n_rescued
    # without the flags: today's files
    a, c, log = str(tmp_path / "plain.a"), str(tmp_path / "plain.c"), str(tmp_path / "plain.log")
    r = run(base + ["--batch", "4096", "--abundance", a, "--calls", c, "--log", log, "-g", str(tmp_path / "g4")])
    assert r.returncode == 0, r.stderr
    assert open(c, "rb").read() == today and open(a, "rb").read() == today_a and "rescued record" not in open(log).read()
