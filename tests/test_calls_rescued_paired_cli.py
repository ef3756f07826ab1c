"""`groot-hip align (--paired | --interleaved) --abundance a.tsv --abundanceRescued --rescuedPaired --calls c.tsv --callsPaired --callsRescued
--callsRescuedPaired` against the rule in plain Python (tests/calls_rescued_pairs_def.py): the calls file must be, byte for byte,
groot_host_calls_from_table over the definition's table, whatever the number of contexts, the batch size, or a reopen of the context in the
middle of the run; with --bootstraps --callSupport and --rarefy the files are the host functions' over the same table and classes; without
the flag the run is refused in today's words.  The fragments are those of tests/test_rescued_paired_cli.py."""
import os
import re
import subprocess

import pytest

from calls_rescued_pairs_def import expect
from groot_amd import device, host
from oracle import oracle_py as O
from rescue_calls_def import exact_rows, rescued_records
from rescue_def import Tables
from rescue_sets_def import rescued_sets
from test_abundance import _names, abundance_text
from test_coverage_cli import run
from test_rescued_paired_cli import frags  # noqa: F401  (fixture)
from test_variants_cli import cli, sample  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DEPTH = 5.0


@pytest.fixture(scope="module")
def expected(sample, frags):
    """the definition at M = 2 over the mates of the interleaved file"""
    index = sample[0]
    reads = open(frags[2], "rb").read().split(b"\n")[1::4]
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
    res = {i: v.paths for i, v in rescued_sets(index, 2, reads, has, t)[0].items()}
    w = expect(index.arrays["graph_path_off"], exact, res, exact_rows(index, alns, off), rescued_records(index, 2, reads, has, t), len(reads))
    assert w.units.ecs == frags[3].ecs                                  # the classes of --rescuedPaired
    print(w.stats, w.kinds)
    assert w.stats["exact_records"] > 20 and w.stats["rescued_records"] > 100 and w.kinds["placements, rescued + rescued joined"] > 10
    return w


def _numbers(w):
    s = w.stats
    return s["exact_records"], s["exact_left_out"], s["rescued_records"], s["rescued_left_out"], s["host_records"]


def _line(text):
    m = re.search(r"calls: fragments with a rescued mate: (\d+) exact record\(s\) beside a rescued partner piled up and (\d+) left out, (\d+) placement\(s\) of rescued mates "
                  r"piled up and (\d+) left out on ARGs outside their unit; (\d+) of them on ARGs of more than 4 graphs; the table started with (\d+) slot\(s\)", text)
    return m and tuple(int(x) for x in m.groups())


def test_calls_file_equals_the_definition(cli, sample, frags, expected, tmp_path):
    index, idx_dir = sample[:2]
    r1, r2, il = frags[:3]
    w = expected
    host.calls_from_table(index, *w.table.arrays(), out_path=str(tmp_path / "calls.want"), call_depth=DEPTH)
    want = (tmp_path / "calls.want").read_bytes()
    want_a = abundance_text(_names(index), index.view.n_paths, w.table.ecs)
    slots = 1 << 18
    base = [cli, "align", "-i", idx_dir, "-p", "4", "-t", "0.99", "--noBam", "--callDepth", str(DEPTH), "--abundanceRescued", "--rescuedPaired", "--callsPaired",
            "--callsRescued", "--callsRescuedPaired", "--callSlots", str(slots)]
    # --paired and --interleaved, one ctx, one batch
    for name, how in (("paired", ["--paired", "-f", r1 + "," + r2]), ("inter", ["--interleaved", "-f", il])):
        a, c, log = str(tmp_path / (name + ".a")), str(tmp_path / (name + ".c")), str(tmp_path / (name + ".log"))
        r = run(base + how + ["--batch", "4096", "--abundance", a, "--calls", c, "--log", log, "-g", str(tmp_path / ("g" + name))])
        assert r.returncode == 0, r.stderr
        assert open(c, "rb").read() == want and open(a, "rb").read() == want_a
        text = open(log).read()
        assert _line(text) == _numbers(w) + (slots,), (_line(text), _numbers(w))
        assert "rescued mate(s) counted in their fragments" in text and "rescued record(s) counted in the pileup" not in text and "reopening" not in text
    # two ctxs, small batches, with the support columns and the curve: the host functions over the same table
    a, c, rf, log = str(tmp_path / "ctx2.a"), str(tmp_path / "ctx2.c"), str(tmp_path / "ctx2.r"), str(tmp_path / "ctx2.log")
    r = run(base + ["--paired", "-f", r1 + "," + r2, "--gpus", "1", "--ctxPerGpu", "2", "--batch", "98", "--abundance", a, "--calls", c, "--bootstraps", "20", "--bootSeed", "3",
                    "--callSupport", "--rarefy", rf, "--rarefySteps", "4", "--rarefyReps", "5", "--rarefySeed", "9", "--log", log, "-g", str(tmp_path / "g2")])
    assert r.returncode == 0, r.stderr
    host.calls_support_from_table(index, *w.table.arrays(), out_path=str(tmp_path / "support.want"), n_boot=20, seed=3, call_depth=DEPTH)
    got = open(c, "rb").read()
    assert got == (tmp_path / "support.want").read_bytes()
    assert b"\n".join(b"\t".join(ln.split(b"\t")[:7]) for ln in got.splitlines()) + b"\n" == want
    off, ids, cnt, rows, n = w.table.arrays()
    host.rarefy_from_ecs(index, off, ids, cnt, str(tmp_path / "rarefy.want"), n_rep=5, n_steps=4, seed=9, tuples=rows, tn=n, call_depth=DEPTH)
    assert open(rf, "rb").read() == (tmp_path / "rarefy.want").read_bytes() != b""
    assert _line(open(log).read()) == _numbers(w) + (slots,)
    # the same bytes from an odd batch size of fragments, and through a reopen of the ctx
    for tag, extra in (("small", ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "97"]), ("grow", ["--maxReadLen", "64", "--batch", "128"])):
        a, c, log = str(tmp_path / (tag + ".a")), str(tmp_path / (tag + ".c")), str(tmp_path / (tag + ".log"))
        r = run(base + extra + ["--interleaved", "-f", il, "--abundance", a, "--calls", c, "--log", log, "-g", str(tmp_path / ("g" + tag))])
        assert r.returncode == 0, r.stderr
        assert open(c, "rb").read() == want and open(a, "rb").read() == want_a, tag
        text = open(log).read()
        assert ("reopening the GPU context" in text) == (tag == "grow") and _line(text) == _numbers(w) + (slots,)


def test_a_table_too_small_fails_the_run(cli, sample, frags, expected, tmp_path):
    """--callSlots 2: the one-pass records of the first batch find no room; the run fails, names the flag and writes no calls file"""
    idx_dir = sample[1]
    c = tmp_path / "c.tsv"
    cmd = [cli, "align", "-i", idx_dir, "-p", "4", "-t", "0.99", "--noBam", "--abundanceRescued", "--rescuedPaired", "--callsPaired", "--callsRescued",
           "--callsRescuedPaired", "--callSlots", "2", "--interleaved", "-f", frags[2], "--batch", "4096", "--abundance", str(tmp_path / "a.tsv"), "--calls", str(c),
           "--log", str(tmp_path / "log"), "-g", str(tmp_path / "g")]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, timeout=600, env=dict(os.environ, GROOT_TEST_ACOV_SLOTS="2"))
    assert r.returncode != 0 and b"--callSlots" in r.stderr + open(str(tmp_path / "log"), "rb").read() and not c.exists()


def test_without_the_flag_todays_refusal(cli, sample, frags, tmp_path):
    idx_dir = sample[1]
    r = run([cli, "align", "-i", idx_dir, "--noBam", "--interleaved", "-f", frags[2], "--abundance", str(tmp_path / "a.tsv"), "--abundanceRescued", "--rescuedPaired",
             "--calls", str(tmp_path / "c.tsv"), "--callsPaired", "--callsRescued"])
    assert r.returncode == 1
    assert r.stderr == b"--rescuedPaired cannot be combined with --calls: its pileup has no rule for a fragment with a rescued mate\n"
