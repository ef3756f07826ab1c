"""`groot-hip align --paired -f R1,R2 --abundance a.tsv --calls c.tsv --callsPaired` (and --interleaved) against the rule of
tests/acov_pairs_def.py: the calls file must be, byte for byte, test_calls.calls_text over the table restated from the CPU oracle's records
of the interleaved reads -- whatever the input form, the batch size or the number of contexts; the abundance file is that of
`--paired --abundance`, the BAM that of the unpaired run; with --bootstraps --callSupport and --rarefy the first seven columns stay and
the others are the host functions' over the same table and ECs; the log names the records piled up and left out.  The fragments are
those of tests/test_paired_cli.py on the arg-annot index."""
import gzip
import re

import numpy as np
import pytest

from acov_pairs_def import paired_table_of_alns, unit_sets_of_alns
from groot_amd import device, host
from oracle import oracle_py as O
from test_abundance import _names, em_py
from test_calls import calls_text
from test_paired_cli import _fragments, _write, run

pytestmark = pytest.mark.gpu

LINE = r"calls: (\d+) record\(s\) of fragments piled up, (\d+) left out on ARGs outside their fragment's set; (\d+) read\(s\) in joined fragments, (\d+) fragment\(s\)"


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


@pytest.fixture(scope="module")
def sample(argannot_index, tmp_path_factory):
    """(index, its directory, R1, R2, the interleaved file, the restated table, the records left out, the reads of joined fragments, the
    --abundanceMin that keeps the plain-Python pileup to a handful of ARGs)"""
    index = argannot_index
    tmp = tmp_path_factory.mktemp("calls_paired_cli")
    (tmp / "idx").mkdir()
    index.save(str(tmp / "idx" / "groot.gidx"))
    frags = _fragments(index, 1200, 78)
    r1, r2, il = _write(tmp, frags)
    seq, off = O.pack_reads([m for f in frags for m in f])
    o = O.Run(index, 0.99)
    o.batch(seq, off)
    alns = o.alns().astype(device.ALN_DTYPE)
    table, left = paired_table_of_alns(index, alns, off)
    unit, joined_reads = unit_sets_of_alns(alns, 2 * len(frags))
    # the input holds the case: joined fragments with records outside their set, split and single ones
    sets = [set() for _ in range(2 * len(frags))]
    for r, p in zip(alns["read_id"].tolist(), alns["ref_id"].tolist()):
        sets[r].add(p)
    split = sum(1 for i in range(len(frags)) if sets[2 * i] and sets[2 * i + 1] and not sets[2 * i] & sets[2 * i + 1])
    single = sum(1 for i in range(len(frags)) if bool(sets[2 * i]) != bool(sets[2 * i + 1]))
    assert left >= 100 and joined_reads >= 1000 and split >= 30 and single >= 30 and int(table.n.sum()) + left == len(alns), (left, joined_reads, split, single)
    alpha, _, _ = em_py(index.view.n_paths, table.ecs)
    cut = float(sorted(alpha)[-6])
    assert cut >= 1.0
    return index, str(tmp / "idx"), r1, r2, il, table, left, joined_reads, cut


def _inflate(p):
    return re.sub(rb"\tDT:[0-9TZ:-]+", b"\tDT:-", gzip.open(p, "rb").read())


def test_calls_file_equals_the_rule(cli, sample, tmp_path):
    index, idx_dir, r1, r2, il, table, left, joined_reads, cut = sample
    names, lens = _names(index), index.arrays["path_len"].astype(np.int64)
    want = calls_text(names, lens, table, min_reads=cut)
    assert want.count(b"\n") == 6
    base = [cli, "align", "-i", idx_dir, "-p", "4", "--abundanceMin", repr(cut)]

    def go(tag, extra):
        o = {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in ("a", "c", "log", "bam")}
        r = run(base + extra + ["--abundance", o["a"], "--log", o["log"], "-g", str(tmp_path / ("g" + tag))])
        assert r.returncode == 0, r.stderr
        return o

    plain = go("plain", ["-f", il, "--batch", "700", "--bam", str(tmp_path / "plain.bam")])
    units = go("units", ["--paired", "-f", r1 + "," + r2, "--batch", "700", "--noBam"])
    outs = [go("paired", ["--paired", "-f", r1 + "," + r2, "--batch", "700", "--calls", str(tmp_path / "paired.c"), "--callsPaired", "--bam", str(tmp_path / "paired.bam")]),
            go("inter", ["--interleaved", "-f", il, "--batch", "700", "--calls", str(tmp_path / "inter.c"), "--callsPaired", "--noBam"]),
            go("shard", ["--paired", "-f", r1 + "," + r2, "--batch", "1001", "--ctxPerGpu", "2", "--calls", str(tmp_path / "shard.c"), "--callsPaired", "--noBam"])]
    for o in outs:
        assert open(o["c"], "rb").read() == want
        assert open(o["a"], "rb").read() == open(units["a"], "rb").read() != open(plain["a"], "rb").read()
        m = re.search(LINE, open(o["log"]).read())
        assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (int(table.n.sum()), left, joined_reads), (m and m.groups(), int(table.n.sum()), left, joined_reads)
    assert _inflate(outs[0]["bam"]) == _inflate(plain["bam"])


def test_support_columns_and_the_curve_over_the_same_table(cli, sample, tmp_path):
    index, idx_dir, r1, r2, il, table, left, joined_reads, cut = sample
    names, lens = _names(index), index.arrays["path_len"].astype(np.int64)
    want = calls_text(names, lens, table, min_reads=cut)
    a, c, rf, log = (str(tmp_path / ("s" + e)) for e in (".a", ".c", ".r", ".log"))
    r = run([cli, "align", "-i", idx_dir, "-p", "4", "--abundanceMin", repr(cut), "--paired", "-f", r1 + "," + r2, "--batch", "700", "--noBam", "--abundance", a, "--calls", c,
             "--callsPaired", "--bootstraps", "20", "--bootSeed", "3", "--callSupport", "--rarefy", rf, "--rarefySteps", "4", "--rarefyReps", "5", "--rarefySeed", "9",
             "--log", log, "-g", str(tmp_path / "gs")])
    assert r.returncode == 0, r.stderr
    got = open(c, "rb").read()
    assert b"\n".join(b"\t".join(ln.split(b"\t")[:7]) for ln in got.splitlines()) + b"\n" == want
    host.calls_support_from_table(index, *table.arrays(), out_path=str(tmp_path / "support.want"), n_boot=20, seed=3, min_reads=cut)
    assert got == (tmp_path / "support.want").read_bytes() and all(len(ln.split(b"\t")) == 10 for ln in got.splitlines())
    off, ids, cnt, rows, n = table.arrays()
    host.rarefy_from_ecs(index, off, ids, cnt, str(tmp_path / "rarefy.want"), n_rep=5, n_steps=4, seed=9, min_reads=cut, tuples=rows, tn=n)
    assert open(rf, "rb").read() == (tmp_path / "rarefy.want").read_bytes() != b""
