"""`groot-hip align --indels i.tsv [--rescueGap G] [--gapEventSlots N]` against the definition: the file must be, byte for byte, the
plain-Python writer (tests/test_indels.py, indels_py) applied to the brute force of the definition over all (path, strand, x, type, g, k)
(tests/gap_def.py), with "candidate and not rescued" and the rescued depth from tests/rescue_def.py and "has a record" and the exact
depth from the CPU oracle's records -- whatever the number of contexts, the batch size, or a reopen of the context in the middle of the
run.  The reads are simulated from an allele of arg-annot.90 with a planted 3-base deletion and, elsewhere in it, a planted 1-base
insertion: both lines must be in the file, and the --variants and --report files of the same run are those of a run without --indels."""
import os
import tarfile

import numpy as np
import pytest

from conftest import DATA
from gap_def import DEL, INS, Brute, GapTables
from groot_amd import device, host
from oracle import oracle_py as O
from rescue_def import Tables, _rc, path_texts
from test_coverage import expand_coverage
from test_coverage_cli import run
from test_indels import indels_py

pytestmark = pytest.mark.gpu
AT_DEL, AT_INS, G = 300, 500, 3


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """(index of the first 24 clusters of arg-annot.90, its directory, the FASTQ, the reads, the path, the two expected line heads)"""
    tmp = tmp_path_factory.mktemp("indels_cli")
    with tarfile.open(os.path.join(DATA, "arg-annot.90.tar.gz")) as tf:
        names = sorted(n for n in tf.getnames() if os.path.basename(n).startswith("cluster") and n.endswith(".msa"))[:24]
        tf.extractall(tmp, members=[tf.getmember(n) for n in names])
    index = host.Index.from_msa_files([str(tmp / n) for n in names])
    (tmp / "idx").mkdir()
    index.save(str(tmp / "idx" / "groot.gidx"))
    texts = path_texts(index)
    assert all(t is not None and t[1] == 0 for t in texts)
    rng = np.random.default_rng(31)
    p0 = next(p for p, t in enumerate(texts) if len(t[0]) >= 700 and all(c in b"ACGT" for c in t[0]))
    ref = texts[p0][0]
    ins = bytes([next(c for c in b"ACGT" if c != ref[AT_INS - 1] and c != ref[AT_INS])])      # (no neighbour alike: it stays where it is planted)
    allele = ref[:AT_DEL] + ref[AT_DEL + 3:AT_INS] + ins + ref[AT_INS:]           # the sample's allele: ref[300, 303) gone, one base in front of ref[500]
    reads = [allele[s:s + 100] for s in range(0, len(allele) - 100, 3)]
    for p in range(0, len(texts), 3):                                             # sequencing errors on other ARGs: 1, 2 and 3 per read
        t = texts[p][0]
        for k in range(6):
            s = int(rng.integers(0, len(t) - 100))
            r = bytearray(t[s:s + 100].replace(b"N", b"A"))
            for at in rng.choice(100, 1 + k % 3, replace=False):
                r[at] = int(rng.choice([c for c in b"ACGT" if c != r[at]]))
            reads.append(bytes(r))
    reads += [allele[280:350], allele[250:300] + b"N" + allele[301:350]]          # across the deletion, but too short for a gap; not A/C/G/T
    reads = [_rc(r) if i & 1 else r for i, r in enumerate(reads)]
    fq = tmp / "sample.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    s = AT_DEL                                                                    # the deletion, left-aligned: the line names the base before it
    while ref[s - 1] == ref[s + 2]:
        s -= 1
    name = index.path_name(p0).lstrip("*").encode()
    heads = (b"%s\t%d\tDEL\t3\t%s\t" % (name, s, ref[s:s + 3]), b"%s\t%d\tINS\t1\t%s\t" % (name, AT_INS, ins))
    return index, str(tmp / "idx"), str(fq), reads, heads


_MEMO = {}


def _expected(index, reads, min_reads, min_share, M=2):
    """the file under the thresholds; the tables of the brute forces are made once"""
    if M not in _MEMO:
        seq, off = O.pack_reads(reads)
        run_ = O.Run(index, 0.99)
        run_.batch(seq, off)
        alns = run_.alns().astype(device.ALN_DTYPE)
        has = np.bincount(alns["read_id"].astype(np.int64), minlength=len(reads)) > 0
        t = Tables(index, M)
        t.add(reads, has)
        gt = GapTables(index, M, G, Brute(index, M, g_max=G))
        gt.add(reads, has)
        o = index.arrays["path_name_off"].astype(np.int64)
        names = [index.arrays["path_names"].tobytes()[a:b] for a, b in zip(o, o[1:])]
        _MEMO[M] = (gt, t, expand_coverage(index, alns, off)[1], names, int(has.sum()))
    gt, t, exact, names, mapped = _MEMO[M]
    return indels_py(names, [x[0] for x in t.texts], gt.sorted_events(), gt.gdepth, t.depth(), exact, min_reads, min_share), gt, mapped


def test_indels_file_equals_the_definition(cli, sample, tmp_path):
    index, idx_dir, fq, reads, heads = sample
    want, gt, mapped = _expected(index, reads, 1, 0.0)                # (every event and every substitution a line: the variants file is not empty)
    lines = [next(ln for ln in want.split(b"\n") if ln.startswith(h)) for h in heads]                 # the planted deletion and insertion
    print(b"\n".join(lines).decode(), gt.stats, "events", len(gt.events), "reads", len(reads), "with a record", mapped)
    assert all(int(ln.split(b"\t")[5]) >= 15 for ln in lines) and gt.stats["rescued"] >= 40 and gt.stats["too_short"] >= 1 and mapped > 50
    assert gt.stats["rescued"] < gt.stats["candidates"] and gt.stats["del_placements"] >= 15 and gt.stats["ins_placements"] >= 15
    base = [cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.99", "--variantMinReads", "1", "--variantMinShare", "0"]
    outs = {}
    for tag, extra in (("one", ["--batch", "4096"]), ("ctx2", ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "97"]), ("grow", ["--maxReadLen", "64", "--batch", "128"])):
        i, v, rep, log = (str(tmp_path / (tag + e)) for e in (".indels", ".variants", ".report", ".log"))
        r = run(base + extra + ["--indels", i, "--rescueGap", str(G), "--gapEventSlots", "4096", "--variants", v, "--report", rep, "--covCutoff", "0.5", "--noBam", "--log", log,
                                "-g", str(tmp_path / ("g" + tag))])
        assert r.returncode == 0, r.stderr
        assert open(i, "rb").read() == want, tag
        ln = next(x for x in open(log) if "indels: " in x)
        assert ("indels: %d read(s) left by up to 2 substitution(s) tried with one gap of up to 3 base(s): %d rescued in %d placement(s) (%d DEL, %d INS), %d distinct event(s); "
                "left out: %d too short; %d line(s) written" % (gt.stats["candidates"], gt.stats["rescued"], gt.stats["placements"], gt.stats["del_placements"],
                                                               gt.stats["ins_placements"], len(gt.events), gt.stats["too_short"], want.count(b"\n"))) in ln, ln
        outs[tag] = (open(v, "rb").read(), open(rep, "rb").read())
    assert "reopening the GPU context" in open(str(tmp_path / "grow.log")).read() and "reopening" not in open(str(tmp_path / "one.log")).read()
    # the variants and the report beside it are those of a run without --indels
    v, rep = str(tmp_path / "plain.variants"), str(tmp_path / "plain.report")
    r = run(base + ["--batch", "4096", "--variants", v, "--report", rep, "--covCutoff", "0.5", "--noBam", "--log", str(tmp_path / "plain.log"), "-g", str(tmp_path / "gplain")])
    assert r.returncode == 0, r.stderr
    assert (open(v, "rb").read(), open(rep, "rb").read()) == outs["one"] == outs["ctx2"] == outs["grow"] and b"" not in outs["one"]


def test_alone_with_other_thresholds_and_a_table_too_small(cli, sample, tmp_path):
    """--indels without --variants (rescue and coverage are counted all the same) under the default thresholds: the two planted events
    and no other; with two slots the run fails with the reason and leaves no indels file"""
    index, idx_dir, fq, reads, heads = sample
    want, gt, _ = _expected(index, reads, 2, 0.1)
    assert [ln.startswith(h) for ln, h in zip(want.split(b"\n"), heads)] == [True, True] and want.count(b"\n") == 2 < len(gt.events)
    base = [cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.99", "--batch", "500", "--noBam", "--report", str(tmp_path / "r.tsv"), "--covCutoff", "0.5"]
    i = str(tmp_path / "i.tsv")
    r = run(base + ["--indels", i, "--log", str(tmp_path / "i.log"), "-g", str(tmp_path / "gi")])
    assert r.returncode == 0, r.stderr
    assert open(i, "rb").read() == want
    i2, log = str(tmp_path / "i2.tsv"), str(tmp_path / "i2.log")
    r = run(base + ["--indels", i2, "--gapEventSlots", "2", "--log", log, "-g", str(tmp_path / "gi2")])
    assert r.returncode == 1 and not os.path.exists(i2)
    assert "event_slots = 2" in open(log).read() and b"event_slots = 2" in r.stderr
