"""`groot-hip align --abundance a.tsv --abundanceRescued --indels i.tsv --abundanceGapped --calls c.tsv --callsRescued --callsGapped` against
the definition: the calls file must be, byte for byte, groot_host_calls_from_table over the table of the definition -- the oracle's
records, the brute-forced placements of the rescued reads and the gapped records of the gap-rescued reads under S++(r)
(tests/gap_calls_def.py) -- whatever the number of contexts, the batch size, or a reopen of the context in the middle of the run; with
--bootstraps --callSupport and --rarefy the files are the host functions' over the same table; without the flag the calls file is that of
--callsRescued alone, and the abundance, indels and variants files do not depend on it.  The index and the reads are those of
tests/gap_ec_case.py.  One end-to-end statement on an allele of arg-annot.90 with a planted 3-base deletion (the construction of
tests/test_variants_cli.py): at --callDepth 5 more of the allele is covered with the gap-placed reads than without them, and the deleted
bases stay uncovered -- asserted on the CPU before the device is asked."""
import os
import re
import tarfile

import numpy as np
import pytest

import gap_def
import gap_ec_case
from conftest import DATA
from gap_calls_def import gap_calls, rows_of, table_of3
from gap_sets_def import gap_sets
from groot_amd import device, host
from oracle import oracle_py as O
from rescue_calls_def import exact_rows, rescued_records
from rescue_def import A, Tables, _rc, path_texts
from rescue_sets_def import rescued_sets
from test_abundance import _names, abundance_text
from test_coverage_cli import run

pytestmark = pytest.mark.gpu

LINE = r"calls: (\d+) gapped placement\(s\) of gap-placed reads piled up as (\d+) record\(s\), a deletion as two and an insertion as one, (\d+) of them"


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


@pytest.fixture(scope="module")
def sample(tmp_path_factory, native_libs):
    """(the case, its index directory, its reads as a FASTQ file)"""
    case = gap_ec_case.case(tmp_path_factory)
    tmp = tmp_path_factory.mktemp("calls_gapped_cli")
    (tmp / "idx").mkdir()
    case.index.save(str(tmp / "idx" / "groot.gidx"))
    fq = tmp / "sample.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(case.reads)))
    return case, str(tmp / "idx"), str(fq)


def _gap_line(log):
    text = open(log).read()
    m = re.search(LINE, text)
    return text, tuple(int(x) for x in m.groups()) if m else None


def test_calls_file_equals_the_definition(cli, sample, tmp_path):
    case, idx_dir, fq = sample
    index, gc = case.index, gap_calls(case)
    with_, without, c = gc.table(), gc.table(gapped=False), gc.counts()
    host.calls_from_table(index, *with_.arrays(), out_path=str(tmp_path / "with.want"))
    host.calls_from_table(index, *without.arrays(), out_path=str(tmp_path / "without.want"))
    want, today = (tmp_path / "with.want").read_bytes(), (tmp_path / "without.want").read_bytes()
    names, P = _names(index), index.view.n_paths
    want_a, today_a = abundance_text(names, P, with_.ecs), abundance_text(names, P, without.ecs)
    assert c["records"] >= 1000 and c["host_records"] >= 100 and want != today and want_a != today_a and today.count(b"\n") > 0
    stats = (c["placements"], c["records"], c["host_records"])
    # (-t 0.9: the threshold the case's records were made with)
    base = [cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.9", "--noBam", "--gapEventSlots", "4096", "--variantMinReads", "1", "--variantMinShare", "0",
            "--abundanceRescued"]
    on = ["--abundanceGapped", "--callsRescued", "--callsGapped", "--callSlots", str(1 << 16)]
    # one ctx, one batch
    a, cf, log, i1, v1 = (str(tmp_path / ("one" + e)) for e in (".a", ".c", ".log", ".indels", ".variants"))
    r = run(base + on + ["--batch", "4096", "--abundance", a, "--calls", cf, "--indels", i1, "--variants", v1, "--log", log, "-g", str(tmp_path / "g1")])
    assert r.returncode == 0, r.stderr
    assert open(cf, "rb").read() == want and open(a, "rb").read() == want_a
    text, m = _gap_line(log)
    assert m == stats and "reopening" not in text, (m, stats)
    assert "calls: %d rescued record(s) counted in the pileup" % c["res_records"] in text and "%d gap-placed read(s) counted in the equivalence classes" % c["gap"] in text
    # two ctxs, small batches, with the support columns and the curve: the host functions over the same table
    a, cf, rf, log = (str(tmp_path / ("ctx2" + e)) for e in (".a", ".c", ".r", ".log"))
    r = run(base + on + ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "97", "--abundance", a, "--calls", cf, "--indels", str(tmp_path / "ctx2.indels"), "--rescueGap", "3",
                         "--bootstraps", "20", "--bootSeed", "3", "--callSupport", "--rarefy", rf, "--rarefySteps", "4", "--rarefyReps", "5", "--rarefySeed", "9", "--log", log,
                         "-g", str(tmp_path / "g2")])
    assert r.returncode == 0, r.stderr
    host.calls_support_from_table(index, *with_.arrays(), out_path=str(tmp_path / "support.want"), n_boot=20, seed=3)
    got = open(cf, "rb").read()
    assert got == (tmp_path / "support.want").read_bytes()
    assert b"\n".join(b"\t".join(ln.split(b"\t")[:7]) for ln in got.splitlines()) + b"\n" == want
    off, ids, cnt, rows, n = with_.arrays()
    host.rarefy_from_ecs(index, off, ids, cnt, str(tmp_path / "rarefy.want"), n_rep=5, n_steps=4, seed=9, tuples=rows, tn=n)
    assert open(rf, "rb").read() == (tmp_path / "rarefy.want").read_bytes() != b""
    assert _gap_line(log)[1] == stats
    assert (tmp_path / "ctx2.indels").read_bytes() == open(i1, "rb").read()
    # through a reopen of the ctx
    a, cf, log = (str(tmp_path / ("grow" + e)) for e in (".a", ".c", ".log"))
    r = run(base + on + ["--maxReadLen", "64", "--batch", "128", "--abundance", a, "--calls", cf, "--indels", str(tmp_path / "grow.indels"), "--log", log, "-g", str(tmp_path / "g3")])
    assert r.returncode == 0, r.stderr
    assert open(cf, "rb").read() == want and open(a, "rb").read() == want_a
    text, m = _gap_line(log)
    assert "reopening the GPU context" in text and m == stats
    # without the flag: the calls file of --callsRescued alone (the gap reads piled up nowhere), and the same indels and variants beside it
    a, cf, log, i0, v0 = (str(tmp_path / ("plain" + e)) for e in (".a", ".c", ".log", ".indels", ".variants"))
    r = run(base + ["--callsRescued", "--callSlots", str(1 << 16), "--batch", "4096", "--abundance", a, "--calls", cf, "--indels", i0, "--variants", v0, "--log", log,
                    "-g", str(tmp_path / "g4")])
    assert r.returncode == 0, r.stderr
    assert open(cf, "rb").read() == today and open(a, "rb").read() == today_a and _gap_line(log)[1] is None
    assert open(i1, "rb").read() == open(i0, "rb").read() != b""
    assert open(v1, "rb").read() == open(v0, "rb").read() != b""
    # and the abundance file of --abundanceGapped without --calls is the one written beside the calls
    a, log = str(tmp_path / "nocalls.a"), str(tmp_path / "nocalls.log")
    r = run(base + ["--abundanceGapped", "--batch", "4096", "--abundance", a, "--indels", str(tmp_path / "nocalls.indels"), "--log", log, "-g", str(tmp_path / "g5")])
    assert r.returncode == 0, r.stderr
    assert open(a, "rb").read() == want_a and (tmp_path / "nocalls.indels").read_bytes() == open(i1, "rb").read()


DEL_AT, DEL_LEN, DEPTH = 300, 3, 5.0


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """(index of the first 8 clusters of arg-annot.90, its directory, the FASTQ, the reads, the path of the allele): the sample's allele is
    the indexed one without bases 300..302; the reads tile it, both strands in turn"""
    tmp = tmp_path_factory.mktemp("calls_gapped_planted")
    with tarfile.open(os.path.join(DATA, "arg-annot.90.tar.gz")) as tf:
        names = sorted(n for n in tf.getnames() if os.path.basename(n).startswith("cluster") and n.endswith(".msa"))[:8]
        tf.extractall(tmp, members=[tf.getmember(n) for n in names])
    index = host.Index.from_msa_files([str(tmp / n) for n in names])
    (tmp / "idx").mkdir()
    index.save(str(tmp / "idx" / "groot.gidx"))
    texts = path_texts(index)
    assert all(t is not None and t[1] == 0 for t in texts)
    p0 = next(p for p, t in enumerate(texts) if len(t[0]) >= 700 and all(c in b"ACGT" for c in t[0]))
    ref = texts[p0][0]
    allele = ref[:DEL_AT] + ref[DEL_AT + DEL_LEN:]
    reads = [allele[s:s + 100] for s in range(0, len(allele) - 100, 3)]
    reads = [_rc(r) if i & 1 else r for i, r in enumerate(reads)]
    fq = tmp / "sample.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    return index, str(tmp / "idx"), str(fq), reads, p0


def _covered(index, table, p, path):
    """per base of path p: covered or not in the calls file the host writes for `table`; and the file's bytes"""
    host.calls_from_table(index, *table.arrays(), out_path=str(path), call_depth=DEPTH)
    name = _names(index)[p].lstrip("*").encode()
    text = path.read_bytes()
    line = next(ln.split(b"\t") for ln in text.splitlines() if ln.split(b"\t")[0] == name)
    return np.concatenate([np.full(int(n), op == b"M") for n, op in re.findall(rb"(\d+)([MD])", line[5])]), text


def test_a_planted_deletion_is_covered_up_to_the_hole(cli, planted, tmp_path):
    index, idx_dir, fq, reads, p0 = planted
    M, G = 2, 3
    seq, off = O.pack_reads(reads)
    r = O.Run(index, 0.99)
    r.batch(seq, off)
    alns = r.alns().astype(device.ALN_DTYPE)
    exact = {}
    for i, p in zip(alns["read_id"].tolist(), alns["ref_id"].tolist()):
        exact.setdefault(i, set()).add(p)
    exact = {i: tuple(sorted(s)) for i, s in exact.items()}
    has = [i in exact for i in range(len(reads))]
    t = Tables(index, M)
    (res, left), rrec = rescued_sets(index, M, reads, has, t), rescued_records(index, M, reads, has, t)
    brute = gap_def.Brute(index, M, g_max=G)
    gap = gap_sets(index, M, G, reads, has, brute.placements)[0]
    kept = {i: gap_def.keep(brute.placements(reads[i]), M, G)[1] for i in left if len(reads[i]) >= A * (M + 3)}
    kept = {i: k for i, k in kept.items() if k}
    grec = {i: rows_of(k, len(reads[i]), lambda p: 0) for i, k in kept.items()}
    ex_rows = exact_rows(index, alns, off)
    with_ = table_of3(exact, ex_rows, res, rrec, gap, grec, kept)
    without = table_of3(exact, ex_rows, res, rrec, {}, {})
    # the CPU first
    cov1, want = _covered(index, with_, p0, tmp_path / "with.want")
    cov0, today = _covered(index, without, p0, tmp_path / "without.want")
    print("planted deletion: %d gap-rescued reads; %d of %d bases at depth >= %g without them, %d with them" % (len(gap), int(cov0.sum()), len(cov0), DEPTH, int(cov1.sum())))
    assert len(gap) >= 10 and int(cov1.sum()) > int(cov0.sum()) and not cov1[DEL_AT:DEL_AT + DEL_LEN].any()
    base = [cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.99", "--noBam", "--callDepth", str(DEPTH), "--batch", "4096", "--abundanceRescued", "--callsRescued",
            "--callSlots", str(1 << 16)]
    got = []
    for tag, flags in (("without", []), ("with", ["--abundanceGapped", "--callsGapped"])):
        a, cf = str(tmp_path / (tag + ".a")), str(tmp_path / (tag + ".c"))
        r = run(base + flags + ["--abundance", a, "--calls", cf, "--indels", str(tmp_path / (tag + ".indels")), "--log", str(tmp_path / (tag + ".log")), "-g", str(tmp_path / ("g" + tag))])
        assert r.returncode == 0, r.stderr
        got.append(open(cf, "rb").read())
    assert got[0] == today and got[1] == want
    name = _names(index)[p0].lstrip("*").encode()
    cigars = [next(ln.split(b"\t")[5] for ln in g.splitlines() if ln.split(b"\t")[0] == name) for g in got]
    cov = [np.concatenate([np.full(int(n), op == b"M") for n, op in re.findall(rb"(\d+)([MD])", c)]) for c in cigars]
    assert int(cov[1].sum()) > int(cov[0].sum()) and not cov[1][DEL_AT:DEL_AT + DEL_LEN].any()
