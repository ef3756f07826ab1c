"""`groot-hip align --rescuedBam r.bam --indels i.tsv --rescuedBamGaps [--gapRecordSlots N]` against the definition: after inflation the
file's records must be, byte for byte, the plain-Python writer (tests/test_rescued_gapped_bam.py, merged_py) applied to BOTH brute forces
-- the rescued records (tests/rescue_records_def.py) and the gapped records (tests/gap_records_def.py), with "has a record" from the CPU
oracle -- whatever the number of contexts, the batch size, or a reopen of the context in the middle of the run.  The reads are those of
tests/test_indels_cli.py, rebuilt here: simulated from an allele of arg-annot.90 with a planted 3-base deletion and a planted 1-base
insertion.  Every line of the indels file has exactly its `reads` records in the BAM whose CIGAR and POS show that event; the main BAM on
stdout, --indels, --variants and --report are those of a run without the switch; and --rescuedBam --indels without the switch writes
the rescued records alone, as it always did."""
import os
import re
import shutil
import tarfile

import numpy as np
import pytest

from bamread import read_bam
from conftest import DATA
from gap_def import Brute
from gap_records_def import records as gap_records
from groot_amd import device, host
from oracle import oracle_py as O
from rescue_def import Tables, _rc, path_texts
from rescue_records_def import records
from test_coverage_cli import run
from test_rescued_bam import aux_of, records_py, split_bam
from test_rescued_gapped_bam import merged_py

pytestmark = pytest.mark.gpu
AT_DEL, AT_INS, G = 300, 500, 3


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """the sample of tests/test_indels_cli.py: (index of the first 24 clusters of arg-annot.90, its directory, the FASTQ, the reads)"""
    tmp = tmp_path_factory.mktemp("rescued_gaps_cli")
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
    ins = bytes([next(c for c in b"ACGT" if c != ref[AT_INS - 1] and c != ref[AT_INS])])
    allele = ref[:AT_DEL] + ref[AT_DEL + 3:AT_INS] + ins + ref[AT_INS:]
    reads = [allele[s:s + 100] for s in range(0, len(allele) - 100, 3)]
    for p in range(0, len(texts), 3):
        t = texts[p][0]
        for k in range(6):
            s = int(rng.integers(0, len(t) - 100))
            r = bytearray(t[s:s + 100].replace(b"N", b"A"))
            for at in rng.choice(100, 1 + k % 3, replace=False):
                r[at] = int(rng.choice([c for c in b"ACGT" if c != r[at]]))
            reads.append(bytes(r))
    reads += [allele[280:350], allele[250:300] + b"N" + allele[301:350]]
    reads = [_rc(r) if i & 1 else r for i, r in enumerate(reads)]
    fq = tmp / "sample.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    return index, str(tmp / "idx"), str(fq), reads


def _definitions(index, reads, M=2):
    """(rescued records, gapped records, the texts) of the whole sample as one batch"""
    seq, off = O.pack_reads(reads)
    run_ = O.Run(index, 0.99)
    run_.batch(seq, off)
    has = np.bincount(run_.alns().astype(device.ALN_DTYPE)["read_id"].astype(np.int64), minlength=len(reads)) > 0
    t = Tables(index, M)
    return records(index, M, reads, has, t), gap_records(index, M, G, Brute(index, M, g_max=G), reads, has), t.texts


def _events_shown(bam):
    """{(ref_id, 1-based position of the base before the gap, type, bases): records} over the gapped records of a BAM, from CIGAR, POS,
    SEQ (an insertion's bases) and MD (a deletion's)"""
    out = {}
    for r, a in zip(read_bam(bam)[2], aux_of(split_bam(bam)[2])):
        m = re.fullmatch(r"(\d+)M(\d+)([ID])(\d+)M", r["cigar"])
        if not m:
            assert re.fullmatch(r"\d+M", r["cigar"])
            continue
        k, g, typ = int(m.group(1)), int(m.group(2)), m.group(3)
        bases = r["seq"][k:k + g] if typ == "I" else re.search(r"\^([ACGTN]+)", a[4]["MD"]).group(1)
        assert len(bases) == g and a[4]["NM"] >= g
        key = (r["ref_id"], r["pos"] + k, "INS" if typ == "I" else "DEL", bases)
        out[key] = out.get(key, 0) + 1
    return out


def test_rescued_bam_with_gaps_equals_the_definitions(cli, sample, tmp_path):
    index, idx_dir, fq, reads = sample
    rec, grec, texts = _definitions(index, reads)
    # (two reads in three of the reads with sequencing errors have at most two: rescued; some fifteen reads cross either planted event)
    assert len(rec) >= 20 and len(grec) >= 30 and set(grec["type"].tolist()) == {0, 1} and set(grec["strand"].tolist()) == {0, 1}
    assert not set(rec["read"].tolist()) & set(grec["read"].tolist())
    names, quals = [b"r%d" % i for i in range(len(reads))], [b"I" * len(r) for r in reads]
    plain = [(int(r["read"]), int(r["path"]), int(r["pos"]), int(r["strand"]), int(r["d"]), tuple(int(x) for x in r["mm"])) for r in rec]
    gplain = [(int(r["read"]), int(r["path"]), int(r["pos"]), int(r["k"]), int(r["strand"]), int(r["d"]), int(r["type"]), int(r["g"]), tuple(int(x) for x in r["mm"]))
              for r in grec]
    ref_base = lambda p, y: texts[p][0][y - texts[p][1]]
    want = merged_py(names, reads, quals, plain, gplain, ref_base)
    parent = records_py(names, reads, quals, plain, ref_base)            # what --rescuedBam --indels writes without the switch
    base = [cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.99", "--variantMinReads", "1", "--variantMinShare", "0"]
    outs = {}
    for tag, extra in (("one", ["--batch", "4096"]), ("ctx2", ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "97"]), ("grow", ["--maxReadLen", "64", "--batch", "128"]),
                       ("noswitch", ["--batch", "4096"])):
        f = {e: str(tmp_path / (tag + "." + e)) for e in ("rbam", "indels", "tsv", "report", "log", "bam")}
        flags = ["--indels", f["indels"], "--rescueGap", str(G), "--variants", f["tsv"], "--report", f["report"], "--covCutoff", "0.5", "--log", f["log"],
                 "-g", str(tmp_path / ("g" + tag)), "--rescuedBam", f["rbam"]]
        r = run(base + extra + flags + (["--rescuedBamGaps"] if tag != "noswitch" else []))
        assert r.returncode == 0, r.stderr
        open(f["bam"], "wb").write(r.stdout)                             # the main BAM goes to stdout
        outs[tag] = (read_bam(f["bam"])[1:], open(f["indels"], "rb").read(), open(f["tsv"], "rb").read(), open(f["report"], "rb").read())
        got = split_bam(f["rbam"])[2]
        log = open(f["log"]).read()
        if tag == "noswitch":
            assert got == parent and "gap-placed reads" not in log
            continue
        assert got == want, tag
        n_reads = len(np.unique(rec["read"])) + len(np.unique(grec["read"]))
        assert "rescued reads: %d record(s) of %d read(s) written to %s (up to 2 substitution(s))" % (len(rec) + len(grec), n_reads, f["rbam"]) in log, log
        assert "gap-placed reads: %d record(s) of %d read(s) among them (one gap of up to 3 base(s))" % (len(grec), len(np.unique(grec["read"]))) in log, log
    assert "reopening the GPU context" in open(str(tmp_path / "grow.log")).read() and "reopening" not in open(str(tmp_path / "one.log")).read()
    # the main BAM, the indels, the variants and the report are those of the run without the switch
    assert outs["one"] == outs["ctx2"] == outs["grow"] == outs["noswitch"] and len(outs["one"][0][1]) > 50 and all(outs["one"][1:])
    # every line of the indels file: reads = the records whose CIGAR and POS show that event
    o = index.arrays["path_name_off"].astype(np.int64)
    path_of = {index.arrays["path_names"].tobytes()[a:b].lstrip(b"*"): p for p, (a, b) in enumerate(zip(o, o[1:]))}
    shown = _events_shown(str(tmp_path / "one.rbam"))
    lines = [ln.split(b"\t") for ln in outs["one"][1].splitlines()]
    assert len(lines) >= 2 and {ln[2] for ln in lines} == {b"DEL", b"INS"}
    for ln in lines:
        assert shown.pop((path_of[ln[0]], int(ln[1]), ln[2].decode(), ln[4].decode()), 0) == int(ln[5]), ln
    assert not shown                                                     # ... and no record shows another event
    # an ordinary BAM: `report` reads it
    shutil.copy(str(tmp_path / "one.rbam"), str(tmp_path / "gapped.bam"))
    r = run([cli, "report", "--bamFile", str(tmp_path / "gapped.bam"), "-c", "0.5", "--log", str(tmp_path / "rep.log")])
    # (it runs; the hundred records cover less than half of any gene, so whether a line comes out is the cutoff's business)
    assert r.returncode == 0 and r.stderr == b"" and all(ln.count(b"\t") == 3 for ln in r.stdout.splitlines()), (r.stdout, r.stderr)


def test_a_run_without_room_fails_and_names_the_flag(cli, sample, tmp_path):
    index, idx_dir, fq, reads = sample
    r = run([cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.99", "--batch", "4096", "--rescuedBam", str(tmp_path / "r.bam"), "--indels", str(tmp_path / "i.tsv"),
             "--rescuedBamGaps", "--gapRecordSlots", "10", "--bam", str(tmp_path / "m.bam"), "--log", str(tmp_path / "l.log"), "-g", str(tmp_path / "g")])
    assert r.returncode == 1 and b"slots_per_batch" in r.stderr and b"room for 10" in r.stderr and b"--gapRecordSlots" in r.stderr, r.stderr
