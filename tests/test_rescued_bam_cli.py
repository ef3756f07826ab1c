"""`groot-hip align --rescuedBam r.bam [--rescue M] [--rescuedBamSlots N]` against the definition: after inflation the file's records
must be, byte for byte, the plain-Python writer (tests/test_rescued_bam.py, records_py) applied to the brute force of the rescued records
(tests/rescue_records_def.py) with "has a record" from the CPU oracle -- whatever the number of contexts, the batch size, or a reopen of
the context in the middle of the run.  The reads are those of tests/test_variants_cli.py: simulated from an allele of arg-annot.90 with
one planted SNP.  The main BAM, --report and --variants of the same run are those of a run without the flag; every line of the variants
file has exactly its alt_reads records in the new BAM whose MD shows that base at that position; `report` reads the new file."""
import re
import shutil

import numpy as np
import pytest

from bamread import read_bam
from groot_amd import device
from oracle import oracle_py as O
from rescue_def import Tables
from rescue_records_def import records
from test_coverage_cli import run
from test_rescued_bam import aux_of, records_py, split_bam
from test_variants_cli import cli, sample  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _definition(index, reads, M):
    seq, off = O.pack_reads(reads)
    run_ = O.Run(index, 0.99)
    run_.batch(seq, off)
    has = np.bincount(run_.alns().astype(device.ALN_DTYPE)["read_id"].astype(np.int64), minlength=len(reads)) > 0
    t = Tables(index, M)
    return records(index, M, reads, has, t), t


def _shown(bam):
    """{(ref_id, 0-based path position, the read's base there): records} over the mismatches the MD strings of a BAM show"""
    out = {}
    recs = read_bam(bam)[2]
    for r, (name, ref_id, pos, flag, tags) in zip(recs, aux_of(split_bam(bam)[2])):
        at, num = 0, ""
        for ch in tags["MD"]:
            if ch.isdigit():
                num += ch
                continue
            at += int(num)
            out[(ref_id, pos + at, r["seq"][at])] = out.get((ref_id, pos + at, r["seq"][at]), 0) + 1
            at, num = at + 1, ""
        assert at + int(num) == len(r["seq"]) and tags["NM"] == sum(c.isalpha() for c in tags["MD"])
    return out


def test_rescued_bam_equals_the_definition(cli, sample, tmp_path):
    index, idx_dir, fq, reads, p0, ref, alt = sample
    rec, t = _definition(index, reads, 2)
    n_reads = len(np.unique(rec["read"]))
    assert len(rec) > n_reads > 100 and {1, 2} <= set(rec["d"].tolist()) and set(rec["strand"].tolist()) == {0, 1}
    names, quals = [b"r%d" % i for i in range(len(reads))], [b"I" * len(r) for r in reads]
    plain = [(int(r["read"]), int(r["path"]), int(r["pos"]), int(r["strand"]), int(r["d"]), tuple(int(x) for x in r["mm"])) for r in rec]
    want = records_py(names, reads, quals, plain, lambda p, y: t.texts[p][0][y - t.texts[p][1]])
    base = [cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.99"]
    outs = {}
    for tag, extra in (("one", ["--batch", "4096"]), ("ctx2", ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "97"]), ("grow", ["--maxReadLen", "64", "--batch", "128"]),
                       ("plain", ["--batch", "4096"])):
        f = {e: str(tmp_path / (tag + "." + e)) for e in ("rbam", "bam", "tsv", "report", "log")}
        flags = ["--variants", f["tsv"], "--report", f["report"], "--covCutoff", "0.5", "--bam", f["bam"], "--log", f["log"], "-g", str(tmp_path / ("g" + tag))]
        r = run(base + extra + flags + (["--rescuedBam", f["rbam"]] if tag != "plain" else []))
        assert r.returncode == 0 and r.stdout == b"", r.stderr
        outs[tag] = (read_bam(f["bam"])[1:], open(f["tsv"], "rb").read(), open(f["report"], "rb").read())
        if tag == "plain":
            continue
        text, refs, got = split_bam(f["rbam"])
        assert got == want, tag
        undated = lambda h: re.sub(rb"DT:[^\t]*", b"", h)
        assert len(refs) == index.view.n_paths and undated(text) == undated(split_bam(f["bam"])[0])      # the header groot_bam_open writes, as the main BAM has it
        ln = next(x for x in open(f["log"]) if "rescued reads: " in x)
        assert "rescued reads: %d record(s) of %d read(s) written to %s (up to 2 substitution(s))" % (len(rec), n_reads, f["rbam"]) in ln, ln
    assert "reopening the GPU context" in open(str(tmp_path / "grow.log")).read() and "reopening" not in open(str(tmp_path / "one.log")).read()
    # the main BAM, the variants file and the report are those of the run without the flag
    assert outs["one"] == outs["ctx2"] == outs["grow"] == outs["plain"] and len(outs["plain"][0][1]) > 50 and outs["plain"][1] and outs["plain"][2]
    # every line of the variants file: alt_reads = the records of the new BAM whose MD shows that base at that position
    o = index.arrays["path_name_off"].astype(np.int64)
    path_of = {index.arrays["path_names"].tobytes()[a:b].lstrip(b"*"): p for p, (a, b) in enumerate(zip(o, o[1:]))}
    shown = _shown(str(tmp_path / "one.rbam"))
    lines = [ln.split(b"\t") for ln in outs["one"][1].splitlines()]
    assert len(lines) >= 1 and any(path_of[ln[0]] == p0 and int(ln[1]) == 301 and ln[3] == alt for ln in lines)      # the planted SNP among them
    for ln in lines:
        assert shown.get((path_of[ln[0]], int(ln[1]) - 1, ln[3].decode()), 0) == int(ln[4]), ln
    # an ordinary BAM: `report` reads it
    shutil.copy(str(tmp_path / "one.rbam"), str(tmp_path / "rescued.bam"))                                          # (report wants a .bam extension)
    r = run([cli, "report", "--bamFile", str(tmp_path / "rescued.bam"), "-c", "0.5", "--log", str(tmp_path / "rep.log")])
    assert r.returncode == 0 and r.stdout.count(b"\n") >= 1 and all(ln.count(b"\t") == 3 for ln in r.stdout.splitlines()), (r.stdout, r.stderr)


def test_a_run_without_room_fails_and_says_so(cli, sample, tmp_path):
    index, idx_dir, fq, reads, p0, ref, alt = sample
    r = run([cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.99", "--batch", "4096", "--rescuedBam", str(tmp_path / "r.bam"), "--rescuedBamSlots", "10",
             "--bam", str(tmp_path / "m.bam"), "--log", str(tmp_path / "l.log"), "-g", str(tmp_path / "g")])
    assert r.returncode == 1 and b"slots_per_batch" in r.stderr and b"room for 10" in r.stderr, r.stderr
