"""`groot-hip align --variants v.tsv [--rescue M] [--variantMinReads N] [--variantMinShare S]` against the definition: the file must be, byte
for byte, the plain-Python writer (tests/test_variants.py, variants_py) applied to the brute force of the definition over all (path,
strand, x) (tests/rescue_def.py, Tables) with "has a record" and the exact depth from the CPU oracle's records -- whatever the number of
contexts, the batch size, or a reopen of the context in the middle of the run.  The reads are simulated from an allele of arg-annot.90
with one planted SNP: its line must be in the file, and the --report of the same run is the report of a run without --variants."""
import os
import tarfile

import numpy as np
import pytest

from bamread import read_bam
from conftest import DATA
from groot_amd import device, host
from oracle import oracle_py as O
from rescue_def import Tables, _rc, path_texts
from test_coverage import expand_coverage
from test_coverage_cli import run
from test_variants import variants_py

pytestmark = pytest.mark.gpu
SNP = 300


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """(index of the first 24 clusters of arg-annot.90, its directory, the FASTQ, the reads, path and alt base of the planted SNP)"""
    tmp = tmp_path_factory.mktemp("variants_cli")
    with tarfile.open(os.path.join(DATA, "arg-annot.90.tar.gz")) as tf:
        names = sorted(n for n in tf.getnames() if os.path.basename(n).startswith("cluster") and n.endswith(".msa"))[:24]
        tf.extractall(tmp, members=[tf.getmember(n) for n in names])
    index = host.Index.from_msa_files([str(tmp / n) for n in names])
    (tmp / "idx").mkdir()
    index.save(str(tmp / "idx" / "groot.gidx"))
    texts = path_texts(index)
    assert all(t is not None and t[1] == 0 for t in texts)
    rng = np.random.default_rng(21)
    p0 = next(p for p, t in enumerate(texts) if len(t[0]) >= 700 and all(c in b"ACGT" for c in t[0]))
    ref = texts[p0][0]
    alt = bytes([next(c for c in b"ACGT" if c != ref[SNP])])
    allele = ref[:SNP] + alt + ref[SNP + 1:]                          # the sample's allele: one substitution away from the indexed one
    reads = [allele[s:s + 100] for s in range(0, len(allele) - 100, 3)]
    for p in range(0, len(texts), 3):                                 # sequencing errors on other ARGs: 1, 2 and 3 per read
        t = texts[p][0]
        for k in range(12):
            s = int(rng.integers(0, len(t) - 100))
            r = bytearray(t[s:s + 100].replace(b"N", b"A"))
            for at in rng.choice(100, 1 + k % 3, replace=False):
                r[at] = int(rng.choice([c for c in b"ACGT" if c != r[at]]))
            reads.append(bytes(r))
    reads += [allele[200:240], allele[250:300] + b"N" + allele[301:350]]      # too short, not A/C/G/T
    reads = [_rc(r) if i & 1 else r for i, r in enumerate(reads)]
    fq = tmp / "sample.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    return index, str(tmp / "idx"), str(fq), reads, p0, ref[SNP:SNP + 1], alt


def _expected(index, reads, M, min_reads, min_share):
    seq, off = O.pack_reads(reads)
    run_ = O.Run(index, 0.99)
    run_.batch(seq, off)
    alns = run_.alns().astype(device.ALN_DTYPE)
    has = np.bincount(alns["read_id"].astype(np.int64), minlength=len(reads)) > 0
    t = Tables(index, M)
    t.add(reads, has)
    exact = expand_coverage(index, alns, off)[1]
    o = index.arrays["path_name_off"].astype(np.int64)
    names = [index.arrays["path_names"].tobytes()[a:b] for a, b in zip(o, o[1:])]
    return variants_py(names, [x[0] for x in t.texts], t.depth(), t.alt.reshape(-1), exact, min_reads, min_share), t, int(has.sum())


def test_variants_file_equals_the_definition(cli, sample, tmp_path):
    index, idx_dir, fq, reads, p0, ref, alt = sample
    want, t, mapped = _expected(index, reads, 2, 2, 0.1)
    name = index.path_name(p0).lstrip("*").encode()
    line = next(ln for ln in want.split(b"\n") if ln.startswith(b"%s\t%d\t%s\t%s\t" % (name, SNP + 1, ref, alt)))      # the planted SNP
    print(line.decode(), t.stats, "reads", len(reads), "with a record", mapped)
    assert int(line.split(b"\t")[4]) >= 20 and t.stats["rescued"] > 100 and t.stats["too_short"] == 1 and t.stats["non_acgt"] == 1 and mapped > 50
    assert t.stats["rescued"] < t.stats["candidates"]                 # (three errors are one too many for M = 2)
    base = [cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.99"]
    outs = {}
    for tag, extra in (("one", ["--batch", "4096"]), ("ctx2", ["--gpus", "1", "--ctxPerGpu", "2", "--batch", "97"]), ("grow", ["--maxReadLen", "64", "--batch", "128"])):
        v, rep, log = (str(tmp_path / (tag + e)) for e in (".tsv", ".report", ".log"))
        r = run(base + extra + ["--variants", v, "--report", rep, "--covCutoff", "0.5", "--noBam", "--log", log, "-g", str(tmp_path / ("g" + tag))])
        assert r.returncode == 0, r.stderr
        assert open(v, "rb").read() == want, tag
        ln = next(x for x in open(log) if "variants: " in x)
        assert ("variants: %d unaligned read(s) tried with up to 2 substitution(s): %d rescued (%d without one) in %d placement(s); left out: 1 too short, 1 not A/C/G/T; "
                "%d line(s) written" % (t.stats["candidates"], t.stats["rescued"], t.stats["exact"], t.stats["placements"], want.count(b"\n"))) in ln, ln
        outs[tag] = open(rep, "rb").read()
    assert "reopening the GPU context" in open(str(tmp_path / "grow.log")).read() and "reopening" not in open(str(tmp_path / "one.log")).read()
    # the report beside it is the report of a run without --variants
    rep = str(tmp_path / "plain.report")
    r = run(base + ["--batch", "4096", "--report", rep, "--covCutoff", "0.5", "--noBam", "--log", str(tmp_path / "plain.log"), "-g", str(tmp_path / "gplain")])
    assert r.returncode == 0, r.stderr
    assert open(rep, "rb").read() == outs["one"] == outs["ctx2"] == outs["grow"] != b""


def test_thresholds_and_a_bam_beside_it(cli, sample, tmp_path):
    """--rescue 1 with other thresholds, and without --report: coverage is counted for the exact depth all the same, the BAM's records are those of a run without it"""
    index, idx_dir, fq, reads, p0, ref, alt = sample
    want, t, _ = _expected(index, reads, 1, 1, 0.0)                  # (every single sequencing error is a line now, those of reads with two are not)
    assert want.count(b"\n") > 20
    base = [cli, "align", "-i", idx_dir, "-f", fq, "-p", "4", "-t", "0.99", "--batch", "500"]
    v, bam, plain = str(tmp_path / "v.tsv"), str(tmp_path / "v.bam"), str(tmp_path / "plain.bam")
    r = run(base + ["--variants", v, "--rescue", "1", "--variantMinReads", "1", "--variantMinShare", "0", "--bam", bam, "--log", str(tmp_path / "v.log"), "-g", str(tmp_path / "gv")])
    assert r.returncode == 0, r.stderr
    assert open(v, "rb").read() == want
    r = run(base + ["--bam", plain, "--log", str(tmp_path / "p.log"), "-g", str(tmp_path / "gp")])
    assert r.returncode == 0, r.stderr
    assert read_bam(bam)[2] == read_bam(plain)[2] and len(read_bam(bam)[2]) > 50
