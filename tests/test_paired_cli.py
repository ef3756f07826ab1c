"""`groot-hip align --paired -f R1,R2` / `--interleaved -f il.fq` and the reader behind them (groot_reads_open_paired).

The definition, quoted from include/groot_hip.h and DESIGN.md section 12:

    With pairing on, reads 2i and 2i+1 of a batch are the mates of fragment i.  The index is batch-relative: read_id - first_read_id;
    first_read_id may be odd.  Let A = S(r_2i) and B = S(r_2i+1), S(r) exactly as above.
      joined:  A and B intersect.  The fragment is one unit with the set A n B.
      split:   A and B are non-empty and do not intersect.  The fragment is two units, A and B, exactly as without pairing (mates on
               different genes are evidence for both).
      single:  exactly one of A, B is non-empty.  The fragment is one unit with that set.
      none:    both are empty.  There is no unit.

The expected --abundance and --sharedReads files come from the records of an UNPAIRED run's BAM on the interleaved file, read through
tests/bamread.py and grouped by QNAME stem, with the restatement above in plain Python."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from bamread import read_bam
from conftest import REPO
from groot_amd import host, synth
from test_abundance import _names, abundance_text
from test_path_pass import _COMP
from test_shared_reads import shared_rows


@pytest.fixture(scope="module")
def cli(hip_lib):
    import __graft_entry__ as g

    return g.build_cli()


def run(cmd):
    return subprocess.run(cmd, cwd=REPO, capture_output=True, timeout=600)


def _fragments(index, n, seed, L=100):
    """[(mate 1, mate 2)]: mate 1 at offset x of a path text, mate 2 at x + d on the other strand; every 10th a chimera of two paths,
    every 13th with one mate damaged in the middle, every 29th noise"""
    cat, off, lens = synth.reference_sequences(index)
    rng = np.random.default_rng(seed)
    ok = np.flatnonzero(lens >= 3 * L)
    out = []

    def piece(p, x):
        return bytes(cat[off[p] + x:off[p] + x + L])

    for i in range(n):
        p = int(rng.choice(ok))
        x = int(rng.integers(0, lens[p] - 2 * L))
        d = int(rng.integers(20, min(400, lens[p] - L - x) + 1))
        m1, m2 = piece(p, x), piece(p, x + d)
        if i % 10 == 9:
            q = int(rng.choice(ok))
            m2 = piece(q, int(rng.integers(0, lens[q] - L)))
        if i % 13 == 12:
            bad = bytearray(m1 if i & 1 else m2)
            for k in (L // 3, L // 2, 2 * L // 3):
                bad[k] = _COMP[bad[k]]
            m1, m2 = (bytes(bad), m2) if i & 1 else (m1, bytes(bad))
        if i % 29 == 28:
            m1, m2 = ("".join(rng.choice(list("ACGT"), L)).encode() for _ in range(2))
        out.append((m1, m2.translate(_COMP)[::-1]))
    return out


def _write(tmp, frags, gz=False, names=None):
    """R1, R2 and the interleaved file, names f<i>/1 and f<i>/2"""
    op = (lambda p: gzip.open(p, "wb")) if gz else (lambda p: open(p, "wb"))
    ext = ".fq.gz" if gz else ".fq"
    r1, r2, il = (str(tmp / (n + ext)) for n in ("R1", "R2", "il"))
    with op(r1) as f1, op(r2) as f2, op(il) as fi:
        for i, (a, b) in enumerate(frags):
            n1, n2 = names(i) if names else (b"f%d/1" % i, b"f%d/2" % i)
            x = b"@" + n1 + b"\n" + a + b"\n+\n" + b"I" * len(a) + b"\n"
            y = b"@" + n2 + b" second mate\n" + b + b"\n+\n" + b"H" * len(b) + b"\n"
            f1.write(x), f2.write(y), fi.write(x + y)
    return r1, r2, il


# ---- the reader, no GPU -------------------------------------------------------------------------------------------------------

def _batches(**kw):
    r = host.ParallelReads(**kw)
    out = [(b["n"], b["names"], b["seqs"], b["quals"], b["packed"].tobytes(), b["seq_len"].tolist()) for b in r.batches()]
    r.close()
    return out


def _toy(n, L=40, seed=3, vary=False):
    rng = np.random.default_rng(seed)
    seq = lambda: "".join(rng.choice(list("ACGTN"), int(rng.integers(20, 60)) if vary else L)).encode()
    return [(seq(), seq()) for _ in range(n)]


@pytest.mark.parametrize("gz", [False, True])
def test_two_lists_and_one_interleaved_stream_give_the_same_batches(native_libs, tmp_path, gz):
    """mates interleaved (2i from the first list, 2i+1 from the second), n_reads even, an odd max_batch_reads rounded down, a fragment
    never cut by max_batch_bases; text blocks far smaller than the files, so that fragments straddle block ends in both streams"""
    frags = _toy(700, vary=True)
    r1, r2, il = _write(tmp_path, frags, gz)
    want = [(a, b) for a, b in frags]
    for kw in ({"max_batch_reads": 101}, {"max_batch_reads": 64, "max_batch_bases": 1500}, {}):
        # (a batch never spans two text blocks, in any mode: with blocks this small the block ends cut the batches too, at different
        # fragments in the two modes -- so the batches are compared with the default block, the contents with the small ones)
        assert _batches(files=[il], interleaved=True, threads=3, **kw) == _batches(files=[r1], mates=[r2], threads=3, **kw)
        got2 = _batches(files=[r1], mates=[r2], block_bytes=4096, threads=3, **kw)
        got1 = _batches(files=[il], interleaved=True, block_bytes=4096, threads=3, **kw)
        plain = _batches(files=[il], block_bytes=1 << 20, threads=1, max_batch_reads=1 << 20)
        assert [x for b in got1 for x in zip(*b[1:4])] == [x for b in got2 for x in zip(*b[1:4])] and all(b[0] % 2 == 0 and b[0] > 0 for b in got1)
        assert all(b[0] % 2 == 0 and b[0] > 0 for b in got2)
        if "max_batch_reads" in kw:
            assert max(b[0] for b in got2) <= kw["max_batch_reads"] & ~1
        if "max_batch_bases" in kw:
            assert all(sum(b[5]) <= kw["max_batch_bases"] for b in got2) and len(got2) > 700 * 2 // 64
        seqs = [s for b in got2 for s in b[2]]
        assert seqs == [m for f in want for m in f] == [s for b in plain for s in b[2]]
        assert [n for b in got2 for n in b[1]] == [n for b in plain for n in b[1]]
        assert [q for b in got2 for q in b[3]] == [q for b in plain for q in b[3]]
        # the packed bases are in read order: what the unpaired reader packs for the same reads
        if not kw:
            whole = _batches(files=[r1], mates=[r2], threads=3)
            assert len(whole) == len(plain) == 1 and whole[0][4] == plain[0][4] and whole[0][5] == plain[0][5]


def test_file_pairs_are_taken_two_at_a_time(native_libs, tmp_path):
    a, b = _toy(150, seed=5), _toy(90, seed=6)
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    a1, a2, _ = _write(tmp_path / "a", a)
    b1, b2, _ = _write(tmp_path / "b", b, names=lambda i: (b"g%d" % i, b"g%d" % i))      # names without /1 /2 agree as they are
    got = _batches(files=[a1, b1], mates=[a2, b2], block_bytes=2048)
    assert [s for x in got for s in x[2]] == [m for f in a + b for m in f]
    assert all(x[0] % 2 == 0 for x in got)


def test_reader_errors(native_libs, tmp_path):
    frags = _toy(300)
    (tmp_path / "ok").mkdir(), (tmp_path / "bad").mkdir(), (tmp_path / "slash").mkdir()
    r1, r2, il = _write(tmp_path / "ok", frags)
    # a mismatch names the 1-based fragment number and both names
    b1, b2, bil = _write(tmp_path / "bad", frags, names=lambda i: (b"f%d/1" % i, b"f%d/2" % (i if i != 211 else 9999)))
    for kw in ({"files": [b1], "mates": [b2]}, {"files": [bil], "interleaved": True}):
        with pytest.raises(host.GrootError) as e:
            _batches(block_bytes=4096, **kw)
        assert e.value.code == -3 and "fragment 212" in str(e.value) and "f211/1" in str(e.value) and "f9999/2" in str(e.value), str(e.value)
    # only a trailing /1 or /2 is removed, and the name ends at the first whitespace
    s1, s2, _ = _write(tmp_path / "slash", frags[:4], names=lambda i: (b"f%d/1x" % i, b"f%d/2x" % i))
    with pytest.raises(host.GrootError) as e:
        _batches(files=[s1], mates=[s2])
    assert "fragment 1" in str(e.value)
    # a list that ends before its partner
    short = str(tmp_path / "short.fq")
    open(short, "wb").write(b"".join(open(r2, "rb").read().split(b"\n@")[0:1]) + b"\n")
    lines = open(r2, "rb").read().split(b"\n")
    open(short, "wb").write(b"\n".join(lines[:4 * 250]) + b"\n")
    for kw in ({"files": [r1], "mates": [short]}, {"files": [short], "mates": [r1]}):
        with pytest.raises(host.GrootError) as e:
            _batches(block_bytes=4096, **kw)
        assert e.value.code == -3 and "partner" in str(e.value), str(e.value)
    # an interleaved stream with an odd number of records
    odd = str(tmp_path / "odd.fq")
    lines = open(il, "rb").read().split(b"\n")
    open(odd, "wb").write(b"\n".join(lines[:4 * 401]) + b"\n")
    with pytest.raises(host.GrootError) as e:
        _batches(files=[odd], interleaved=True, block_bytes=4096)
    assert e.value.code == -3 and "odd number" in str(e.value)
    with pytest.raises(host.GrootError):
        _batches(files=[r1, r1], mates=[r2])


def test_refusals(cli, tmp_path):
    """flag combinations that are refused before anything is opened"""
    r1, r2, il = _write(tmp_path, _toy(4))
    base = [cli, "align", "-i", str(tmp_path), "--log", str(tmp_path / "x.log")]
    ab = ["--abundance", str(tmp_path / "a.tsv"), "--noBam"]
    r = run(base + ["--paired", "-f", r1 + "," + r2])
    assert r.returncode != 0 and b"--paired" in r.stderr and b"--sharedReads" in r.stderr and b"--abundance" in r.stderr
    r = run(base + ["--interleaved", "-f", il, "--report", str(tmp_path / "r.tsv")])
    assert r.returncode != 0 and b"--interleaved" in r.stderr and b"--abundance" in r.stderr
    r = run(base + ["--paired", "-f", ",".join([r1, r2, il])] + ab)
    assert r.returncode != 0 and b"two at a time" in r.stderr and b"3 file(s)" in r.stderr
    r = run(base + ["--paired", "--interleaved", "-f", r1 + "," + r2] + ab)
    assert r.returncode != 0 and b"--paired and --interleaved" in r.stderr
    assert not os.path.exists(tmp_path / "a.tsv") and not os.path.exists(tmp_path / "x.log")
    for flag in ("--paired", "--interleaved"):
        r = run([cli, "report", flag, "--bamFile", str(tmp_path / "none.bam"), "--abundance", str(tmp_path / "a.tsv"), "--log", str(tmp_path / "r.log")])
        assert r.returncode != 0 and b"mate flags" in r.stderr and b"align --paired" in r.stderr


# ---- the command line on the GPU ------------------------------------------------------------------------------------------------

def _units_of_bam(index, bam):
    """per QNAME the set of references; fragments by QNAME stem (f<i>/1, f<i>/2) -> the unit sets, by the definition"""
    _, refs, recs = read_bam(bam)
    assert [n for n, _ in refs] == _names(index)
    sets = {}
    for r in recs:
        sets.setdefault(r["name"].split()[0], set()).add(r["ref_id"])
    stems = sorted({q.rsplit("/", 1)[0] for q in sets}, key=lambda s: int(s[1:]))
    units, cls = [], {"joined": 0, "split": 0, "single": 0}
    for s in stems:
        a, b = sets.get(s + "/1", set()), sets.get(s + "/2", set())
        if a & b:
            units.append(tuple(sorted(a & b)))
            cls["joined"] += 1
        elif a and b:
            units += [tuple(sorted(a)), tuple(sorted(b))]
            cls["split"] += 1
        else:
            units.append(tuple(sorted(a or b)))
            cls["single"] += 1
    return units, cls


@pytest.mark.gpu
def test_paired_interleaved_and_sharded_runs_write_the_expected_files(cli, argannot_index, tmp_path):
    index = argannot_index
    idx_dir = tmp_path / "idx"
    idx_dir.mkdir()
    index.save(str(idx_dir / "groot.gidx"))
    frags = _fragments(index, 1500, 77)
    r1, r2, il = _write(tmp_path, frags)
    base = [cli, "align", "-i", str(idx_dir), "-p", "4", "--batch", "700"]

    def outs(tag):
        return {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in ("ab", "sh", "rep", "log", "bam")}

    def go(tag, extra, bam=True):
        o = outs(tag)
        r = run(base + extra + ["--abundance", o["ab"], "--report", o["rep"], "--sharedReads", o["sh"], "--log", o["log"], "-g", str(tmp_path / ("g" + tag))]
                + (["--bam", o["bam"]] if bam else ["--noBam"]))
        assert r.returncode == 0, r.stderr
        return o

    plain = go("plain", ["-f", il])
    units, cls = _units_of_bam(index, plain["bam"])
    assert cls["joined"] > 800 and cls["split"] >= 50 and cls["single"] >= 50, cls
    ecs = {}
    for u in units:
        ecs[u] = ecs.get(u, 0) + 1
    want_ab = abundance_text(_names(index), index.view.n_paths, sorted(ecs.items()))
    pairs = {}
    for u, c in ecs.items():
        for i, a in enumerate(u):
            for b in u[i:]:
                pairs[(a, b)] = pairs.get((a, b), 0) + c
    rep_rows = [ln.split("\t") for ln in open(plain["rep"]).read().splitlines()]
    want_sh = "".join("%s\t%s\t%d\n" % row for row in shared_rows(index, rep_rows, pairs)).encode()
    assert want_ab.count(b"\n") > 5 and want_sh.count(b"\n") > 5
    assert open(plain["ab"], "rb").read() != want_ab                           # the per-mate file differs: the input tells the two apart

    paired = go("paired", ["--paired", "-f", r1 + "," + r2])
    inter = go("inter", ["--interleaved", "-f", il], bam=False)
    shard = go("shard", ["--paired", "-f", r1 + "," + r2, "--ctxPerGpu", "2", "--batch", "1001"], bam=False)
    for o in (paired, inter, shard):
        assert open(o["ab"], "rb").read() == want_ab
        assert open(o["sh"], "rb").read() == want_sh
        assert open(o["rep"], "rb").read() == open(plain["rep"], "rb").read()      # coverage does not depend on pairing
        log = open(o["log"]).read()
        assert "paired-end input: %d fragment(s), %d joined, %d split, %d single" % (len(frags), cls["joined"], cls["split"], cls["single"]) in log, log
    # the mates as ordinary records, interleaved: the BAM of the unpaired run (but for the second its @RG line was stamped with)
    inflate = lambda p: re.sub(rb"\tDT:[0-9TZ:-]+", b"\tDT:-", gzip.open(p, "rb").read())
    assert inflate(paired["bam"]) == inflate(plain["bam"])

    boot = outs("boot")
    r = run(base + ["--paired", "-f", r1 + "," + r2, "--abundance", boot["ab"], "--bootstraps", "20", "--noBam", "--log", boot["log"], "-g", str(tmp_path / "gboot")])
    assert r.returncode == 0, r.stderr
    rows = [ln.split(b"\t") for ln in open(boot["ab"], "rb").read().splitlines()]
    assert all(len(x) == 8 for x in rows)
    assert b"".join(b"\t".join(x[:4]) + b"\n" for x in rows) == want_ab
