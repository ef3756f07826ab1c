"""Report coverage without a BAM: records per reference and the pileup of every reference, accumulated on the device while
aligning (Aligner.coverage, kernels_cov.hpp) and turned into `groot report` lines on the host (host.report_coverage).  The
expectations come from the alignment records themselves: reporting.go:104-127 adds 1 to every base of [Pos, Pos + M] (both ends,
clipped to the last base) of the record's reference, M = read length - clips; the rows must be the ones `groot report` writes for a
BAM of the same records."""
import os
import subprocess

import numpy as np
import pytest

from conftest import DATA, REPO
from groot_amd import device, host, synth
from oracle import oracle_py as O

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def expand_coverage(index, alns, seq_off):
    """numpy restatement of reporting.go:100-127 over expanded records -> (records[n_paths], depth[sum path_len]) as uint64"""
    lens = index.arrays["path_len"].astype(np.int64)
    base = np.zeros(len(lens) + 1, dtype=np.int64)
    base[1:] = np.cumsum(lens)
    records = np.bincount(alns["ref_id"].astype(np.int64), minlength=len(lens)).astype(np.uint64)
    off = np.asarray(seq_off, dtype=np.int64)
    rid = alns["read_id"].astype(np.int64)
    m = (off[rid + 1] - off[rid]) - alns["start_clip"].astype(np.int64) - alns["end_clip"].astype(np.int64)
    ref = alns["ref_id"].astype(np.int64)
    pos = alns["pos"].astype(np.int64)
    end = np.minimum(pos + m, lens[ref] - 1)
    ok = pos <= end
    diff = np.zeros(int(base[-1]) + 1, dtype=np.int64)
    np.add.at(diff, base[ref[ok]] + pos[ok], 1)
    np.add.at(diff, base[ref[ok]] + end[ok] + 1, -1)
    depth = np.cumsum(diff[:-1])
    return records, depth.astype(np.uint64)


def clipped_reads(index, n, seed, min_len=60, max_len=150):
    """substrings of the indexed paths in both orientations, a share of them with a wrong first and/or last base (1H clips on the
    records) and a share ending on the last base of their path"""
    cat, o, lens = synth.reference_sequences(index)
    rng = np.random.default_rng(seed)
    reads = []
    for i in range(n):
        s = int(rng.integers(0, len(lens)))
        L = min(int(rng.integers(min_len, max_len + 1)), int(lens[s]))
        st = int(lens[s]) - L if i % 5 == 0 else int(rng.integers(0, lens[s] - L + 1))
        r = bytearray(cat[int(o[s]) + st:int(o[s]) + st + L].tobytes())
        kind = i % 4
        flip = lambda b: b"ACGT"[(b"ACGT".index(bytes([b])) + 1 + int(rng.integers(0, 3))) % 4] if bytes([b]) in b"ACGT" else ord("A")
        if kind in (1, 3):
            r[0] = flip(r[0])
        if kind in (2, 3):
            r[-1] = flip(r[-1])
        r = bytes(r)
        if rng.integers(0, 2):
            r = r.translate(COMP)[::-1]
        reads.append(r)
    return reads


def _batch(reads):
    seq, off = O.pack_reads(reads)
    names = [b"r%d" % i for i in range(len(reads))]
    name_off = np.zeros(len(reads) + 1, dtype=np.uint64)
    name_off[1:] = np.cumsum([len(x) for x in names])
    return {"seq": seq, "seq_off": off, "qual": np.full(len(seq), 40, dtype=np.uint8), "names": np.frombuffer(b"".join(names), dtype=np.uint8),
            "name_off": name_off}


@pytest.mark.parametrize("which", ["small", "resfinder"])
def test_report_from_counts_equals_report_from_bam(which, small_index, resfinder_index, tmp_path):
    """host.report_coverage on the numpy pileup of the oracle's records == host.report on a BAM of the same records"""
    index = small_index if which == "small" else resfinder_index
    reads = clipped_reads(index, 3000, 7 if which == "small" else 8)
    b = _batch(reads)
    run = O.Run(index, 0.99)
    run.batch(b["seq"], b["seq_off"])
    al = run.alns().astype(device.ALN_DTYPE)
    assert (al["start_clip"] == 1).any() and (al["end_clip"] == 1).any() and len(np.unique(al["ref_id"])) > 20
    records, depth = expand_coverage(index, al, b["seq_off"])
    # some record's span reaches (and is clipped at) its path's last base
    lens = index.arrays["path_len"].astype(np.int64)
    m = np.diff(b["seq_off"].astype(np.int64))[al["read_id"]] - al["start_clip"] - al["end_clip"]
    assert (al["pos"].astype(np.int64) + m >= lens[al["ref_id"]] - 1).any()
    bam = str(tmp_path / "x.bam")
    w = host.BamWriter(bam, index, date="2020-01-01T00:00:00Z")
    w.write(al, b)
    w.close()
    for cutoff, low in ((0.97, False), (0.5, False), (0.0, True), (0.5, True)):
        want = host.report(bam, cutoff, low_cov=low)
        got = host.report_coverage(index, records, depth, cutoff, low_cov=low)
        assert got == want, (cutoff, low)
    assert len(host.report(bam, 0.5)) > 0
    # the file is byte for byte the same too
    host.report(bam, 0.5, out_path=str(tmp_path / "a.tsv"))
    host.report_coverage(index, records, depth, 0.5, out_path=str(tmp_path / "b.tsv"))
    assert open(tmp_path / "a.tsv", "rb").read() == open(tmp_path / "b.tsv", "rb").read()
    with pytest.raises(host.GrootError):
        host.report_coverage(index, records, depth, 1.5)                 # cmd/report.go:95-97
    with pytest.raises(ValueError):
        host.report_coverage(index, records[:-1], depth)


def test_report_from_counts_edges(testgfa_index):
    """the quirks of test_report.py::test_pileup_and_cigar_quirks, from counts"""
    idx = testgfa_index
    lens = idx.arrays["path_len"].astype(np.int64)
    L, name = int(lens[0]), idx.path_name(0).lstrip("*")
    records = np.zeros(idx.view.n_paths, dtype=np.uint64)
    depth = np.zeros(int(lens.sum()), dtype=np.uint64)
    depth[0:101] = 1
    depth[300:351] = 1
    records[0] = 2
    assert host.report_coverage(idx, records, depth, 0.0) == [(name, 2, L, f"101M199D51M{L - 351}D")]
    assert host.report_coverage(idx, records, depth, 0.0, low_cov=True) == []
    depth[:] = 0
    depth[int(lens[0]):int(lens[0]) + int(lens[1])] = 3     # a pileup without records is not reported (reporting.go:128)
    assert host.report_coverage(idx, records * 0, depth, 0.0) == []


# ---- the device side ------------------------------------------------------------------------------------------------------

STAGES = {"path_first": {}, "lean_first": {"GROOT_LEAN": "1"}, "align_kernel": {"GROOT_NO_PATH_PASS": "1"}}


def _stage(monkeypatch, stage):
    for v in ("GROOT_NO_PATH_PASS", "GROOT_LEAN", "GROOT_TEST_SMALL_BUFFERS"):
        monkeypatch.delenv(v, raising=False)
    for k, v in STAGES[stage].items():
        monkeypatch.setenv(k, v)


def _global_off(batches):
    lens = np.concatenate([np.diff(off.astype(np.int64)) for _, off in batches])
    g = np.zeros(len(lens) + 1, dtype=np.int64)
    g[1:] = np.cumsum(lens)
    return g


def _run_batches(index, batches, **kw):
    """every batch through one Aligner with coverage on -> (device records, depth, the oracle's records of the same reads)"""
    al = device.Aligner(index, max_batch_reads=max(len(off) - 1 for _, off in batches), **kw)
    al.coverage_enable()
    run = O.Run(index, 0.99)
    first = 0
    for seq, off in batches:
        al.submit(seq, off, first_read_id=first)
        run.batch(seq, off, first_read_id=first)
        al.wait()
        first += len(off) - 1
    records, depth = al.coverage()
    al.close()
    return records, depth, run.alns().astype(device.ALN_DTYPE)


def _assert_coverage(index, records, depth, alns, batches):
    want_r, want_d = expand_coverage(index, alns, _global_off(batches))
    assert records.sum() == len(alns) > 0
    assert np.array_equal(records, want_r)
    assert np.array_equal(depth, want_d), np.flatnonzero(depth != want_d)[:10]


def _reads_batches(index, n_batches, n, seed):
    return [O.pack_reads(clipped_reads(index, n, seed + b)) for b in range(n_batches)]


@pytest.mark.gpu
@pytest.mark.parametrize("stage,memo,rod", [("path_first", True, False), ("path_first", False, True), ("lean_first", True, True),
                                            ("lean_first", False, False), ("align_kernel", True, False), ("align_kernel", False, True)])
@pytest.mark.parametrize("which", ["small", "argannot", "resfinder"])
def test_device_coverage_equals_the_records(which, stage, memo, rod, small_index, argannot_index, resfinder_index, hip_lib, monkeypatch):
    """records and the whole pileup from the device == the numpy expansion of the oracle's records, over three batches of mixed
    lengths with 1H clips, under each align stage, with the memo on and off, with results in HBM or copied out"""
    _stage(monkeypatch, stage)
    index = {"small": small_index, "argannot": argannot_index, "resfinder": resfinder_index}[which]
    batches = _reads_batches(index, 3, 2000, {"small": 11, "argannot": 21, "resfinder": 31}[which])
    r, d, alns = _run_batches(index, batches, results_on_device=rod, memo_budget_mb=0 if memo else device.MEMO_OFF)
    assert (alns["start_clip"] == 1).any() and (alns["end_clip"] == 1).any()
    _assert_coverage(index, r, d, alns, batches)


@pytest.mark.gpu
def test_coverage_accumulates_resets_and_switches_off(small_index, hip_lib, monkeypatch):
    _stage(monkeypatch, "path_first")
    batches = _reads_batches(small_index, 2, 1500, 41)
    al = device.Aligner(small_index, max_batch_reads=2048, memo_budget_mb=device.MEMO_OFF)
    with pytest.raises(host.GrootError):
        al.coverage()                                            # off: nothing to export
    al.coverage_enable()
    run = O.Run(small_index, 0.99)
    al.submit(*batches[0], first_read_id=0)
    run.batch(*batches[0], first_read_id=0)
    al.wait()
    r1, d1 = al.coverage()
    _assert_coverage(small_index, r1, d1, run.alns().astype(device.ALN_DTYPE), batches[:1])
    n0 = len(batches[0][1]) - 1
    al.submit(*batches[1], first_read_id=n0)
    run.batch(*batches[1], first_read_id=n0)
    al.wait()
    r2, d2 = al.coverage()
    _assert_coverage(small_index, r2, d2, run.alns().astype(device.ALN_DTYPE), batches)
    al.coverage_reset()
    r3, d3 = al.coverage()
    assert not r3.any() and not d3.any()
    al.submit(*batches[1], first_read_id=n0)
    al.wait()
    r4, d4 = al.coverage()
    assert np.array_equal(r4, r2 - r1) and np.array_equal(d4, d2 - d1)
    al.coverage_enable(False)
    with pytest.raises(host.GrootError):
        al.coverage()
    al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
def test_redone_batch_counts_once(small_index, hip_lib, monkeypatch, rod):
    """GROOT_TEST_SMALL_BUFFERS: every growable buffer starts too small, the first pass of each batch overflows and is redone at
    collect.  Only the redo counts."""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    batches = _reads_batches(small_index, 2, 3000, 51)
    r, d, alns = _run_batches(small_index, batches, results_on_device=rod, memo_budget_mb=device.MEMO_OFF)
    _assert_coverage(small_index, r, d, alns, batches)


@pytest.mark.gpu
def test_coverage_off_changes_nothing(small_index, hip_lib, monkeypatch):
    """counts and records with coverage on == without it"""
    _stage(monkeypatch, "path_first")
    seq, off = _reads_batches(small_index, 1, 3000, 61)[0]
    out = []
    for on in (False, True):
        al = device.Aligner(small_index, max_batch_reads=4096)
        if on:
            al.coverage_enable()
        al.submit(seq, off)
        c = al.wait()
        out.append((c, al.alns()))
        al.close()
    assert out[0][0] == out[1][0]
    assert all(np.array_equal(out[0][1][f], out[1][1][f]) for f in device.ALN_DTYPE.names)


@pytest.mark.gpu
def test_coverage_at_benchmark_size(argannot_index, hip_lib, monkeypatch):
    """1 M error-free 100 bp reads of the configs[2] generator, in one batch: the device coverage == the numpy expansion of that run's
    own records"""
    _stage(monkeypatch, "path_first")
    cat, o, lens = synth.reference_sequences(argannot_index)
    n = 1 << 20
    seq, off, _ = synth.reads_np(cat, o, lens, n, 100)
    al = device.Aligner(argannot_index, max_batch_reads=n)
    al.coverage_enable()
    al.submit(seq, off)
    al.wait()
    alns = al.alns()
    records, depth = al.coverage()
    al.close()
    want_r, want_d = expand_coverage(argannot_index, alns, off)
    assert len(alns) > 10 * n
    assert np.array_equal(records, want_r) and np.array_equal(depth, want_d)
