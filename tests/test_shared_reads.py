"""Shared reads: for every pair of reported references a <= b, the reads with at least one record on a and one on b (the
multimapper check of the reference tutorial).  S(r) = the global paths carrying a record of read r (every traversal, both strands,
primary and secondary); shared[a][b] = |{r : a, b in S(r)}|, the diagonal being the distinct reads of a reference.  The device
counts (Aligner.shared, kernels_shared.hpp) group records by input read; the BAM path (host.report_shared) by QNAME.  The
expectations are recomputed here from the records themselves."""
import numpy as np
import pytest

from bamread import read_bam
from groot_amd import device, host, synth
from oracle import oracle_py as O
from test_coverage import _batch, _stage, clipped_reads, expand_coverage


def pairs_of_sets(read_ref):
    """{(a, b): reads} over (read, ref) pairs (duplicates allowed)"""
    sets = {}
    for r, p in read_ref:
        sets.setdefault(r, set()).add(int(p))
    out = {}
    for s in sets.values():
        s = sorted(s)
        for i, a in enumerate(s):
            for b in s[i:]:
                out[(a, b)] = out.get((a, b), 0) + 1
    return out


def pairs_of_alns(alns):
    return pairs_of_sets(zip(alns["read_id"].tolist(), alns["ref_id"].tolist()))


def shared_rows(index, report_rows, pairs):
    """the expected lines: pairs of reported references, header order, names as the report prints them"""
    names = [index.path_name(p).lstrip("*") if index.path_name(p).startswith("*") else index.path_name(p) for p in range(index.view.n_paths)]
    rep = {r[0] for r in report_rows}
    return [(names[a], names[b], n) for (a, b), n in sorted(pairs.items()) if n and names[a] in rep and names[b] in rep]


# ---- host, no GPU ------------------------------------------------------------------------------------------------------

def _counts(idx, covered):
    """records / depth with path p (of covered: {p: (records, [(lo, hi)])}) covered on [lo, hi) spans"""
    lens = idx.arrays["path_len"].astype(np.int64)
    base = np.concatenate([[0], np.cumsum(lens)])
    records = np.zeros(idx.view.n_paths, dtype=np.uint64)
    depth = np.zeros(int(lens.sum()), dtype=np.uint64)
    for p, (n, spans) in covered.items():
        records[p] = n
        for lo, hi in spans:
            depth[base[p] + lo:base[p] + hi] = 1
    return records, depth, lens


def test_from_counts_cutoff_lowcov_names_and_diagonal(testgfa_index, tmp_path):
    idx = testgfa_index
    n = idx.view.n_paths
    assert n >= 4
    star = [p for p in range(n) if idx.path_name(p).startswith("*")]
    assert star, "the fixture has a cluster representative"
    s = star[0]
    lens = idx.arrays["path_len"].astype(np.int64)
    others = [p for p in range(n) if p != s]
    p0, p1, p2 = others[:3]
    L0 = int(lens[p0])
    # s: full; p0: exactly 97 % covered (as a prefix); p1: 96 % (below the default cutoff); p2: full but with an internal gap
    cov = {s: (5, [(0, int(lens[s]))]), p0: (3, [(0, (97 * L0 + 99) // 100)]), p1: (2, [(0, int(lens[p1]) * 96 // 100)]),
           p2: (4, [(0, 10), (20, int(lens[p2]))])}
    records, depth, _ = _counts(idx, cov)
    raw = [(s, s, 5), (s, p0, 2), (s, p1, 1), (p0, p0, 3), (p0, p2, 1), (p1, p1, 2), (p2, p2, 4), (s, p2, 0), (p2, p2, 0)]
    raw = [(min(x, y), max(x, y), c) for x, y, c in raw]
    pa = np.array([r[0] for r in raw], dtype=np.uint32)
    pb = np.array([r[1] for r in raw], dtype=np.uint32)
    cnt = np.array([r[2] for r in raw], dtype=np.uint64)
    nm = lambda p: idx.path_name(p)[1:] if idx.path_name(p).startswith("*") else idx.path_name(p)
    want_all = sorted((a, b, c) for a, b, c in raw if c)
    order = [nm(p) for p in range(n)]

    # 0.97: p0 exactly at the cutoff is in, p1 (96 %) out; --lowCov (0.97): p2's internal gap drops it too
    for cutoff, low, reported in ((0.97, False, {s, p0, p2}), (0.0, False, {s, p0, p1, p2}), (0.5, True, {s, p0})):
        rep = host.report_coverage(idx, records, depth, cutoff, low_cov=low)
        assert {r[0] for r in rep} == {nm(p) for p in reported}, (cutoff, low)
        got = host.shared_from_counts(idx, records, depth, pa, pb, cnt, cutoff, low_cov=low)
        assert got == sorted(got, key=lambda r: (order.index(r[0]), order.index(r[1])))      # header order
        assert got == [(nm(a), nm(b), c) for a, b, c in want_all if a in reported and b in reported], (cutoff, low)
        assert all(not r[0].startswith("*") and not r[1].startswith("*") for r in got)
        assert any(r[0] == r[1] for r in got)                                                 # the diagonal lines are there
        assert any(r[0] == nm(s) for r in got)                                                # the '*' name, stripped
    # pairs in any order, repeated pairs summed (the lists of two contexts)
    perm = np.random.default_rng(3).permutation(len(pa))
    got = host.shared_from_counts(idx, records, depth, np.concatenate([pa[perm], pa]), np.concatenate([pb[perm], pb]),
                                  np.concatenate([cnt[perm], cnt]), 0.0)
    assert got == [(a, b, 2 * c) for a, b, c in host.shared_from_counts(idx, records, depth, pa, pb, cnt, 0.0)]
    # nothing reported: an empty file
    out = tmp_path / "empty.tsv"
    assert host.shared_from_counts(idx, records * 0, depth, pa, pb, cnt, 0.0, out_path=str(out)) == []
    assert out.read_bytes() == b""
    # a > b, b out of range, a cutoff above 1
    for bad in (([p1], [p0]), ([0], [n])):
        with pytest.raises(host.GrootError):
            host.shared_from_counts(idx, records, depth, *bad, [1], 0.0)
    with pytest.raises(host.GrootError):
        host.shared_from_counts(idx, records, depth, pa, pb, cnt, 1.5)


def _oracle_alns(index, reads):
    b = _batch(reads)
    run = O.Run(index, 0.99)
    run.batch(b["seq"], b["seq_off"])
    return b, run.alns().astype(device.ALN_DTYPE)


@pytest.mark.parametrize("which", ["small", "resfinder"])
@pytest.mark.parametrize("interleave", [False, True])
def test_report_shared_on_a_bam(which, interleave, small_index, resfinder_index, tmp_path):
    """groot_host_report_shared: the report is groot_host_report's byte for byte, the shared file the pairs recomputed from the BAM's
    own records grouped by QNAME -- also when the records of different reads are interleaved, as the reference writes them"""
    index = small_index if which == "small" else resfinder_index
    b, al = _oracle_alns(index, clipped_reads(index, 2500, 17 if which == "small" else 18))
    if interleave:
        al = al[np.random.default_rng(5).permutation(len(al))]
    bam = str(tmp_path / "x.bam")
    w = host.BamWriter(bam, index, date="2020-01-01T00:00:00Z")
    w.write(al, b)
    w.close()
    _, _, recs = read_bam(bam)
    if interleave:
        names = [r["name"] for r in recs]
        assert any(names[i] != names[i + 1] and names[i] in names[i + 2:i + 50] for i in range(len(names) - 2))
    multi = pairs_of_sets((r["name"], r["ref_id"]) for r in recs if r["flag"] != 4)
    assert any(a != b for a, b in multi)
    for cutoff, low in ((0.97, False), (0.5, False), (0.0, True)):
        rep_file, sh_file = tmp_path / "r.tsv", tmp_path / "s.tsv"
        rep, sh = host.report_shared(bam, cutoff, low_cov=low, report_out=str(rep_file), shared_out=str(sh_file))
        host.report(bam, cutoff, low_cov=low, out_path=str(tmp_path / "want.tsv"))
        assert rep_file.read_bytes() == (tmp_path / "want.tsv").read_bytes()
        assert sh == shared_rows(index, rep, multi), (cutoff, low)
        # the device-side host function agrees on the same records
        records, depth = expand_coverage(index, al, b["seq_off"])
        keys = sorted(pairs_of_alns(al).items())
        pa = np.array([k[0][0] for k in keys], dtype=np.uint32)
        pb = np.array([k[0][1] for k in keys], dtype=np.uint32)
        cn = np.array([k[1] for k in keys], dtype=np.uint64)
        host.shared_from_counts(index, records, depth, pa, pb, cn, cutoff, low_cov=low, out_path=str(tmp_path / "d.tsv"))
        assert (tmp_path / "d.tsv").read_bytes() == sh_file.read_bytes()
    assert len(host.report_shared(bam, 0.5)[1]) > 0


# ---- the device side ------------------------------------------------------------------------------------------------------

def _dev_pairs(al):
    a, b, c = al.shared()
    assert np.all(a <= b) and np.all(c > 0)
    assert np.all(np.diff(a.astype(np.int64) * (1 << 32) + b) > 0)        # ascending, each pair once
    return {(int(x), int(y)): int(z) for x, y, z in zip(a, b, c)}


def _run(index, batches, check_slow=False, **kw):
    """every batch through one Aligner with shared reads (and coverage) on -> (device pairs, stats, the oracle's records)"""
    al = device.Aligner(index, max_batch_reads=max(len(off) - 1 for _, off in batches), **kw)
    al.shared_enable()
    al.coverage_enable()
    run = O.Run(index, 0.99)
    first = 0
    for seq, off in batches:
        al.submit(seq, off, first_read_id=first)
        run.batch(seq, off, first_read_id=first)
        al.wait()
        first += len(off) - 1
    pairs, stats = _dev_pairs(al), al.shared_stats()
    al.close()
    return pairs, stats, run.alns().astype(device.ALN_DTYPE)


def _multi_graph_reads(index, n, seed):
    """reads on segments that several graphs share (their records lie in more than one graph): the slow path"""
    cat, o, lens = synth.reference_sequences(index)
    seq, off, _ = synth.reads_np(cat, o, lens, 20000, 100, seed=seed)
    reads = [bytes(seq[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]
    b, al = _oracle_alns(index, reads)
    rid, g = al["read_id"].astype(np.int64), al["graph_id"].astype(np.int64)
    keys = np.unique(rid * (1 << 20) + g) >> 20
    ids, cnt = np.unique(keys, return_counts=True)
    multi = ids[cnt > 1][:n]
    seq = b["seq"]
    off = b["seq_off"].astype(np.int64)
    return [bytes(seq[off[i]:off[i + 1]]) for i in multi]


@pytest.mark.gpu
@pytest.mark.parametrize("stage,memo,rod", [("path_first", True, False), ("path_first", False, True), ("lean_first", True, True),
                                            ("lean_first", False, False), ("align_kernel", True, False), ("align_kernel", False, True)])
@pytest.mark.parametrize("which", ["small", "argannot", "resfinder"])
def test_device_pairs_equal_the_records(which, stage, memo, rod, small_index, argannot_index, resfinder_index, hip_lib, monkeypatch):
    """the device pairs == the pairs of the oracle's records grouped by read, over three batches with reads in several graphs mixed
    in, under each align stage, memo on and off, results in HBM or copied out"""
    _stage(monkeypatch, stage)
    index = {"small": small_index, "argannot": argannot_index, "resfinder": resfinder_index}[which]
    seed = {"small": 11, "argannot": 21, "resfinder": 31}[which]
    multi = _multi_graph_reads(index, 200, seed + 100)
    batches = [O.pack_reads(clipped_reads(index, 2000, seed + k) + multi) for k in range(3)]
    pairs, stats, alns = _run(index, batches, results_on_device=rod, memo_budget_mb=0 if memo else device.MEMO_OFF)
    want = pairs_of_alns(alns)
    assert len(want) > 20 and any(a != b for a, b in want)
    assert pairs == want
    assert stats["reads"] == len(np.unique(alns["read_id"]))
    assert stats["slow_reads"] == 0                                       # reads in 2 to 4 graphs take the fast path


@pytest.mark.gpu
@pytest.mark.parametrize("slow", [False, True])
def test_slow_path_and_wide_sets(argannot_index, hip_lib, monkeypatch, slow):
    """reads whose set is wide (segments of the widest graph) and reads in several graphs: on the fast path (one to kSharedSegs
    segments per read) and, under GROOT_TEST_SHARED_SLOW, every read in more than one graph on the wave-per-read slow path"""
    _stage(monkeypatch, "path_first")
    if slow:
        monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    idx = argannot_index
    gpo = idx.arrays["graph_path_off"].astype(np.int64)
    wide = int(np.argmax(np.diff(gpo)))
    multi = _multi_graph_reads(idx, 400, 71)
    assert len(multi) > 20
    cat, o, lens = synth.reference_sequences(idx)
    wide_reads = []
    for p in range(int(gpo[wide]), int(gpo[wide + 1])):
        s = bytes(cat[int(o[p]):int(o[p]) + int(lens[p])])
        wide_reads += [s[i:i + 100] for i in range(0, max(1, len(s) - 100), 97)]
    pairs, stats, alns = _run(idx, [O.pack_reads(multi), O.pack_reads(wide_reads)])
    want = pairs_of_alns(alns)
    assert pairs == want
    key = np.unique(alns["read_id"].astype(np.int64) * (1 << 20) + alns["ref_id"])
    assert np.bincount(key >> 20).max() > 64                              # sets past one mask word
    graphs = np.bincount(np.unique(alns["read_id"].astype(np.int64) * (1 << 20) + alns["graph_id"]) >> 20)
    assert (graphs >= 3).any()
    n_multi = int((graphs > 1).sum())
    assert n_multi >= len(multi)
    assert stats["slow_reads"] == (n_multi if slow else 0)


@pytest.mark.gpu
def test_shared_accumulates_resets_and_switches_off(small_index, hip_lib, monkeypatch):
    _stage(monkeypatch, "path_first")
    batches = [O.pack_reads(clipped_reads(small_index, 1500, 41 + k)) for k in range(2)]
    al = device.Aligner(small_index, max_batch_reads=2048, memo_budget_mb=device.MEMO_OFF)
    with pytest.raises(host.GrootError):
        al.shared()                                                       # off: nothing to export
    al.shared_reset()                                                     # off: a no-op
    al.shared_enable()
    run = O.Run(small_index, 0.99)
    al.submit(*batches[0], first_read_id=0)
    run.batch(*batches[0], first_read_id=0)
    al.wait()
    p1 = _dev_pairs(al)
    assert p1 == pairs_of_alns(run.alns().astype(device.ALN_DTYPE))
    n0 = len(batches[0][1]) - 1
    al.submit(*batches[1], first_read_id=n0)
    run.batch(*batches[1], first_read_id=n0)
    al.wait()
    p2 = _dev_pairs(al)
    assert p2 == pairs_of_alns(run.alns().astype(device.ALN_DTYPE))
    al.shared_reset()
    assert _dev_pairs(al) == {} and al.shared_stats()["reads"] == 0
    al.submit(*batches[1], first_read_id=n0)
    al.wait()
    p4 = _dev_pairs(al)
    assert p4 == {k: v - p1.get(k, 0) for k, v in p2.items() if v - p1.get(k, 0)}
    al.shared_enable(False)
    with pytest.raises(host.GrootError):
        al.shared()
    al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
def test_redone_batch_counts_once(small_index, hip_lib, monkeypatch, rod):
    """GROOT_TEST_SMALL_BUFFERS: the first pass of each batch overflows and is redone at collect; only the redo counts"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    batches = [O.pack_reads(clipped_reads(small_index, 3000, 51 + k)) for k in range(2)]
    pairs, stats, alns = _run(small_index, batches, results_on_device=rod, memo_budget_mb=device.MEMO_OFF)
    assert pairs == pairs_of_alns(alns)
    assert stats["reads"] == len(np.unique(alns["read_id"]))


@pytest.mark.gpu
def test_shared_off_changes_nothing(small_index, hip_lib, monkeypatch):
    """counts, records and coverage with shared reads on == without them"""
    _stage(monkeypatch, "path_first")
    seq, off = O.pack_reads(clipped_reads(small_index, 3000, 61))
    out = []
    for on in (False, True):
        al = device.Aligner(small_index, max_batch_reads=4096)
        al.coverage_enable()
        if on:
            al.shared_enable()
        al.submit(seq, off)
        c = al.wait()
        out.append((c, al.alns(), al.coverage()))
        al.close()
    assert out[0][0] == out[1][0]
    assert all(np.array_equal(out[0][1][f], out[1][1][f]) for f in device.ALN_DTYPE.names)
    assert all(np.array_equal(x, y) for x, y in zip(out[0][2], out[1][2]))


@pytest.mark.gpu
def test_shared_at_benchmark_size(argannot_index, hip_lib, monkeypatch):
    """10 M error-free 100 bp reads of the configs[2] generator in one batch: the device pairs == the pairs of that run's own records"""
    _stage(monkeypatch, "path_first")
    cat, o, lens = synth.reference_sequences(argannot_index)
    n = 10_000_000
    seq, off, _ = synth.reads_np(cat, o, lens, n, 100)
    al = device.Aligner(argannot_index, max_batch_reads=n)
    al.shared_enable()
    al.submit(seq, off)
    al.wait()
    alns = al.alns()
    pairs = _dev_pairs(al)
    stats = al.shared_stats()
    al.close()
    assert len(alns) > 10 * n
    # the records' pairs, in numpy: sorted unique (read, ref), then per distinct set its count
    key = np.unique(alns["read_id"].astype(np.int64) * 2048 + alns["ref_id"].astype(np.int64))
    rid, ref = key >> 11, key & 2047
    starts = np.flatnonzero(np.r_[True, rid[1:] != rid[:-1]])
    sets = {}
    for s, e in zip(starts, np.r_[starts[1:], len(rid)]):
        t = ref[s:e].tobytes()
        sets[t] = sets.get(t, 0) + 1
    want = {}
    for t, c in sets.items():
        v = np.frombuffer(t, dtype=np.int64)
        ia, ib = np.triu_indices(len(v))
        for a, b in zip(v[ia].tolist(), v[ib].tolist()):
            want[(a, b)] = want.get((a, b), 0) + c
    assert pairs == want
    assert stats["reads"] == len(starts) and stats["distinct_sets"] <= len(sets) + stats["slow_reads"]
