"""Abundance by EM over equivalence classes.  S(r) is the set of global paths (BAM header order) that carry at least one record of
input read r: every traversal, both strands, primary and secondary; reads with no record are in no class.  An EC is a distinct non-empty
S(r), written as its global path IDs in ascending order; count(EC) is the number of reads r with that S(r).  Canonical EC order is
lexicographic on the ascending ID lists; the EM visits ECs in this order.  The EM restates src/em/em.go NewEM / Run / Return
(lines 29-158) over all n_paths of the index; em_py below restates it once more in plain Python, and the library must equal it bit
for bit.  The device (Aligner.ecs, kernels_ec.hpp) groups records by input read, the BAM path (host.report_abundance) by QNAME; the
expectations are recomputed here from the records themselves."""
import math

import numpy as np
import pytest

from bamread import read_bam
from groot_amd import device, host
from oracle import oracle_py as O
from test_coverage import _stage, clipped_reads
from test_shared_reads import _multi_graph_reads, _oracle_alns


def em_py(n_paths, ecs, min_iter=50, max_iter=10000):
    """em.go Run over [(ids, count)] in the order given -> (alpha, iterations, alpha before the zeroing)"""
    tol = math.nextafter(1.0, 2.0) - 1.0
    alpha = [1.0 / n_paths] * n_paths if n_paths else []
    before = list(alpha)
    nxt = [0.0] * n_paths
    final = False
    it = 0
    while it < max_iter:
        for ids, c in ecs:
            c = float(c)
            if c == 0:
                continue
            denom = 0.0
            for p in ids:
                denom += alpha[p]
            if denom < tol:
                continue
            norm = c / denom
            for p in ids:
                nxt[p] += alpha[p] * norm
        changed = 0
        for p in range(n_paths):
            if nxt[p] > 1e-2 and abs(nxt[p] - alpha[p]) / nxt[p] > 1e-2:
                changed += 1
            alpha[p] = nxt[p]
            nxt[p] = 0.0
        stop = changed == 0 and it > min_iter
        if final:
            break
        if stop:
            final = True
            before = list(alpha)
            for p in range(n_paths):
                if alpha[p] < 1e-7 / 10.0:
                    alpha[p] = 0.0
        it += 1
    return alpha, it, before


def csr(ecs):
    off = np.zeros(len(ecs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(i) for i, _ in ecs])
    ids = np.array([p for i, _ in ecs for p in i], dtype=np.uint32)
    return off, ids, np.array([c for _, c in ecs], dtype=np.uint64)


def ecs_of_sets(read_ref):
    """[(ids tuple, reads)] in canonical order over (read, ref) pairs (duplicates allowed)"""
    sets = {}
    for r, p in read_ref:
        sets.setdefault(r, set()).add(int(p))
    out = {}
    for s in sets.values():
        k = tuple(sorted(s))
        out[k] = out.get(k, 0) + 1
    return sorted(out.items())


def ecs_of_alns(alns):
    return ecs_of_sets(zip(alns["read_id"].tolist(), alns["ref_id"].tolist()))


def abundance_text(names, n_paths, ecs, min_reads=1.0):
    """the expected file: em_py over the canonical ECs, one line per path with alpha >= min_reads"""
    if not ecs:
        return b""
    alpha, _, _ = em_py(n_paths, ecs)
    reads = [0] * n_paths
    for ids, c in ecs:
        for p in ids:
            reads[p] += c
    total = 0.0
    for a in alpha:
        total += a
    out = ""
    for p in range(n_paths):
        if alpha[p] >= min_reads:
            nm = names[p][1:] if names[p].startswith("*") else names[p]
            out += "%s\t%d\t%.2f\t%.6f\n" % (nm, reads[p], alpha[p], alpha[p] / total if total > 0 else 0.0)
    return out.encode()


def _names(index):
    return [index.path_name(p) for p in range(index.view.n_paths)]


# ---- host, no GPU ------------------------------------------------------------------------------------------------------

def _check_em(n_paths, ecs, min_iter=50, max_iter=10000):
    a, it = host.em(n_paths, *csr(ecs), min_iter=min_iter, max_iter=max_iter)
    want, wit, before = em_py(n_paths, ecs, min_iter, max_iter)
    assert it == wit
    assert a.tobytes() == np.array(want, dtype=np.float64).tobytes()        # bit for bit
    return a, it, before


def test_em_single_path_and_count_zero_ecs():
    a, it, _ = _check_em(3, [((0, 2), 0), ((1,), 10), ((0, 1, 2), 0)])
    assert a[1] == 10.0 and a[0] == 0.0 and a[2] == 0.0
    # settled at iteration 1; no path changed at the first iteration above min: one more round, then the stop
    assert it == 50 + 2


def test_em_stop_at_min_plus_one():
    for mn in (0, 3, 50):
        _, it, _ = _check_em(2, [((0,), 7), ((1,), 3)], min_iter=mn)
        assert it == mn + 2


def test_em_reaches_max_iterations():
    ecs = [((0, 1, 2), 1000), ((0, 1), 50), ((1, 2), 45), ((0,), 1)]
    _, it_full, _ = _check_em(4, ecs)
    assert 100 < it_full < 10000
    _, it, _ = _check_em(4, ecs, min_iter=1, max_iter=100)
    assert it == 100


def test_em_zeroes_tiny_alpha():
    ecs = [((0, 1), 10), ((0,), 1000), ((2,), 4)]
    a, _, before = _check_em(3, ecs)
    assert 0 < before[1] < 1e-8 and a[1] == 0.0
    assert a[0] > 1000 and a[2] == 4.0


def test_em_empty_and_errors():
    a, it, _ = _check_em(5, [])
    assert not a.any() and it == 50 + 2
    with pytest.raises(host.GrootError):
        host.em(3, *csr([((0,), 1)]), min_iter=10, max_iter=5)          # em.go:31-33
    with pytest.raises(host.GrootError):
        host.em(3, *csr([((3,), 1)]))                                    # an ID past n_paths


def test_em_random_ecs_bit_for_bit():
    rng = np.random.default_rng(9)
    n = 40
    ecs = sorted({tuple(sorted(set(rng.integers(0, n, int(rng.integers(1, 6))).tolist()))): int(rng.integers(0, 50)) for _ in range(120)}.items())
    _check_em(n, ecs)


def test_abundance_from_ecs_any_order_and_repeats(testgfa_index, tmp_path):
    idx = testgfa_index
    n = idx.view.n_paths
    ecs = [((0,), 12), ((0, 1), 5), ((1, n - 1), 3), ((n - 1,), 9), ((2,), 0)]
    want = abundance_text(_names(idx), n, sorted(ecs))
    out = tmp_path / "a.tsv"
    rows = host.abundance_from_ecs(idx, *csr(ecs), out_path=str(out))
    assert out.read_bytes() == want and len(rows) == want.count(b"\n") > 0
    assert all(not r[0].startswith("*") for r in rows)
    # shuffled, IDs reversed, every count split in two halves given apart: canonicalised and summed to the same file
    rev = [(tuple(reversed(i)), c) for i, c in ecs]
    half = [(i, c // 2) for i, c in rev] + [(i, c - c // 2) for i, c in rev[::-1]]
    host.abundance_from_ecs(idx, *csr(half), out_path=str(tmp_path / "b.tsv"))
    assert (tmp_path / "b.tsv").read_bytes() == want
    # the threshold; no ECs: an empty file
    assert host.abundance_from_ecs(idx, *csr(ecs), min_reads=1e9) == []
    host.abundance_from_ecs(idx, *csr([]), min_reads=0.0, out_path=str(tmp_path / "e.tsv"))
    assert (tmp_path / "e.tsv").read_bytes() == b""


@pytest.mark.parametrize("which", ["small", "resfinder"])
@pytest.mark.parametrize("interleave", [False, True])
def test_report_abundance_on_a_bam(which, interleave, small_index, resfinder_index, tmp_path):
    """groot_host_report_abundance == the lines computed here from the BAM's own records grouped by QNAME -- also when the records of
    different reads are interleaved, as the reference writes them -- and == abundance_from_ecs on the records' ECs"""
    index = small_index if which == "small" else resfinder_index
    b, al = _oracle_alns(index, clipped_reads(index, 2500, 17 if which == "small" else 18))
    if interleave:
        al = al[np.random.default_rng(5).permutation(len(al))]
    bam = str(tmp_path / "x.bam")
    w = host.BamWriter(bam, index, date="2020-01-01T00:00:00Z")
    w.write(al, b)
    w.close()
    _, _, recs = read_bam(bam)
    ecs = ecs_of_sets((r["name"], r["ref_id"]) for r in recs if r["flag"] != 4)
    assert any(len(i) > 1 for i, _ in ecs)
    want = abundance_text(_names(index), index.view.n_paths, ecs)
    assert want.count(b"\n") > 3
    out = tmp_path / "a.tsv"
    rows = host.report_abundance(bam, out_path=str(out))
    assert out.read_bytes() == want
    assert len(rows) == want.count(b"\n")
    host.abundance_from_ecs(index, *csr(ecs_of_alns(al)), out_path=str(tmp_path / "d.tsv"))
    assert (tmp_path / "d.tsv").read_bytes() == want
    assert host.report_abundance(bam, min_reads=0.5) != []


# ---- the device side ------------------------------------------------------------------------------------------------------

def _dev_ecs(al):
    off, ids, cnt = al.ecs()
    ecs = [(tuple(ids[off[i]:off[i + 1]].tolist()), int(cnt[i])) for i in range(len(cnt))]
    assert ecs == sorted(ecs) and all(c > 0 for _, c in ecs)              # canonical order, each EC once
    assert all(len(i) and list(i) == sorted(set(i)) for i, _ in ecs)
    return ecs


def _run(index, batches, shared=False, **kw):
    """every batch through one Aligner with EC counting on -> (device ECs, stats, the oracle's records)"""
    al = device.Aligner(index, max_batch_reads=max(len(off) - 1 for _, off in batches), **kw)
    al.ec_enable()
    if shared:
        al.shared_enable()
    run = O.Run(index, 0.99)
    first = 0
    for seq, off in batches:
        al.submit(seq, off, first_read_id=first)
        run.batch(seq, off, first_read_id=first)
        al.wait()
        first += len(off) - 1
    ecs, stats = _dev_ecs(al), al.ec_stats()
    al.close()
    return ecs, stats, run.alns().astype(device.ALN_DTYPE)


@pytest.mark.gpu
@pytest.mark.parametrize("stage,memo,rod", [("path_first", True, False), ("path_first", False, True), ("lean_first", True, True),
                                            ("lean_first", False, False), ("align_kernel", True, False), ("align_kernel", False, True)])
@pytest.mark.parametrize("which", ["small", "argannot", "resfinder"])
def test_device_ecs_equal_the_records(which, stage, memo, rod, small_index, argannot_index, resfinder_index, hip_lib, monkeypatch):
    """the device ECs == the ECs of the oracle's records grouped by read, over three batches with reads in several graphs mixed in,
    under each align stage, memo on and off, results in HBM or copied out"""
    _stage(monkeypatch, stage)
    index = {"small": small_index, "argannot": argannot_index, "resfinder": resfinder_index}[which]
    seed = {"small": 11, "argannot": 21, "resfinder": 31}[which]
    multi = _multi_graph_reads(index, 200, seed + 100)
    batches = [O.pack_reads(clipped_reads(index, 2000, seed + k) + multi) for k in range(3)]
    ecs, stats, alns = _run(index, batches, results_on_device=rod, memo_budget_mb=0 if memo else device.MEMO_OFF)
    want = ecs_of_alns(alns)
    assert len(want) > 10 and any(len(i) > 1 for i, _ in want)
    assert ecs == want
    assert stats["reads"] == len(np.unique(alns["read_id"])) and stats["distinct"] == len(want)
    assert stats["slow_reads"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("slow", [False, True])
def test_slow_path_and_wide_sets(argannot_index, hip_lib, monkeypatch, slow):
    """reads in several graphs and reads with wide sets; under GROOT_TEST_SHARED_SLOW every read in more than one graph is folded in
    on the host from its records"""
    # (arg-annot reads lie in at most three graphs: without the switch no read is slow here.  Reads in more than four graphs, with sets
    # of several hundred paths, are in test_counter_edges.py)
    from groot_amd import synth

    _stage(monkeypatch, "path_first")
    if slow:
        monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    idx = argannot_index
    gpo = idx.arrays["graph_path_off"].astype(np.int64)
    wide = int(np.argmax(np.diff(gpo)))
    multi = _multi_graph_reads(idx, 400, 71)
    cat, o, lens = synth.reference_sequences(idx)
    wide_reads = []
    for p in range(int(gpo[wide]), int(gpo[wide + 1])):
        s = bytes(cat[int(o[p]):int(o[p]) + int(lens[p])])
        wide_reads += [s[i:i + 100] for i in range(0, max(1, len(s) - 100), 97)]
    # a few reads per batch on the slow path (one by one on the host), and many (in one copy)
    batches = [O.pack_reads(multi[:20] + wide_reads[:200]), O.pack_reads(multi), O.pack_reads(wide_reads)]
    ecs, stats, alns = _run(idx, batches, shared=True)
    assert ecs == ecs_of_alns(alns)
    assert max(len(i) for i, _ in ecs) > 64                                # sets past one mask word
    graphs = np.bincount(np.unique(alns["read_id"].astype(np.int64) * (1 << 20) + alns["graph_id"]) >> 20)
    assert (graphs >= 3).any()
    assert stats["slow_reads"] == (int((graphs > 1).sum()) if slow else int((graphs > 4).sum()))


@pytest.mark.gpu
def test_table_growth_with_batches_in_flight(argannot_index, hip_lib, monkeypatch):
    """GROOT_TEST_EC_SLOTS=64: the run-wide table starts tiny and grows (rehashed in stream order) while several batches are in flight"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_EC_SLOTS", "64")
    idx = argannot_index
    multi = _multi_graph_reads(idx, 150, 81)
    batches = [O.pack_reads(clipped_reads(idx, 1500, 90 + k) + multi) for k in range(7)]
    al = device.Aligner(idx, max_batch_reads=max(len(off) - 1 for _, off in batches), pipeline_depth=3, memo_budget_mb=device.MEMO_OFF)
    al.ec_enable()
    run = O.Run(idx, 0.99)
    first, pending = 0, 0
    for seq, off in batches:
        if pending == 3:
            al.release(al.collect()["ticket"])
            pending -= 1
        al.submit(seq, off, first_read_id=first)
        run.batch(seq, off, first_read_id=first)
        pending += 1
        first += len(off) - 1
    for _ in range(pending):
        al.release(al.collect()["ticket"])
    ecs, stats = _dev_ecs(al), al.ec_stats()
    al.close()
    assert ecs == ecs_of_alns(run.alns().astype(device.ALN_DTYPE))
    assert stats["grows"] >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
def test_redone_batch_counts_once(small_index, hip_lib, monkeypatch, rod):
    """GROOT_TEST_SMALL_BUFFERS: the first pass of each batch overflows and is redone at collect; only the redo counts"""
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    batches = [O.pack_reads(clipped_reads(small_index, 3000, 51 + k)) for k in range(2)]
    ecs, stats, alns = _run(small_index, batches, results_on_device=rod, memo_budget_mb=device.MEMO_OFF)
    assert ecs == ecs_of_alns(alns)
    assert stats["reads"] == len(np.unique(alns["read_id"]))


@pytest.mark.gpu
def test_ec_accumulates_resets_and_switches_off(small_index, hip_lib, monkeypatch):
    _stage(monkeypatch, "path_first")
    batches = [O.pack_reads(clipped_reads(small_index, 1500, 41 + k)) for k in range(2)]
    al = device.Aligner(small_index, max_batch_reads=2048, memo_budget_mb=device.MEMO_OFF)
    with pytest.raises(host.GrootError):
        al.ecs()                                                          # off: nothing to export
    al.ec_reset()                                                         # off: a no-op
    al.ec_enable()
    run = O.Run(small_index, 0.99)
    al.submit(*batches[0], first_read_id=0)
    run.batch(*batches[0], first_read_id=0)
    al.wait()
    e1 = dict(_dev_ecs(al))
    assert e1 == dict(ecs_of_alns(run.alns().astype(device.ALN_DTYPE)))
    n0 = len(batches[0][1]) - 1
    al.submit(*batches[1], first_read_id=n0)
    run.batch(*batches[1], first_read_id=n0)
    al.wait()
    e2 = dict(_dev_ecs(al))
    assert e2 == dict(ecs_of_alns(run.alns().astype(device.ALN_DTYPE)))
    al.ec_reset()
    assert _dev_ecs(al) == [] and al.ec_stats()["reads"] == 0
    al.submit(*batches[1], first_read_id=n0)
    al.wait()
    assert dict(_dev_ecs(al)) == {k: v - e1.get(k, 0) for k, v in e2.items() if v - e1.get(k, 0)}
    al.ec_enable(False)
    with pytest.raises(host.GrootError):
        al.ecs()
    al.close()


@pytest.mark.gpu
def test_ec_changes_nothing(small_index, hip_lib, monkeypatch):
    """counts, records, coverage and shared pairs with EC counting on == without it; shared reads alone give the same pairs"""
    _stage(monkeypatch, "path_first")
    seq, off = O.pack_reads(clipped_reads(small_index, 3000, 61) + _multi_graph_reads(small_index, 100, 62))
    out = []
    for ec, sh in ((False, True), (True, True), (True, False), (False, False)):
        al = device.Aligner(small_index, max_batch_reads=4096)
        al.coverage_enable()
        if ec:
            al.ec_enable()
        if sh:
            al.shared_enable()
        al.submit(seq, off)
        c = al.wait()
        out.append((c, al.alns(), al.coverage(), al.shared() if sh else None, _dev_ecs(al) if ec else None))
        al.close()
    for o in out[1:]:
        assert o[0] == out[0][0]
        assert all(np.array_equal(out[0][1][f], o[1][f]) for f in device.ALN_DTYPE.names)
        assert all(np.array_equal(x, y) for x, y in zip(out[0][2], o[2]))
    assert all(np.array_equal(x, y) for x, y in zip(out[0][3], out[1][3]))
    assert out[1][4] == out[2][4] == ecs_of_alns(out[0][1])


@pytest.mark.gpu
def test_ec_at_benchmark_size(argannot_index, hip_lib, monkeypatch):
    """10 M error-free 100 bp reads of the configs[2] generator in one batch: the device ECs == the ECs of that run's own records"""
    from groot_amd import synth

    _stage(monkeypatch, "path_first")
    cat, o, lens = synth.reference_sequences(argannot_index)
    n = 10_000_000
    seq, off, _ = synth.reads_np(cat, o, lens, n, 100)
    al = device.Aligner(argannot_index, max_batch_reads=n)
    al.ec_enable()
    al.submit(seq, off)
    al.wait()
    alns = al.alns()
    d_off, d_ids, d_cnt = al.ecs()
    stats = al.ec_stats()
    al.close()
    assert len(alns) > 10 * n
    key = np.unique(alns["read_id"].astype(np.int64) * 2048 + alns["ref_id"].astype(np.int64))
    rid, ref = key >> 11, key & 2047
    starts = np.flatnonzero(np.r_[True, rid[1:] != rid[:-1]])
    sets = {}
    for s, e in zip(starts, np.r_[starts[1:], len(rid)]):
        t = tuple(ref[s:e].tolist())
        sets[t] = sets.get(t, 0) + 1
    got = {tuple(d_ids[d_off[i]:d_off[i + 1]].tolist()): int(d_cnt[i]) for i in range(len(d_cnt))}
    assert got == sets
    assert stats["reads"] == len(starts) and stats["distinct"] == len(sets)
    # the EM of configs[2]'s ECs: the library's and em_py agree bit for bit
    ecs = sorted(sets.items())
    a, it = host.em(argannot_index.view.n_paths, *csr(ecs))
    want, wit, _ = em_py(argannot_index.view.n_paths, ecs)
    assert it == wit and a.tobytes() == np.array(want, dtype=np.float64).tobytes()
