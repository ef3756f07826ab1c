"""Bootstrap intervals of the abundance estimate (include/groot_host.h, "bootstrap intervals").

Input: ECs in canonical order as CSR (n_ec, off, ids, count over n_paths paths), N = the sum of count; B replicates, a 64-bit seed,
n_draws per replicate (0 means N).  Draw j (0 <= j < n_draws) of replicate b, all arithmetic modulo 2^64:

    z = seed + (b * n_draws + j + 1) * 0x9E3779B97F4A7C15
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB
    z =  z ^ (z >> 31)
    t = high 64 bits of the 128-bit product z * N          (0 <= t < N)
    e = the EC with cum[e] <= t < cum[e+1]                 (an EC with count 0 is never drawn)
    boot_count[b][e] += 1

alpha_b = groot_host_em over boot_count[b], bit for bit, with its own iteration count.  Per path p over x_b = alpha_b[p], sums in order
of b, no FMA: boot_mean = (sum x_b) / B; boot_sd = sqrt(sum (x_b - boot_mean)^2 / (B - 1)), 0 when B = 1; with v = the x_b sorted
and q = (25 * (B - 1)) // 1000, boot_lo = v[q], boot_hi = v[B - 1 - q].  The file gets these four columns, "%.2f", after today's four.

The host library is compared with the plain-Python restatement below, the device (kernels_boot.hpp) with the host library -- in
boot_count, alpha and iterations, bit for bit: the definitions allow no tolerance."""
import bisect
import math

import numpy as np
import pytest

from groot_amd import device, host
from oracle import oracle_py as O
from test_abundance import _names, abundance_text, csr, em_py
from test_coverage import _stage, clipped_reads
from test_shared_reads import _multi_graph_reads

M64 = (1 << 64) - 1


def draws_py(counts, n_boot, seed, n_draws=0):
    """the resampling above in plain Python -> [n_boot][n_ec]"""
    cum = [0]
    for c in counts:
        cum.append(cum[-1] + int(c))
    total = cum[-1]
    n_draws = n_draws or total
    out = []
    for b in range(n_boot):
        row = [0] * len(counts)
        for j in range(n_draws if counts else 0):
            z = (seed + (b * n_draws + j + 1) * 0x9E3779B97F4A7C15) & M64
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
            z = z ^ (z >> 31)
            t = (z * total) >> 64
            row[bisect.bisect_right(cum, t) - 1] += 1
        out.append(row)
    return out


def bootstrap_py(n_paths, ecs, n_boot, seed, n_draws=0, min_iter=50, max_iter=10000):
    bc = draws_py([c for _, c in ecs], n_boot, seed, n_draws)
    alpha, its = [], []
    for row in bc:
        a, it, _ = em_py(n_paths, [(ids, c) for (ids, _), c in zip(ecs, row)], min_iter, max_iter)
        alpha.append(a)
        its.append(it)
    return (np.array(bc, dtype=np.uint64).reshape(n_boot, len(ecs)), np.array(alpha, dtype=np.float64).reshape(n_boot, n_paths),
            np.array(its, dtype=np.uint32))


def same(got, want):
    """boot_count, alpha, iterations: bit for bit"""
    for g, w, what in zip(got, want, ("boot_count", "alpha", "iterations")):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint64 if g.dtype.itemsize == 8 else np.uint32) != w.view(np.uint64 if w.dtype.itemsize == 8 else np.uint32))
            raise AssertionError(f"{what}: {len(bad)} difference(s), the first at {bad[0].tolist()}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}")


def random_ecs(seed, n_paths=40, n=300, max_len=6, max_count=50):
    rng = np.random.default_rng(seed)
    ecs = {tuple(sorted(set(rng.integers(0, n_paths, int(rng.integers(1, max_len))).tolist()))): int(rng.integers(0, max_count)) for _ in range(n)}
    assert any(c == 0 for c in ecs.values())
    return sorted(ecs.items())


BIG = [((0, 1), 1 << 39), ((1,), 3), ((0, 2), (1 << 40) + 12345), ((2, 3), 0), ((3,), 7)]     # totals above 2^40


def stats_text(names, n_paths, ecs, boot_alpha, min_reads=1.0):
    """the expected file: today's four columns (abundance_text), then mean / sd / lo / hi of the replicates"""
    base = abundance_text(names, n_paths, ecs, min_reads).decode().splitlines()
    alpha, _, _ = em_py(n_paths, ecs)
    B = len(boot_alpha)
    out, k = "", 0
    for p in range(n_paths):
        if not alpha[p] >= min_reads:
            continue
        x = [float(boot_alpha[b][p]) for b in range(B)]
        s = 0.0
        for v in x:
            s += v
        mean = s / B
        s2 = 0.0
        for v in x:
            d = v - mean
            s2 += d * d
        sd = math.sqrt(s2 / (B - 1)) if B > 1 else 0.0
        v = sorted(x)
        q = (25 * (B - 1)) // 1000
        out += base[k] + "\t%.2f\t%.2f\t%.2f\t%.2f\n" % (mean, sd, v[q], v[B - 1 - q])
        k += 1
    assert k == len(base)
    return out.encode()


# ---- host, no GPU ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 7, 0xFFFFFFFFFFFFFFF1])
def test_host_equals_python_on_random_ecs(seed):
    ecs = random_ecs(3)
    n = sum(c for _, c in ecs)
    for n_draws in (0, n // 3, n + 17):
        same(host.em_bootstrap(40, *csr(ecs), 3, seed=seed, n_draws=n_draws), bootstrap_py(40, ecs, 3, seed, n_draws))


def test_host_equals_python_above_2_40():
    assert sum(c for _, c in BIG) > 1 << 40
    got = host.em_bootstrap(4, *csr(BIG), 4, seed=5, n_draws=20000)
    same(got, bootstrap_py(4, BIG, 4, 5, 20000))
    assert got[0][:, 3].sum() == 0 and got[0][:, 0].min() > 5000 and got[0][:, 2].min() > 12000


def test_resampling_properties():
    ecs = random_ecs(11)
    n = sum(c for _, c in ecs)
    args = csr(ecs)
    b7 = host.em_bootstrap(40, *args, 7, seed=3)
    assert (b7[0].sum(axis=1) == n).all()                                              # every replicate's counts sum to n_draws
    zero = np.array([c == 0 for _, c in ecs])
    assert zero.any() and not b7[0][:, zero].any()                                     # an EC with count 0 is never drawn
    same(host.em_bootstrap(40, *args, 3, seed=3), tuple(x[:3] for x in b7))            # B = 3 is the prefix of B = 7
    assert not np.array_equal(host.em_bootstrap(40, *args, 3, seed=4)[0], b7[0][:3])   # another seed, other counts
    assert len({r.tobytes() for r in b7[0]}) == 7                                      # the replicates differ from each other
    d = host.em_bootstrap(40, *args, 2, seed=3, n_draws=1234)
    assert (d[0].sum(axis=1) == 1234).all()
    for threads in (3, 16):
        same(host.em_bootstrap(40, *args, 7, seed=3, threads=threads), b7)
    assert len(set(b7[2].tolist())) > 1                                                # replicates stop at different iterations


def test_errors_and_no_ecs():
    ecs = [((0,), 4), ((0, 1), 2)]
    with pytest.raises(host.GrootError):
        host.em_bootstrap(2, *csr(ecs), 0)                                             # n_boot = 0
    with pytest.raises(host.GrootError):
        host.em_bootstrap(2, *csr([((0,), 0), ((1,), 0)]), 3)                          # N = 0 with n_ec > 0
    with pytest.raises(host.GrootError):
        host.em_bootstrap(2, *csr(ecs), 3, min_iter=10, max_iter=5)
    with pytest.raises(host.GrootError):
        host.em_bootstrap(2, *csr([((2,), 1)]), 3)                                     # an ID past n_paths
    bc, alpha, its = host.em_bootstrap(5, *csr([]), 3)                                 # n_ec = 0: the EM of no ECs
    want = em_py(5, [])
    assert bc.shape == (3, 0) and not alpha.any() and its.tolist() == [want[1]] * 3


def test_ecs_canonical(testgfa_index):
    n = testgfa_index.view.n_paths
    ecs = [((0,), 12), ((0, 1), 5), ((1, n - 1), 3), ((n - 1,), 9), ((2,), 0)]
    rev = [(tuple(reversed(i)), c) for i, c in ecs]
    half = [(i, c // 2) for i, c in rev] + [(i, c - c // 2) for i, c in rev[::-1]]
    off, ids, cnt = host.ecs_canonical(n, *csr(half))
    want = csr(sorted((i, c) for i, c in ecs if c))
    assert all(np.array_equal(x, y) for x, y in zip((off, ids, cnt), want))


@pytest.mark.parametrize("B", [1, 2, 40, 41, 100])
def test_file_equals_the_python_statistics(B, testgfa_index, tmp_path):
    idx = testgfa_index
    n = idx.view.n_paths
    assert (25 * (B - 1)) // 1000 == {1: 0, 2: 0, 40: 0, 41: 1, 100: 2}[B]
    ecs = [((0,), 120), ((0, 1), 50), ((1, n - 1), 30), ((n - 1,), 90), ((2,), 0), ((0, 1, n - 1), 400), ((1,), 40), ((3,), 25), ((2, 3), 14)]
    can = sorted((i, c) for i, c in ecs if c)
    _, alpha, _ = bootstrap_py(n, can, B, 9)
    want = stats_text(_names(idx), n, can, alpha)
    assert want.count(b"\n") >= 3 and all(ln.count(b"\t") == 7 for ln in want.splitlines())
    if B > 1:
        assert any(float(ln.split(b"\t")[5]) > 0 for ln in want.splitlines())          # a spread to print
    out = tmp_path / "a.tsv"
    rows = host.abundance_boot_from_ecs(idx, *csr(ecs[::-1]), B, seed=9, threads=4, out_path=str(out))      # computed by the library
    assert out.read_bytes() == want and len(rows) == want.count(b"\n")
    host.abundance_boot_from_ecs(idx, *csr(ecs), B, seed=9, boot_alpha=alpha, out_path=str(tmp_path / "b.tsv"))   # ready-made replicates
    assert (tmp_path / "b.tsv").read_bytes() == want
    # the first four columns are the file without bootstraps
    host.abundance_from_ecs(idx, *csr(ecs), out_path=str(tmp_path / "c.tsv"))
    assert [b"\t".join(ln.split(b"\t")[:4]) for ln in want.splitlines()] == (tmp_path / "c.tsv").read_bytes().splitlines()
    assert host.abundance_boot_from_ecs(idx, *csr(ecs), B, min_reads=1e9) == []
    host.abundance_boot_from_ecs(idx, *csr([]), B, min_reads=0.0, out_path=str(tmp_path / "e.tsv"))
    assert (tmp_path / "e.tsv").read_bytes() == b""


# ---- the device side ------------------------------------------------------------------------------------------------------

def _dev_vs_host(n_paths, ecs, n_boot, seed=1, n_draws=0, min_iter=50, max_iter=10000, threads=16):
    args = csr(ecs)
    want = host.em_bootstrap(n_paths, *args, n_boot, seed=seed, n_draws=n_draws, min_iter=min_iter, max_iter=max_iter, threads=threads)
    got = device.em_bootstrap(n_paths, *args, n_boot, seed=seed, n_draws=n_draws, min_iter=min_iter, max_iter=max_iter)
    same(got, want)
    return got


@pytest.mark.gpu
def test_device_small_cases(hip_lib):
    bc, alpha, its = _dev_vs_host(1, [((0,), 9)], 3)                                   # 1 path, 1 EC
    assert (bc == 9).all() and (alpha == 9.0).all()
    _dev_vs_host(3, [((0, 2), 0), ((1,), 10), ((0, 1, 2), 0)], 3)                      # ECs with count 0
    _dev_vs_host(2, [((0,), 7), ((1,), 3)], 3, min_iter=0)
    four = [((0, 1, 2), 1000), ((0, 1), 50), ((1, 2), 45), ((0,), 1)]
    _, _, its = _dev_vs_host(4, four, 3, min_iter=1, max_iter=100)                     # max_iter reached
    assert (its == 100).all()
    # an alpha that decays through the denormal range
    decay = [((0, 1), 10), ((0,), 1000)]
    a, it, _ = em_py(2, decay, min_iter=300)
    assert it > 300 and a[1] == 0.0
    _dev_vs_host(2, decay, 3, min_iter=300)
    bc, _, _ = _dev_vs_host(4, BIG, 4, seed=5, n_draws=20000)                          # totals above 2^40
    assert (bc.sum(axis=1) == 20000).all()
    bc, alpha, its = device.em_bootstrap(5, *csr([]), 3)                               # no ECs
    assert bc.shape == (3, 0) and not alpha.any() and its.tolist() == [em_py(5, [])[1]] * 3
    for bad in (dict(n_boot=0), dict(n_boot=3, min_iter=10, max_iter=5)):
        with pytest.raises(host.GrootError):
            device.em_bootstrap(4, *csr(four), **bad)
    with pytest.raises(host.GrootError):
        device.em_bootstrap(2, *csr([((0,), 0), ((1,), 0)]), 3)
    with pytest.raises(host.GrootError):
        device.em_bootstrap(4, *csr(four), 2, device=device.device_count())            # no such device


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 7, 0xFFFFFFFFFFFFFFF1])
def test_device_random_ecs(seed, hip_lib):
    ecs = random_ecs(3)
    n = sum(c for _, c in ecs)
    for n_draws in (0, n // 3, n + 17):
        _dev_vs_host(40, ecs, 3, seed=seed, n_draws=n_draws)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 64, 300])
def test_device_replicate_counts(B, hip_lib):
    """B = 300 is above the grid of boot_em_kernel (one workgroup per compute unit, 256 of them): workgroups take several replicates"""
    ecs = random_ecs(5, n_paths=30, n=80)
    got = _dev_vs_host(30, ecs, B, seed=2)
    if B == 3:
        same(tuple(x[:3] for x in _dev_vs_host(30, ecs, 7, seed=2)), got)


@pytest.mark.gpu
def test_device_wide_ec_and_path_in_every_ec(hip_lib):
    rng = np.random.default_rng(8)
    ecs = {(0,) + tuple(sorted(set(rng.integers(1, 600, int(rng.integers(1, 5))).tolist()))): int(rng.integers(0, 40)) for _ in range(200)}
    ecs[tuple(range(500))] = 300                                                       # one EC of 500 paths; path 0 is in every EC
    ecs = sorted(ecs.items())
    assert all(0 in i for i, _ in ecs)
    _dev_vs_host(600, ecs, 3, seed=4)


@pytest.mark.gpu
def test_device_past_both_lds_limits(hip_lib):
    """6 000 paths and 40 000 ECs: neither the cumulative table and histogram of the draws (12 bytes an EC) nor alpha and norm of the EM
    (8 bytes a path and an EC) fit the 160 KiB of LDS: the draws search global memory and count with global atomics, the EM keeps its
    arrays in global scratch"""
    rng = np.random.default_rng(12)
    n_paths, n_ec = 6000, 40000
    ecs = {}
    while len(ecs) < n_ec:
        ecs[tuple(sorted(set(rng.integers(0, n_paths, int(rng.integers(1, 5))).tolist())))] = int(rng.integers(0, 30))
    ecs = sorted(ecs.items())
    assert (len(ecs) + 1) * 8 + len(ecs) * 4 > 160 * 1024 and (n_paths + len(ecs)) * 8 > 160 * 1024
    _dev_vs_host(n_paths, ecs, 4, seed=6)


@pytest.mark.gpu
def test_device_lds_between_64_and_160_kib(hip_lib):
    """3 000 paths and 9 000 ECs: 108 KB for the draws and 96 KB for the EM, more than the 64 KiB a workgroup gets on older parts and
    less than the 160 KiB of this one: still the LDS branches"""
    rng = np.random.default_rng(13)
    n_paths, n_ec = 3000, 9000
    ecs = {}
    while len(ecs) < n_ec:
        ecs[tuple(sorted(set(rng.integers(0, n_paths, int(rng.integers(1, 5))).tolist())))] = int(rng.integers(0, 30))
    ecs = sorted(ecs.items())
    assert 64 * 1024 < (n_paths + len(ecs)) * 8 < (len(ecs) + 1) * 8 + len(ecs) * 4 < 160 * 1024
    _dev_vs_host(n_paths, ecs, 3, seed=8)


def _real_ecs(index, seed):
    multi = _multi_graph_reads(index, 200, seed + 100)
    al = device.Aligner(index, max_batch_reads=4096)
    al.ec_enable()
    first = 0
    for k in range(3):
        seq, off = O.pack_reads(clipped_reads(index, 2000, seed + k) + multi)
        al.submit(seq, off, first_read_id=first)
        al.wait()
        first += len(off) - 1
    out = al.ecs()
    al.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["argannot", "resfinder"])
def test_device_real_ecs(which, argannot_index, resfinder_index, hip_lib, monkeypatch):
    """the ECs of a run (Aligner.ecs): the device replicates == the host's, and the file from them == the file the host computes"""
    _stage(monkeypatch, "path_first")
    index = argannot_index if which == "argannot" else resfinder_index
    off, ids, cnt = _real_ecs(index, 21 if which == "argannot" else 31)
    n = index.view.n_paths
    assert len(cnt) > 10 and (np.diff(off) > 1).any()
    want = host.em_bootstrap(n, off, ids, cnt, 8, seed=3, threads=16)
    got = device.em_bootstrap(n, off, ids, cnt, 8, seed=3)
    same(got, want)
    a = host.abundance_boot_from_ecs(index, off, ids, cnt, 8, seed=3, boot_alpha=got[1])
    assert a == host.abundance_boot_from_ecs(index, off, ids, cnt, 8, seed=3, threads=16) and len(a) > 3


@pytest.mark.gpu
def test_bootstrap_beside_batches_in_flight(small_index, hip_lib, monkeypatch):
    """the device entry point called while a ctx has batches in flight on the same GPU: that ctx's counts, records and ECs are what
    they are without the call, and the call's own result is the host's"""
    _stage(monkeypatch, "path_first")
    batches = [O.pack_reads(clipped_reads(small_index, 3000, 71 + k)) for k in range(3)]
    ecs = random_ecs(3)
    want = host.em_bootstrap(40, *csr(ecs), 16, seed=2, threads=16)
    out = []
    for beside in (False, True):
        al = device.Aligner(small_index, max_batch_reads=4096, pipeline_depth=3, memo_budget_mb=device.MEMO_OFF)
        al.ec_enable()
        first = 0
        for seq, off in batches:
            al.submit(seq, off, first_read_id=first)
            first += len(off) - 1
        if beside:
            same(device.em_bootstrap(40, *csr(ecs), 16, seed=2), want)
        res = []
        for _ in batches:
            r = al.collect()
            res.append((r["counts"], np.array(r["travs"], copy=True)))
            al.release(r["ticket"])
        out.append((res, [x.copy() for x in al.ecs()]))
        al.close()
    for (c0, t0), (c1, t1) in zip(out[0][0], out[1][0]):
        assert c0 == c1 and t0.tobytes() == t1.tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(out[0][1], out[1][1]))
