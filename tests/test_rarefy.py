"""Rarefaction curves for --abundance and --calls (include/groot_host.h, "rarefaction curves").  The definition:

Input: canonical ECs (off, ids, count; groot_host_ecs_canonical), cum[0] = 0, cum[e+1] = cum[e] + count[e], N = cum[n_ec], 1 <= N < 2^62;
R >= 1 replicates; a 64-bit seed; n_depths >= 1 depths m[0] <= m[1] <= .. with 1 <= m[d] <= N.
Unit i (0 <= i < N) belongs to the EC e with cum[e] <= i < cum[e+1] (an EC with count 0 owns no unit).
sm(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)      (mod 2^64; the
        mixing steps of the bootstrap's draw)
h   = the smallest integer >= 1 with 2^(2h) >= N;  mask = 2^h - 1                       (domain 2^(2h) < 4 N for N > 4)
k_b = sm(seed + (b + 1) * 0x9E3779B97F4A7C15)
pi_b(j), 0 <= j < N:   x = j
    repeat:  L = x >> h;  Rr = x & mask
             for t = 0 .. 5:  F = sm(k_b + (((t << 32) | Rr) + 1) * 0x9E3779B97F4A7C15) >> (64 - h);   (L, Rr) = (Rr, L ^ F)
             x = (L << h) | Rr
    until x < N                                   (cycle walking: a Feistel network is a bijection of [0, 2^(2h)), so pi_b is a
                                                   bijection of [0, N) and the loop ends)
rare_count[b][d][e] = the number of j < m[d] with pi_b(j) in EC e.

alpha[b][d] = groot_host_em over rare_count[b][d], bit for bit, with its own iteration count.  The file: one line per depth step
s = 1 .. D, m_s = (N / D) * s + ((N % D) * s) / D, steps with m_s = 0 omitted: "fraction (s/D, %.4f) \\t units \\t args_mean (%.2f) \\t args_lo
\\t args_hi", args = the paths with alpha >= abundanceMin, lo / hi = v[q] and v[R-1-q] of the sorted integers, q = 25 (R - 1) / 1000; the step
s = D is the point estimate.  With calls three more columns over called = detected paths whose covered / path_len >= covCutoff.

The host library is compared with the plain-Python restatement below, the device (kernels_rare.hpp) with the host library -- in
rare_count, alpha and iterations, with tobytes(): the definition allows no tolerance."""
import bisect
import math

import numpy as np
import pytest

from groot_amd import device, host

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
E_INVALID, E_UNSUPPORTED = -1, -10        # GROOT_E_INVALID, GROOT_E_UNSUPPORTED


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def em_py(n_paths, ecs, min_iter=50, max_iter=10000):
    """em.go Run over [(ids, count)] in the order given -> (alpha, iterations)"""
    tol = math.nextafter(1.0, 2.0) - 1.0
    alpha = [1.0 / n_paths] * n_paths if n_paths else []
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
            for p in range(n_paths):
                if alpha[p] < 1e-7 / 10.0:
                    alpha[p] = 0.0
        it += 1
    return alpha, it


def csr(ecs):
    off = np.zeros(len(ecs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(i) for i, _ in ecs])
    ids = np.array([p for i, _ in ecs for p in i], dtype=np.uint32)
    return off, ids, np.array([c for _, c in ecs], dtype=np.uint64)


def sm(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def half_bits(n):
    h = 1
    while (1 << (2 * h)) < n:
        h += 1
    return h


def pi_py(seed, b, n, j, walks=None):
    h = half_bits(n)
    mask = (1 << h) - 1
    k = sm((seed + (b + 1) * GOLD) & M64)
    x = j
    while True:
        left, right = x >> h, x & mask
        for t in range(6):
            f = sm((k + (((t << 32) | right) + 1) * GOLD) & M64) >> (64 - h)
            left, right = right, left ^ f
        x = (left << h) | right
        if walks is not None:
            walks[0] += 1
        if x < n:
            return x


def counts_py(counts, n_rep, depths, seed):
    """rare_count[b][d][e] in plain Python"""
    cum = [0]
    for c in counts:
        cum.append(cum[-1] + int(c))
    n = cum[-1]
    out = []
    for b in range(n_rep):
        rows = []
        for m in depths:
            row = [0] * len(counts)
            for j in range(int(m)):                       # every depth from its own definition: no running count to get wrong
                row[bisect.bisect_right(cum, pi_py(seed, b, n, j)) - 1] += 1
            rows.append(row)
        out.append(rows)
    return out


def rarefy_py(n_paths, ecs, n_rep, depths, seed, min_iter=50, max_iter=10000):
    rc = counts_py([c for _, c in ecs], n_rep, depths, seed)
    alpha, its = [], []
    for rows in rc:
        for row in rows:
            a, it = em_py(n_paths, [(ids, c) for (ids, _), c in zip(ecs, row)], min_iter, max_iter)
            alpha.append(a)
            its.append(it)
    D = len(depths)
    return (np.array(rc, dtype=np.uint64).reshape(n_rep, D, len(ecs)), np.array(alpha, dtype=np.float64).reshape(n_rep, D, n_paths),
            np.array(its, dtype=np.uint32).reshape(n_rep, D))


def same(got, want):
    """rare_count, alpha, iterations: bit for bit"""
    for g, w, what in zip(got, want, ("rare_count", "alpha", "iterations")):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint64 if g.dtype.itemsize == 8 else np.uint32) != w.view(np.uint64 if w.dtype.itemsize == 8 else np.uint32))
            raise AssertionError(f"{what}: {len(bad)} difference(s), the first at {bad[0].tolist()}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}")


def invariants(rc, count, depths):
    count = np.asarray(count, dtype=np.uint64)
    assert (rc.sum(axis=2) == np.asarray(depths, dtype=np.uint64)[None, :]).all()                  # the sum over e is m[d]
    assert (rc[:, :-1, :] <= rc[:, 1:, :]).all() and (rc <= count[None, None, :]).all()            # nested, within count
    for d, m in enumerate(depths):
        if m == count.sum():
            assert (rc[:, d, :] == count[None, :]).all()                                           # m[d] = N gives count exactly


SMALL_N = [1, 2, 3, 4, 5, 16, 17, 4096, 4097]          # where h steps (4 -> 5, 16 -> 17, 4096 -> 4097) and where walking never (N = 4, 16, 4096) happens


def ecs_of_total(n):
    """n units over up to three live ECs of four paths, count-0 classes between them"""
    k = min(n, 3)
    parts = [n // k + (n % k if i == 0 else 0) for i in range(k)] + [0] * (3 - k)
    return [((0,), parts[0]), ((0, 1), 0), ((1, 2), parts[1]), ((1, 3), 0), ((2,), 0), ((2, 3), parts[2])]


def depths_of_total(n):
    a = max(1, n // 3)
    return [1, a, a, max(a, 2 * n // 3), n]             # 1 and N, and equal neighbours


BIG = [((0, 1), 1 << 39), ((1,), 3), ((0, 2), 1 << 39), ((2, 3), 0), ((3,), 0)]      # N = 2^40 + 3: unit indices past 2^32
BIG_DEPTHS = [1000, 5000]


def random_ecs(seed, n_paths=40, n=300, max_len=6, max_count=50):
    rng = np.random.default_rng(seed)
    ecs = {tuple(sorted(set(rng.integers(0, n_paths, int(rng.integers(1, max_len))).tolist()))): int(rng.integers(0, max_count)) for _ in range(n)}
    assert any(c == 0 for c in ecs.values())
    return sorted(ecs.items())


def many_ecs(seed, n_paths, n_ec, max_count):
    rng = np.random.default_rng(seed)
    ecs = {}
    while len(ecs) < n_ec:
        ecs[tuple(sorted(set(rng.integers(0, n_paths, int(rng.integers(1, 5))).tolist())))] = int(rng.integers(0, max_count))
    return sorted(ecs.items())


# ---- host against Python, no GPU ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16, 17, 1000, 4097])
def test_pi_is_a_permutation(n):
    walks = [0]
    image = sorted(pi_py(7, 1, n, j, walks) for j in range(n))
    assert image == list(range(n)) and walks[0] < 4 * n + 64
    if n in (4, 16):
        assert walks[0] == n                                # the domain is [0, N): no walk
    assert half_bits(n) == {1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 16: 2, 17: 3, 1000: 5, 4097: 7}[n]


@pytest.mark.parametrize("n", SMALL_N)
def test_host_equals_python(n):
    ecs, depths = ecs_of_total(n), depths_of_total(n)
    assert sum(c for _, c in ecs) == n and depths[0] == 1 and depths[-1] == n and depths[1] == depths[2]
    got = host.em_rarefy(4, *csr(ecs), 2, depths, seed=3)
    same(got, rarefy_py(4, ecs, 2, depths, 3))
    invariants(got[0], [c for _, c in ecs], depths)
    zero = np.array([c == 0 for _, c in ecs])
    assert not got[0][:, :, zero].any()                     # an EC with count 0 owns no unit


def test_host_equals_python_one_ec():
    same(host.em_rarefy(2, *csr([((0, 1), 9)]), 3, [1, 4, 9], seed=1), rarefy_py(2, [((0, 1), 9)], 3, [1, 4, 9], 1))
    rc, alpha, _ = host.em_rarefy(1, *csr([((0,), 9)]), 3, [1, 4, 9], seed=1)
    assert rc.reshape(3, 3).tolist() == [[1, 4, 9]] * 3 and alpha.reshape(3, 3).tolist() == [[1.0, 4.0, 9.0]] * 3


@pytest.mark.parametrize("seed", [1, 7, 0xFFFFFFFFFFFFFFF1])
def test_host_equals_python_on_random_ecs(seed):
    ecs = random_ecs(3, n=60, max_count=12)
    n = sum(c for _, c in ecs)
    depths = [1, n // 4, n // 2, n // 2, n]
    same(host.em_rarefy(40, *csr(ecs), 2, depths, seed=seed), rarefy_py(40, ecs, 2, depths, seed))


def test_host_equals_python_above_2_40():
    assert sum(c for _, c in BIG) == (1 << 40) + 3
    got = host.em_rarefy(4, *csr(BIG), 2, BIG_DEPTHS, seed=5)
    same(got, rarefy_py(4, BIG, 2, BIG_DEPTHS, 5))
    invariants(got[0], [c for _, c in BIG], BIG_DEPTHS)
    assert got[0][:, 1, 0].min() > 2000 and got[0][:, 1, 2].min() > 2000


def test_properties():
    ecs = random_ecs(11)
    count = [c for _, c in ecs]
    n = sum(count)
    args = csr(ecs)
    depths = [1, n // 10, n // 3, n // 3, n - 1, n]
    r7 = host.em_rarefy(40, *args, 7, depths, seed=3)
    invariants(r7[0], count, depths)
    same(host.em_rarefy(40, *args, 3, depths, seed=3), tuple(x[:3] for x in r7))                   # R = 3 is the prefix of R = 7
    for d in (0, 2, 4):                                                                            # a depth alone == inside the longer list
        same(host.em_rarefy(40, *args, 7, [depths[d]], seed=3), tuple(x[:, d:d + 1] for x in r7))
    for threads in (3, 16):
        same(host.em_rarefy(40, *args, 7, depths, seed=3, threads=threads), r7)
    mid = [r.tobytes() for r in r7[0][:, 2, :]]
    assert len(set(mid)) == 7                                                                      # the replicates differ from each other
    others = [host.em_rarefy(40, *args, 1, depths, seed=s)[0][0, 2].tobytes() for s in (4, 0xFFFFFFFFFFFFFFF1)]
    assert len({mid[0], *others}) == 3                                                             # three seeds, three subsamples
    assert (r7[1][:, -1, :] == r7[1][0, -1, :]).all()                                              # at m = N every replicate is the point estimate
    a, it = em_py(40, ecs)
    assert r7[1][0, -1].tobytes() == np.array(a).tobytes() and (r7[2][:, -1] == it).all()


def _invalid(fn):
    ecs = [((0,), 4), ((0, 1), 2)]
    args = csr(ecs)
    bad = [
        lambda: fn(2, *args, 0, [1, 6]),                                       # n_rep = 0
        lambda: fn(2, *args, 3, []),                                           # n_depths = 0
        lambda: fn(2, *args, 3, [0, 6]),                                       # a depth of 0
        lambda: fn(2, *args, 3, [1, 7]),                                       # a depth above N
        lambda: fn(2, *args, 3, [3, 2]),                                       # depths that descend
        lambda: fn(2, *csr([((0,), 0), ((1,), 0)]), 3, [1]),                   # N = 0
        lambda: fn(2, *csr([]), 3, [1]),                                       # N = 0: no ECs at all
        lambda: fn(2, *args, 3, [1, 6], min_iter=10, max_iter=5),              # the EM's own errors
        lambda: fn(2, *args, 3, [1, 6], min_iter=0, max_iter=0),
        lambda: fn(2, *csr([((2,), 1)]), 3, [1]),                              # an ID past n_paths
    ]
    for call in bad:
        with pytest.raises(host.GrootError) as e:
            call()
        assert e.value.code == E_INVALID
    with pytest.raises(host.GrootError) as e:
        fn(2, *csr([((0,), 1 << 61), ((0, 1), 1 << 61)]), 3, [1])              # N = 2^62
    assert e.value.code == E_UNSUPPORTED
    fn(2, *args, 3, [1, 6])


def test_invalid_arguments():
    _invalid(host.em_rarefy)


def test_step_depths():
    for n, D in ((21, 10), (3, 10), (9_970_000, 10), ((1 << 40) + 3, 7), (5, 1), (0, 4)):
        want = [(n // D) * s + ((n % D) * s) // D for s in range(1, D + 1)]
        assert host.rarefy_depths(n, D).tolist() == want and want[-1] == n
    with pytest.raises(host.GrootError):
        host.rarefy_depths(5, 0)


def columns_py(v, R):
    """mean in replicate order, v[q] and v[R-1-q] of the sorted integers"""
    s = 0.0
    for x in v:
        s += float(x)
    w, q = sorted(v), (25 * (R - 1)) // 1000
    return "\t%.2f\t%d\t%d" % (s / R, w[q], w[R - 1 - q])


def file_py(n_paths, ecs, R, D, alpha, min_reads, called=None, called_all=None):
    """the expected file from alpha[R][K][n_paths] at the drawn depths (and called[R][K], with the point estimate's count)"""
    n = sum(c for _, c in ecs)
    m = [(n // D) * s + ((n % D) * s) // D for s in range(1, D + 1)]
    point, _ = em_py(n_paths, ecs)
    out, k = "", 0
    for s in range(1, D + 1):
        if m[s - 1] == 0:
            continue
        out += "%.4f\t%d" % (s / D, m[s - 1])
        if s < D:
            out += columns_py([sum(1 for p in range(n_paths) if alpha[b][k][p] >= min_reads) for b in range(R)], R)
            if called is not None:
                out += columns_py([int(called[b][k]) for b in range(R)], R)
            k += 1
        else:
            a = sum(1 for p in range(n_paths) if point[p] >= min_reads)
            out += "\t%.2f\t%d\t%d" % (a, a, a)
            if called is not None:
                out += "\t%.2f\t%d\t%d" % (called_all, called_all, called_all)
        out += "\n"
    return out.encode()


@pytest.mark.parametrize("R", [1, 20, 41])
def test_writer_on_hand_made_alphas(R, testgfa_index, tmp_path):
    idx = testgfa_index
    n = idx.view.n_paths
    assert (25 * (R - 1)) // 1000 == {1: 0, 20: 0, 41: 1}[R]
    ecs = sorted({(0,): 120, (0, 1): 50, (1, n - 1): 30, (n - 1,): 90, (0, 1, n - 1): 400, (1,): 40, (3,): 25, (2, 3): 14}.items())
    D, K = 10, 9
    rng = np.random.default_rng(R)
    alpha = rng.choice([0.0, 0.5, 0.999999, 1.0, 3.25, 80.0], size=(R, K, n))       # hand-made: values on both sides of and at abundanceMin
    out = tmp_path / "r.tsv"
    lines = host.rarefy_from_ecs(idx, *csr(ecs[::-1]), str(out), n_rep=R, n_steps=D, rare_alpha=alpha)
    want = file_py(n, ecs, R, D, alpha, 1.0)
    assert out.read_bytes() == want and lines == D and all(ln.count(b"\t") == 4 for ln in want.splitlines())
    if R > 1:
        assert any(ln.split(b"\t")[3] != ln.split(b"\t")[4] for ln in want.splitlines())           # an interval to print
    assert host.rarefy_from_ecs(idx, *csr(ecs), str(out), n_rep=R, n_steps=D, rare_alpha=alpha, min_reads=3.25) == D
    assert out.read_bytes() == file_py(n, ecs, R, D, alpha, 3.25)
    # computed inside == the library's replicates handed in; the last line is the abundance file's line count
    total = sum(c for _, c in ecs)
    drawn = host.rarefy_depths(total, D)[:-1]
    _, ra, _ = host.em_rarefy(n, *csr(ecs), R, drawn, seed=9, threads=4)
    host.rarefy_from_ecs(idx, *csr(ecs), str(out), n_rep=R, n_steps=D, seed=9, threads=4)
    assert out.read_bytes() == file_py(n, ecs, R, D, ra, 1.0)
    host.abundance_from_ecs(idx, *csr(ecs), out_path=str(tmp_path / "a.tsv"))
    n_ab = len((tmp_path / "a.tsv").read_bytes().splitlines())
    assert out.read_bytes().splitlines()[-1] == b"1.0000\t%d\t%.2f\t%d\t%d" % (total, n_ab, n_ab, n_ab)


def test_writer_omits_steps_without_units(testgfa_index, tmp_path):
    idx = testgfa_index
    n = idx.view.n_paths
    ecs = [((0,), 2), ((0, 1), 1)]                                                  # N = 3, D = 10: m = 0 0 0 1 1 1 2 2 2 3
    out = tmp_path / "r.tsv"
    assert host.rarefy_from_ecs(idx, *csr(ecs), str(out), n_rep=3, n_steps=10, seed=2, min_reads=0.5) == 7
    _, ra, _ = host.em_rarefy(n, *csr(ecs), 3, [1, 1, 1, 2, 2, 2], seed=2)
    want = file_py(n, ecs, 3, 10, ra, 0.5)
    assert out.read_bytes() == want and want.startswith(b"0.4000\t1\t") and len(want.splitlines()) == 7
    assert host.rarefy_from_ecs(idx, *csr(ecs), str(out), n_rep=3, n_steps=1) == 1 and out.read_bytes() == file_py(n, ecs, 3, 1, None, 1.0)
    assert host.rarefy_from_ecs(idx, *csr([]), str(out), n_rep=3, n_steps=10) == 0 and out.read_bytes() == b""
    for bad in (dict(n_rep=0), dict(n_steps=0)):
        with pytest.raises(host.GrootError) as e:
            host.rarefy_from_ecs(idx, *csr(ecs), str(out), **{**dict(n_rep=3, n_steps=10), **bad})
        assert e.value.code == E_INVALID


def _called_py(idx, table, rc, ra, min_reads, call_depth, cov_cutoff, threads=2):
    """called[R][K] from host.call_support (checked against its own restatement in test_call_support.py) fed as the definition says"""
    from test_calls import _lens
    n, lens = idx.view.n_paths, _lens(idx)
    off, ids, cnt, rows, tn = table.arrays()
    R, K = ra.shape[:2]
    sel = [p for p in range(n) if (ra[:, :, p] >= min_reads).any()]
    cov = host.call_support(n, lens, off, ids, cnt, rows, tn, rc.reshape(R * K, -1), ra.reshape(R * K, n), sel, call_depth=call_depth, threads=threads)
    cov = cov.reshape(R, K, len(sel))
    called = [[sum(1 for i, p in enumerate(sel) if ra[b, k, p] >= min_reads and float(cov[b, k, i]) / float(lens[p]) >= cov_cutoff) for k in range(K)]
              for b in range(R)]
    return sel, cov, called


@pytest.mark.parametrize("R", [1, 20])
def test_writer_with_calls(R, testgfa_index, tmp_path):
    from test_calls import _hand_table
    idx = testgfa_index
    n = idx.view.n_paths
    t = _hand_table(idx)
    off, ids, cnt, rows, tn = t.arrays()
    total, D = int(cnt.sum()), 10
    drawn = host.rarefy_depths(total, D)[:-1]
    assert total == 21 and drawn.min() > 0
    out = tmp_path / "r.tsv"
    called_hi = []
    for depth, cut, min_reads in ((1.0, 0.05, 1.0), (2.0, 0.05, 0.0), (0.5, 0.5, 1.0)):
        rc, ra, _ = host.em_rarefy(n, off, ids, cnt, R, drawn, seed=4)
        sel, cov, called = _called_py(idx, t, rc, ra, min_reads, depth, cut)
        host.calls_from_table(idx, off, ids, cnt, rows, tn, str(tmp_path / "c.tsv"), min_reads=min_reads, call_depth=depth, cov_cutoff=cut)
        called_all = sum(ln.endswith(b"\t1") for ln in (tmp_path / "c.tsv").read_bytes().splitlines())
        want = file_py(n, t.ecs, R, D, ra, min_reads, called, called_all)
        kw = dict(n_rep=R, n_steps=D, seed=4, min_reads=min_reads, tuples=rows, tn=tn, call_depth=depth, cov_cutoff=cut)
        assert host.rarefy_from_ecs(idx, off, ids, cnt, str(out), threads=3, **kw) == D                                 # everything computed inside
        assert out.read_bytes() == want and all(ln.count(b"\t") == 7 for ln in want.splitlines())
        host.rarefy_from_ecs(idx, off, ids, cnt, str(out), rare_count=rc, rare_alpha=ra, **kw)                            # ready-made replicates
        assert out.read_bytes() == want
        host.rarefy_from_ecs(idx, off, ids, cnt, str(out), rare_alpha=ra, covered=cov.reshape(R * len(drawn), len(sel)), **kw)   # ... and covered counts
        assert out.read_bytes() == want
        # the first five columns are the file without calls
        host.rarefy_from_ecs(idx, off, ids, cnt, str(tmp_path / "five.tsv"), n_rep=R, n_steps=D, seed=4, min_reads=min_reads)
        assert [b"\t".join(ln.split(b"\t")[:5]) for ln in want.splitlines()] == (tmp_path / "five.tsv").read_bytes().splitlines()
        called_hi.append([int(ln.split(b"\t")[7]) for ln in want.splitlines()])
    assert called_hi[0][-1] > 0 and called_hi[0][0] < called_hi[0][-1]                                                     # the called curve rises
    with pytest.raises(host.GrootError):
        host.rarefy_from_ecs(idx, off, ids, cnt, str(out), rare_alpha=ra, covered=np.zeros((R * len(drawn), len(sel) + 1)), **kw)
    with pytest.raises(host.GrootError):
        host.rarefy_from_ecs(idx, off, ids, cnt, str(out), **{**kw, "cov_cutoff": 1.5})


# ---- the device against the host library --------------------------------------------------------------------------------------

def _dev_vs_host(n_paths, ecs, n_rep, depths, seed=1, min_iter=50, max_iter=10000, threads=16):
    args = csr(ecs)
    want = host.em_rarefy(n_paths, *args, n_rep, depths, seed=seed, min_iter=min_iter, max_iter=max_iter, threads=threads)
    got = device.em_rarefy(n_paths, *args, n_rep, depths, seed=seed, min_iter=min_iter, max_iter=max_iter)
    same(got, want)
    return got


@pytest.mark.gpu
def test_device_small_totals(hip_lib):
    for n in SMALL_N:
        ecs, depths = ecs_of_total(n), depths_of_total(n)
        rc, _, _ = _dev_vs_host(4, ecs, 2, depths, seed=3)
        invariants(rc, [c for _, c in ecs], depths)
    _dev_vs_host(2, [((0, 1), 9)], 3, [1, 4, 9])                                       # one EC
    _dev_vs_host(1, [((0,), 9)], 3, [9])
    _dev_vs_host(4, ecs_of_total(17), 3, [1, 17], min_iter=0, max_iter=3)              # max_iter reached
    _invalid(device.em_rarefy)
    with pytest.raises(host.GrootError):
        device.em_rarefy(4, *csr(ecs_of_total(17)), 2, [1], device=device.device_count())          # no such device


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 7, 0xFFFFFFFFFFFFFFF1])
def test_device_random_ecs_and_properties(seed, hip_lib):
    ecs = random_ecs(11)
    count = [c for _, c in ecs]
    n = sum(count)
    depths = [1, n // 10, n // 3, n // 3, n - 1, n]
    r7 = _dev_vs_host(40, ecs, 7, depths, seed=seed)
    invariants(r7[0], count, depths)
    same(device.em_rarefy(40, *csr(ecs), 3, depths, seed=seed), tuple(x[:3] for x in r7))          # R = 3 is the prefix of R = 7
    same(device.em_rarefy(40, *csr(ecs), 7, [depths[2]], seed=seed), tuple(x[:, 2:3] for x in r7))  # a depth alone


@pytest.mark.gpu
def test_device_chunk_edges(hip_lib):
    """N = 50 000: depths at a workgroup's chunk of 16 384 draws, one below and one above it, an interval of one draw and one of a single unit"""
    ecs = many_ecs(21, 50, 400, 201)
    count = [c for _, c in ecs]
    count[-1] += 50_000 - sum(count)
    ecs = [(i, c) for (i, _), c in zip(ecs, count)]
    assert sum(count) == 50_000 and min(count) >= 0
    depths = [1, 16383, 16384, 16385, 40000]
    rc, _, _ = _dev_vs_host(50, ecs, 3, depths, seed=5)
    invariants(rc, count, depths)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 3, 64, 300])
def test_device_replicate_counts(R, hip_lib):
    """R = 300 with two depths: 600 count vectors, above the grid of boot_em_kernel (one workgroup per compute unit)"""
    ecs = random_ecs(5, n_paths=30, n=80)
    n = sum(c for _, c in ecs)
    _dev_vs_host(30, ecs, R, [n // 2, n], seed=2)


@pytest.mark.gpu
@pytest.mark.parametrize("n_ec", [9000, 40000])
def test_device_lds_and_global_branch(n_ec, hip_lib):
    """9 000 ECs: cum and the histogram (12 n_ec + 8 bytes) in LDS; 40 000 ECs: the global branch.  N about 10^5."""
    n_paths = 3000 if n_ec == 9000 else 6000
    ecs = many_ecs(13, n_paths, n_ec, 24 if n_ec == 9000 else 6)
    n = sum(c for _, c in ecs)
    assert 70_000 < n < 130_000 and (12 * n_ec + 8 <= 160 * 1024) == (n_ec == 9000)
    depths = [n // 10, n // 2, n]
    rc, _, _ = _dev_vs_host(n_paths, ecs, 3, depths, seed=8)
    invariants(rc, [c for _, c in ecs], depths)


@pytest.mark.gpu
def test_device_above_2_40(hip_lib):
    rc, _, _ = _dev_vs_host(4, BIG, 2, BIG_DEPTHS, seed=5)
    invariants(rc, [c for _, c in BIG], BIG_DEPTHS)


@pytest.mark.gpu
def test_device_real_ecs(argannot_index, hip_lib, monkeypatch, tmp_path):
    """the ECs of the arg-annot run the bootstrap tests use: the device replicates == the host's, and the file from them == the host's"""
    from test_bootstrap import _real_ecs
    from test_coverage import _stage
    _stage(monkeypatch, "path_first")
    index = argannot_index
    off, ids, cnt = _real_ecs(index, 21)
    n = index.view.n_paths
    assert len(cnt) > 10 and (np.diff(off) > 1).any()
    drawn = host.rarefy_depths(int(cnt.sum()), 10)[:-1]
    want = host.em_rarefy(n, off, ids, cnt, 8, drawn, seed=3, threads=16)
    got = device.em_rarefy(n, off, ids, cnt, 8, drawn, seed=3)
    same(got, want)
    assert host.rarefy_from_ecs(index, off, ids, cnt, str(tmp_path / "d.tsv"), n_rep=8, seed=3, rare_alpha=got[1]) == 10
    host.rarefy_from_ecs(index, off, ids, cnt, str(tmp_path / "h.tsv"), n_rep=8, seed=3, threads=16)
    rows = [ln.split(b"\t") for ln in (tmp_path / "d.tsv").read_bytes().splitlines()]
    assert (tmp_path / "d.tsv").read_bytes() == (tmp_path / "h.tsv").read_bytes() and float(rows[0][2]) < float(rows[-1][2])


@pytest.mark.gpu
def test_rarefy_beside_batches_in_flight(small_index, hip_lib, monkeypatch):
    """the device entry point called while a ctx has batches in flight on the same GPU: that ctx's counts, records and ECs are what
    they are without the call, and the call's own result is the host's"""
    from oracle import oracle_py as O
    from test_coverage import _stage, clipped_reads
    _stage(monkeypatch, "path_first")
    batches = [O.pack_reads(clipped_reads(small_index, 3000, 71 + k)) for k in range(3)]
    ecs = random_ecs(3)
    n = sum(c for _, c in ecs)
    depths = [n // 4, n // 2, n]
    want = host.em_rarefy(40, *csr(ecs), 8, depths, seed=2, threads=16)
    out = []
    for beside in (False, True):
        al = device.Aligner(small_index, max_batch_reads=4096, pipeline_depth=3, memo_budget_mb=device.MEMO_OFF)
        al.ec_enable()
        first = 0
        for seq, off in batches:
            al.submit(seq, off, first_read_id=first)
            first += len(off) - 1
        if beside:
            same(device.em_rarefy(40, *csr(ecs), 8, depths, seed=2), want)
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
