"""Assigned coverage (`--calls`): the pileup of the reads the abundance EM assigns to each path.  The definition, quoted from
include/groot_hip.h:

  S(r), equivalence classes (ECs), their canonical order and alpha = groot_host_em over the run's ECs: exactly as for --abundance.
  For an EC e (ascending path IDs) and p in e:   w(e,p) = alpha[p] / denom(e),  denom(e) = sum of alpha[q], q in e, in ID order;
                                                 w(e,p) = 0.0 where the EM skips e (denom < 2^-52).  Double, no FMA contraction.
  A record of read r on path p with an M op of M bases at Pos covers [Pos, last], last = min(Pos + M, path_len(p) - 1), both ends
  included: the interval `report` piles up.  EVERY record counts (both strands, primary and secondary), as in the report.
  The assigned-coverage table of a run is the multiset of records grouped by (e = EC of S(r), p, Pos, last):  n(e,p,Pos,last), integers.
  Per path p, per EC e holding p:  d_e[x] = number of records of (e,p,.,.) covering base x   (integers).
  Assigned depth:  D_p[x] = sum over the ECs holding p, in canonical EC order, of (double)d_e[x] * w(e,p).
  A base is covered when D_p[x] >= callDepth (default 1.0).  breadth = covered / path_len;  depth = (sum of D_p[x] in x order) / path_len.

Everything below restates that in plain Python / numpy on the CPU oracle's expanded records: the host library (groot_host_acov_merge,
groot_host_acov_depth, groot_host_calls_from_table, groot_host_report_calls) and the device table (Aligner.acov, kernels_acov.hpp) must
equal it exactly -- tuple lists as sorted integer arrays, D_p by tobytes(), files as bytes.  No tolerance anywhere."""
import math

import numpy as np
import pytest

from bamread import read_bam
from groot_amd import device, host
from test_abundance import _names, csr, ecs_of_alns, em_py
from test_counter_edges import L, _bad_batch, _build_case, _feed, _feed_pipelined, _of_reads, _CODE
from test_coverage import STAGES, _stage, clipped_reads
from test_shared_reads import _oracle_alns

TOL = math.nextafter(1.0, 2.0) - 1.0


# ---- the restatement ----------------------------------------------------------------------------------------------------------

class Table:
    """ECs in canonical order [(ids, reads)] and the tuples: rows (EC index, path, Pos, last) ascending, n per row"""

    def __init__(self, ecs, rows, n):
        self.ecs, self.rows, self.n = list(ecs), np.asarray(rows, dtype=np.int64).reshape(-1, 4), np.asarray(n, dtype=np.int64)

    def arrays(self):
        return csr(self.ecs) + (self.rows.astype(np.uint32), self.n.astype(np.uint64))


def _group(rows, n):
    """equal rows summed, ascending"""
    rows, n = np.asarray(rows, dtype=np.int64).reshape(-1, 4), np.asarray(n, dtype=np.int64)
    if not len(rows):
        return rows, n
    u, inv = np.unique(rows, axis=0, return_inverse=True)
    return u, np.bincount(inv.reshape(-1), weights=n, minlength=len(u)).astype(np.int64)


def table_of_alns(index, alns, seq_off):
    """the assigned-coverage table of one batch's expanded records (read ids relative to seq_off)"""
    lens = index.arrays["path_len"].astype(np.int64)
    off = np.asarray(seq_off, dtype=np.int64)
    rid, ref, pos = alns["read_id"].astype(np.int64), alns["ref_id"].astype(np.int64), alns["pos"].astype(np.int64)
    m = (off[rid + 1] - off[rid]) - alns["start_clip"].astype(np.int64) - alns["end_clip"].astype(np.int64)
    last = np.minimum(pos + m, lens[ref] - 1)
    ecs = ecs_of_alns(alns)
    ec_index = {ids: i for i, (ids, _) in enumerate(ecs)}
    rr = np.unique(rid * (1 << 20) + ref)
    r, p = rr >> 20, rr & ((1 << 20) - 1)
    starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]]) if len(r) else np.zeros(0, dtype=np.int64)
    ec_of_read = {int(r[s]): ec_index[tuple(p[s:e].tolist())] for s, e in zip(starts, np.r_[starts[1:], len(r)])}
    e = np.array([ec_of_read[int(x)] for x in rid], dtype=np.int64)
    return Table(ecs, *_group(np.stack([e, ref, pos, last], axis=1) if len(rid) else np.zeros((0, 4)), np.ones(len(rid), dtype=np.int64)))


def merge_tables(tables):
    """several tables -> one: ECs canonical with counts summed, tuples renumbered, equal keys summed"""
    count = {}
    for t in tables:
        for ids, c in t.ecs:
            count[ids] = count.get(ids, 0) + c
    ecs = sorted(count.items())
    index = {ids: i for i, (ids, _) in enumerate(ecs)}
    rows, n = [np.zeros((0, 4), dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for t in tables:
        remap = np.array([index[ids] for ids, _ in t.ecs], dtype=np.int64)
        if len(t.rows):
            x = t.rows.copy()
            x[:, 0] = remap[x[:, 0]]
            rows.append(x)
            n.append(t.n)
    return Table(ecs, *_group(np.concatenate(rows), np.concatenate(n)))


def weight_py(ecs, alpha, e, p):
    denom = 0.0
    for q in ecs[e][0]:
        denom += alpha[q]
    if denom < TOL:
        return 0.0
    return alpha[p] / denom


def depth_py(table, alpha, p, length):
    """D_p as a list of Python floats: per EC holding p, in canonical order, the integer d_e, then D += float(d_e) * w"""
    D = [0.0] * length
    rows, n = table.rows, table.n
    for e in sorted(set(rows[rows[:, 1] == p][:, 0].tolist())):
        diff = [0] * (length + 1)
        for (_, _, pos, last), k in zip(rows[(rows[:, 0] == e) & (rows[:, 1] == p)].tolist(), n[(rows[:, 0] == e) & (rows[:, 1] == p)].tolist()):
            if pos >= length or last < pos:
                continue
            diff[pos] += k
            diff[min(last, length - 1) + 1] -= k
        w = weight_py(table.ecs, alpha, e, p)
        d = 0
        for x in range(length):
            d += diff[x]
            D[x] = D[x] + float(d) * w
    return D


def cigar_py(cov):
    """the report's run-length string (reporting.go:178-213) over a 0/1 list"""
    if not cov:
        return ""
    out, counter, pre, sym = "", 1, cov[0], "DM"
    for i in range(1, len(cov)):
        val = cov[i]
        if i == len(cov) - 1:
            if val == pre:
                out += "%d%s" % (counter + 1, sym[val])
            else:
                out += "%d%s1%s" % (counter, sym[pre], sym[val])
            break
        if val == pre:
            counter += 1
        else:
            out += "%d%s" % (counter, sym[pre])
            pre, counter = val, 1
    return out


def calls_text(names, lens, table, alpha=None, min_reads=1.0, call_depth=1.0, cov_cutoff=0.97):
    """the expected file"""
    if not table.ecs:
        return b""
    if alpha is None:
        alpha, _, _ = em_py(len(names), table.ecs)
    out = ""
    for p in range(len(names)):
        if not alpha[p] >= min_reads:
            continue
        length = int(lens[p])
        D = depth_py(table, alpha, p, length)
        cov = [1 if d >= call_depth else 0 for d in D]
        total = 0.0
        for d in D:
            total += d
        breadth, depth = sum(cov) / length, total / length
        nm = names[p][1:] if names[p].startswith("*") else names[p]
        out += "%s\t%.2f\t%d\t%.2f\t%.4f\t%s\t%d\n" % (nm, alpha[p], length, depth, breadth, cigar_py(cov), 1 if breadth >= cov_cutoff else 0)
    return out.encode()


def _lens(index):
    return index.arrays["path_len"].astype(np.int64)


def _write(index, table, path, **kw):
    return host.calls_from_table(index, *table.arrays(), out_path=str(path), **kw)


def _depth_lib(index, table, alpha, p):
    off, ids, _, rows, n = table.arrays()
    return host.acov_depth(index.view.n_paths, off, ids, alpha, rows, n, p, int(_lens(index)[p]))


# ---- host, no GPU ---------------------------------------------------------------------------------------------------------------

def _hand_table(index):
    """ECs over the first paths of the index and tuples that meet every clause of the definition once"""
    n, lens = index.view.n_paths, _lens(index)
    assert n >= 4 and lens[:4].min() >= 40
    last0 = int(lens[0]) - 1
    ecs = sorted({(0,): 7, (0, 1): 5, (0, 1, 2): 3, (0, 3): 2, (0, 2, 3): 4}.items())       # path 0 is in every EC
    e = {ids: i for i, (ids, _) in enumerate(ecs)}
    rows = [
        (e[(0,)], 0, 0, 20), (e[(0,)], 0, 5, 25),
        (e[(0, 1)], 0, 10, 30), (e[(0, 1)], 1, 10, 30),
        (e[(0, 1)], 0, 12, 33),                                   # a read with two records on one path (one on each strand), at different Pos
        (e[(0, 1, 2)], 0, last0 - 10, last0), (e[(0, 1, 2)], 2, 3, 31),      # a record clipped at path_len - 1
        (e[(0, 3)], 0, 15, 18), (e[(0, 3)], 3, 0, 28), (e[(0, 2, 3)], 3, 2, 30),
    ]
    n_rec = [3, 1, 2, 2, 2, 1, 1, 4, 4, 1]
    order = sorted(range(len(rows)), key=lambda i: rows[i])
    return Table(ecs, [rows[i] for i in order], [n_rec[i] for i in order])


def test_hand_made_table_against_the_restatement(testgfa_index, tmp_path):
    idx = testgfa_index
    n, lens, names = idx.view.n_paths, _lens(idx), _names(idx)
    t = _hand_table(idx)
    alpha, _, _ = em_py(n, t.ecs)
    for p in range(4):
        D = depth_py(t, alpha, p, int(lens[p]))
        assert _depth_lib(idx, t, alpha, p).tobytes() == np.array(D, dtype=np.float64).tobytes()
        assert p != 0 or max(D) > 0
    for depth in (1.0, 0.5, 2.0):
        for cut in (0.97, 0.1):
            want = calls_text(names, lens, t, call_depth=depth, cov_cutoff=cut, min_reads=0.0)
            lines, called = _write(idx, t, tmp_path / "c.tsv", call_depth=depth, cov_cutoff=cut, min_reads=0.0)
            assert (tmp_path / "c.tsv").read_bytes() == want and lines == want.count(b"\n") > 1
            assert called == sum(ln.endswith(b"\t1") for ln in want.splitlines())
    # callDepth decides: a lower one covers more
    b = [float(ln.split(b"\t")[4]) for ln in calls_text(names, lens, t, call_depth=0.5, min_reads=0.0).splitlines()]
    a = [float(ln.split(b"\t")[4]) for ln in calls_text(names, lens, t, call_depth=2.0, min_reads=0.0).splitlines()]
    assert all(x >= y for x, y in zip(b, a)) and sum(b) > sum(a)
    # alpha handed in == alpha computed inside
    _write(idx, t, tmp_path / "d.tsv", alpha=np.array(alpha), min_reads=0.0)
    assert (tmp_path / "d.tsv").read_bytes() == calls_text(names, lens, t, min_reads=0.0)
    # an empty table: an empty file
    assert _write(idx, Table([], [], []), tmp_path / "e.tsv") == (0, 0) and (tmp_path / "e.tsv").read_bytes() == b""
    # a tuple whose path is not in its EC, or whose EC is not in the list
    for bad in ((0, 3, 0, 5), (len(t.ecs), 0, 0, 5)):
        with pytest.raises(host.GrootError):
            _write(idx, Table(t.ecs, [bad], [1]), tmp_path / "f.tsv")


def test_an_ec_the_em_skips_weighs_nothing(testgfa_index, tmp_path):
    """alpha of both paths of an EC below 2^-52 in sum: w = 0.0, its records add nothing, and the other ECs' terms are untouched"""
    idx = testgfa_index
    n, lens, names = idx.view.n_paths, _lens(idx), _names(idx)
    ecs = sorted({(0,): 9, (1, 2): 4, (0, 1): 2}.items())
    e = {ids: i for i, (ids, _) in enumerate(ecs)}
    t = Table(ecs, sorted([(e[(0,)], 0, 0, 30), (e[(1, 2)], 1, 0, 30), (e[(1, 2)], 2, 4, 20), (e[(0, 1)], 1, 2, 9), (e[(0, 1)], 0, 2, 9)]), [9, 2, 2, 4, 4])
    alpha = [0.0] * n
    alpha[0], alpha[1], alpha[2] = 11.0, 2.0 ** -54, 2.0 ** -54
    assert weight_py(ecs, alpha, e[(1, 2)], 1) == 0.0 and 0.0 < weight_py(ecs, alpha, e[(0, 1)], 1) < 1e-15
    for p in (0, 1, 2):
        D = depth_py(t, alpha, p, int(lens[p]))
        assert _depth_lib(idx, t, alpha, p).tobytes() == np.array(D, dtype=np.float64).tobytes()
    assert max(depth_py(t, alpha, 2, int(lens[2]))) == 0.0
    want = calls_text(names, lens, t, alpha=alpha, min_reads=0.0)
    _write(idx, t, tmp_path / "c.tsv", alpha=np.array(alpha), min_reads=0.0)
    assert (tmp_path / "c.tsv").read_bytes() == want and want.count(b"\n") == n


def test_depth_exactly_at_and_one_ulp_below_call_depth(testgfa_index, tmp_path):
    """D_p[x] >= callDepth: equal counts, one ulp below does not"""
    idx = testgfa_index
    n, lens, names = idx.view.n_paths, _lens(idx), _names(idx)
    ecs = sorted({(0, 1): 6, (0,): 3}.items())
    e = {ids: i for i, (ids, _) in enumerate(ecs)}
    t = Table(ecs, sorted([(e[(0, 1)], 0, 0, 9), (e[(0, 1)], 1, 0, 9), (e[(0,)], 0, 5, 14)]), [1, 3, 3])
    alpha = [0.0] * n
    alpha[0], alpha[1] = 1.0, 2.0
    D = depth_py(t, alpha, 0, int(lens[0]))
    d_lo, d_hi = D[0], D[5]                      # 3 * (1/3) and that + 1.0
    assert d_lo == 3.0 * (1.0 / 3.0) and d_hi == d_lo + 1.0 and D[14] == 1.0 and D[15] == 0.0
    for depth, covered in ((d_hi, 5), (math.nextafter(d_hi, 3.0), 0), (math.nextafter(d_hi, 0.0), 5), (d_lo, 15), (math.nextafter(1.0, 2.0), 5)):
        want = calls_text(names, lens, t, alpha=alpha, call_depth=depth, min_reads=0.5)
        _write(idx, t, tmp_path / "c.tsv", alpha=np.array(alpha), call_depth=depth, min_reads=0.5)
        assert (tmp_path / "c.tsv").read_bytes() == want
        assert want.splitlines()[0].split(b"\t")[4] == b"%.4f" % (covered / int(lens[0])), (depth, want)


def test_merge_of_exports_that_differ_in_order_and_overlap(testgfa_index):
    idx = testgfa_index
    n = idx.view.n_paths
    a = Table([((0,), 4), ((0, 1), 2), ((2,), 1)], [(0, 0, 0, 9), (1, 0, 3, 12), (1, 1, 3, 12), (2, 2, 1, 5)], [4, 2, 2, 1])
    # the same classes listed in another order, IDs reversed, one class more, one tuple in common
    b_ecs = [((1, 0), 3), ((3,), 5), ((0,), 1)]
    b_rows, b_n = [(0, 1, 3, 12), (0, 0, 7, 20), (1, 3, 0, 4), (2, 0, 0, 9)], [3, 3, 5, 1]
    b_sorted = Table(sorted((tuple(sorted(i)), c) for i, c in b_ecs), [], [])
    remap = {0: 1, 1: 2, 2: 0}                       # position in b_ecs -> position in b_sorted.ecs
    b = Table(b_sorted.ecs, sorted((remap[r[0]],) + r[1:] for r in b_rows), [x for _, x in sorted(zip([(remap[r[0]],) + r[1:] for r in b_rows], b_n))])
    want = merge_tables([a, b])
    assert len(want.ecs) == 4 and dict(want.ecs)[(0, 1)] == 5 and int(want.n[(want.rows == (want.rows[0])).all(axis=1)][0]) == 5
    exp_b = csr(b_ecs) + (np.array(b_rows, dtype=np.uint32), np.array(b_n, dtype=np.uint64))
    off, ids, cnt, rows, tn = host.acov_merge(n, [a.arrays(), exp_b])
    w_off, w_ids, w_cnt, w_rows, w_n = want.arrays()
    assert np.array_equal(off, w_off) and np.array_equal(ids, w_ids) and np.array_equal(cnt, w_cnt)
    assert np.array_equal(rows, w_rows) and np.array_equal(tn, w_n)
    # one export merges to itself; none to nothing
    got = host.acov_merge(n, [a.arrays()])
    assert all(np.array_equal(x, y) for x, y in zip(got, a.arrays()))
    assert [len(x) for x in host.acov_merge(n, [])] == [1, 0, 0, 0, 0]


@pytest.mark.parametrize("interleave", [False, True])
def test_report_calls_on_a_bam(interleave, small_index, tmp_path):
    """groot_host_report_calls == the file computed here from the BAM's own records grouped by QNAME, and == calls_from_table on the
    table of the oracle's records"""
    index = small_index
    b, al = _oracle_alns(index, clipped_reads(index, 1500, 23))
    t = table_of_alns(index, al, b["seq_off"])
    if interleave:
        al = al[np.random.default_rng(5).permutation(len(al))]
    bam = str(tmp_path / "x.bam")
    w = host.BamWriter(bam, index, date="2020-01-01T00:00:00Z")
    w.write(al, b)
    w.close()
    _, _, recs = read_bam(bam)
    assert sum(r["flag"] != 4 for r in recs) == len(al) == int(t.n.sum())
    names, lens = _names(index), _lens(index)
    want = calls_text(names, lens, t)
    assert want.count(b"\n") > 3 and any(len(i) > 1 for i, _ in t.ecs)
    lines, called, tuples = host.report_calls(bam, str(tmp_path / "c.tsv"))
    assert (tmp_path / "c.tsv").read_bytes() == want and lines == want.count(b"\n") and tuples == len(t.n)
    _write(index, t, tmp_path / "d.tsv")
    assert (tmp_path / "d.tsv").read_bytes() == want
    want2 = calls_text(names, lens, t, call_depth=0.5, cov_cutoff=0.3, min_reads=0.5)
    _, called, _ = host.report_calls(bam, str(tmp_path / "e.tsv"), min_reads=0.5, call_depth=0.5, cov_cutoff=0.3)
    assert (tmp_path / "e.tsv").read_bytes() == want2 != want
    assert 0 < called == sum(ln.endswith(b"\t1") for ln in want2.splitlines()) < want2.count(b"\n")


# ---- the device side: the seven graphs of test_counter_edges.py -------------------------------------------------------------------

@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return _build_case(tmp_path_factory.mktemp("calls"))


def _want(index, b):
    """the batch's table, computed once"""
    if getattr(b, "_calls", None) is None:
        b._calls = table_of_alns(index, b.want(index).alns, b.off)
    return b._calls


# the smallest count of every class over the three batches of the case (asserted on the CPU below, and before every GPU run)
# both_strands_read: a read with records on both strands of one path.  The seven graphs are random text, no read of 28 bases lies on
# a path and on its reverse complement: the oracle reaches 0 in every batch, and 0 is asserted (the host test above covers the case by
# hand).  both_strands: paths that carry records of both strands (every second read is reverse-complemented).
FLOOR = {"fast": 1000, "slow": 100, "clipped": 20, "both_strands": 20, "both_strands_read": 0, "equal_tuples": 20, "one_set_many_intervals": 20}


def _classes(index, b):
    w = b.want(index)
    al, t = w.alns, _want(index, b)
    lens = _lens(index)
    off = np.asarray(b.off, dtype=np.int64)
    rid, ref, pos = al["read_id"].astype(np.int64), al["ref_id"].astype(np.int64), al["pos"].astype(np.int64)
    m = (off[rid + 1] - off[rid]) - al["start_clip"].astype(np.int64) - al["end_clip"].astype(np.int64)
    key = rid * 1024 + ref
    fwd, rev = set(key[al["rc"] == 0].tolist()), set(key[al["rc"] == 1].tolist())
    ep = t.rows[:, 0] * 1024 + t.rows[:, 1]
    return {"fast": int(((w.graphs > 0) & (w.graphs <= 4)).sum()), "slow": int((w.graphs > 4).sum()),
            "clipped": int((pos + m > lens[ref] - 1).sum()),                           # records cut at path_len - 1
            "both_strands_read": len(fwd & rev),                                       # (read, path) with a record on each strand
            "both_strands": len(set(ref[al["rc"] == 0].tolist()) & set(ref[al["rc"] == 1].tolist())),
            "equal_tuples": int((t.n >= 2).sum()),                                     # one tuple from several records
            "one_set_many_intervals": int((np.bincount(np.unique(ep, return_inverse=True)[1].reshape(-1)) >= 2).sum())}   # (EC, path) with several intervals


def _assert_classes(index, batches):
    for b in batches:
        c = _classes(index, b)
        assert all(c[k] >= FLOOR[k] for k in FLOOR) and c["both_strands_read"] == 0, (b.name, c)


def test_inputs_hold_every_class(case):
    index, batches = case
    for b in batches:
        print(b.name, _classes(index, b), "tuples", len(_want(index, b).n), "records", int(_want(index, b).n.sum()))
    _assert_classes(index, batches)
    t = merge_tables([_want(index, b) for b in batches])
    assert int(t.n.sum()) == sum(len(b.want(index).alns) for b in batches)
    # equal tuples from different reads
    assert sum(len(_want(index, b).n) for b in batches) > len(t.n)


def _open(index, batches, acov=True, ec_first=False, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    al = device.Aligner(index, threshold=0.9, max_batch_reads=max(1024, max(b.n for b in batches)), **kw)
    if ec_first:
        al.ec_enable()
    if acov:
        al.acov_enable()
    return al


def _dev_table(al):
    off, ids, cnt, rows, n = al.acov()
    ecs = [(tuple(ids[off[i]:off[i + 1]].tolist()), int(cnt[i])) for i in range(len(cnt))]
    assert ecs == sorted(ecs)
    return Table(ecs, rows, n)


def _check(al, index, batches):
    want = merge_tables([_want(index, b) for b in batches])
    got = _dev_table(al)
    assert got.ecs == want.ecs
    assert got.rows.shape == want.rows.shape and np.array_equal(got.rows, want.rows), (got.rows.shape, want.rows.shape)
    assert np.array_equal(got.n, want.n), np.flatnonzero(got.n != want.n)[:10]
    st = al.acov_stats()
    print("acov", st)
    assert st["records"] == int(want.n.sum()) and st["tuples"] == len(want.n), st
    return got, st


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_device_table_equals_the_records(case, hip_lib, monkeypatch, stage, rod):
    """three batches (unclipped, clipped, unclipped) through one ctx under each align stage, results in HBM or copied out; the file
    written from the device table is the file of the records"""
    index, batches = case
    _assert_classes(index, batches)
    _stage(monkeypatch, stage)
    al = _open(index, batches, results_on_device=rod)
    try:
        _feed(al, batches)
        got, st = _check(al, index, batches)
        assert st["slow_records"] > 0
    finally:
        al.close()


@pytest.mark.gpu
def test_depth_and_file_from_the_device_table(case, hip_lib, monkeypatch, tmp_path):
    index, batches = case
    b = batches[1]
    _stage(monkeypatch, "path_first")
    al = _open(index, [b])
    try:
        _feed(al, [b])
        got, _ = _check(al, index, [b])
    finally:
        al.close()
    want = _want(index, b)
    names, lens, n = _names(index), _lens(index), index.view.n_paths
    alpha, _, _ = em_py(n, want.ecs)
    # the paths with the most ECs on them, and a one-path graph
    per_path = np.bincount(np.unique(want.rows[:, :2], axis=0)[:, 1], minlength=n)
    for p in list(np.argsort(per_path)[-2:]) + [int(np.flatnonzero(per_path > 0)[0])]:
        D = depth_py(want, alpha, int(p), int(lens[p]))
        assert _depth_lib(index, got, alpha, int(p)).tobytes() == np.array(D, dtype=np.float64).tobytes()
    few = np.flatnonzero(np.array(alpha) >= 1.0)
    assert len(few) > 3
    cut = sorted(np.array(alpha)[few])[-6] if len(few) > 6 else 1.0       # (the plain-Python pileup of every path would take minutes)
    text = calls_text(names, lens, want, alpha=alpha, min_reads=float(cut))
    _write(index, got, tmp_path / "c.tsv", min_reads=float(cut))
    assert (tmp_path / "c.tsv").read_bytes() == text and text.count(b"\n") >= 4


@pytest.mark.gpu
def test_forced_slow_mode(case, hip_lib, monkeypatch):
    """GROOT_TEST_SHARED_SLOW: every multi-graph read is grouped on the host at collect"""
    index, batches = case
    _assert_classes(index, batches[:2])
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    al = _open(index, batches[:2])
    try:
        _feed(al, batches[:2])
        _, st = _check(al, index, batches[:2])
        multi = sum(int((b.want(index).graphs > 1).sum()) for b in batches[:2])
        assert al.ec_stats()["slow_reads"] == multi and st["slow_records"] > 0
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ec_slots", [None, "8"])
@pytest.mark.parametrize("depth", [0, 3])
def test_table_grows_from_eight_slots(case, hip_lib, monkeypatch, ec_slots, depth):
    """GROOT_TEST_ACOV_SLOTS=8: the claim phase of the first batches runs out of room, the table grows at collect many times and the batch is
    counted again -- once; with GROOT_TEST_EC_SLOTS=8 too the EC table is rehashed under it and the serials must survive"""
    index, batches = case
    _assert_classes(index, batches)
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_ACOV_SLOTS", "8")
    if ec_slots:
        monkeypatch.setenv("GROOT_TEST_EC_SLOTS", ec_slots)
    seq = [batches[0].take(np.arange(300), "300"), batches[0], batches[1], batches[2].take(np.arange(2000), "2000"), batches[2]]
    al = _open(index, seq, pipeline_depth=depth)
    try:
        if depth:
            assert _feed_pipelined(al, seq, depth=depth) == [0] * len(seq)
        else:
            _feed(al, seq)
        _, st = _check(al, index, seq)
        assert st["grows"] >= 5 and st["slots"] >= 2 * st["tuples"], st      # (8 slots to > 2^19 by factors of at most four: at least six steps)
        if ec_slots:
            assert al.ec_stats()["grows"] >= 2
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
def test_redone_batches_count_once(case, hip_lib, monkeypatch, rod):
    """GROOT_TEST_SMALL_BUFFERS: every buffer starts too small, collect redoes the batch; the pass that is redone adds nothing"""
    index, batches = case
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    al = _open(index, batches[:2], results_on_device=rod)
    try:
        _feed(al, batches[:2])
        _check(al, index, batches[:2])
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("kind", sorted(_CODE))
def test_failing_batch(case, hip_lib, monkeypatch, kind, pipelined):
    """a batch that fails with GROOT_E_NOSPACE is not counted; one that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP counts its
    other reads.  Collected alone, and with three batches in flight and good batches on both sides of it."""
    index, (b0, b1, b2) = case
    good = [b0.take(np.arange(3000), "good 0"), b2.take(np.arange(3000), "good 1"), b0.take(np.arange(3000, 6000), "good 2")]
    bad, bad_wants = _bad_batch(index, b1.take(np.arange(2000), "bad"), kind)
    # what the bad batch adds: the table of the batch _bad_batch names as its expectation (its own reads, or the rest without the bad one)
    if kind == "short":
        reads = [bytes(bad.seq[int(bad.off[i]):int(bad.off[i + 1])]) for i in range(bad.n)]
        extra = [_of_reads("short, rest", [r for r in reads if len(r) == L])]
    else:
        extra = [bad] if bad_wants else []
    _stage(monkeypatch, "path_first")
    seq = good[:2] + [bad] + good[2:]
    al = _open(index, seq, max_read_len=64, pipeline_depth=3 if pipelined else 0)
    try:
        if pipelined:
            assert _feed_pipelined(al, seq) == [0, 0, _CODE[kind], 0]
            _check(al, index, good[:2] + extra + good[2:])
        else:
            first = _feed(al, good[:1])
            al.submit(bad.seq, bad.off, first_read_id=first)
            with pytest.raises(host.GrootError) as e:
                al.wait()
            assert e.value.code == _CODE[kind]
            _check(al, index, good[:1] + extra)
            _feed(al, good[1:2], first + bad.n)
            _check(al, index, good[:2] + extra)
    finally:
        al.close()


@pytest.mark.gpu
def test_depth_three_with_empty_and_one_read_batches(case, hip_lib, monkeypatch):
    index, (b0, b1, b2) = case
    w0 = b0.want(index)
    rng = np.random.default_rng(5)
    noise = _of_reads("noise", ["".join(rng.choice(list("ACGT"), L)).encode() for _ in range(500)])
    empty = _of_reads("no reads", [])
    one_slow = b0.take([int(np.flatnonzero(w0.graphs > 4)[0])], "one slow read")
    one_fast = b0.take([int(np.flatnonzero(w0.graphs == 1)[0])], "one fast read")
    seq = [b0, empty, one_slow, noise, one_fast, empty, b1, one_fast]
    assert len(noise.want(index).alns) == 0 and empty.n == 0
    _stage(monkeypatch, "path_first")
    al = _open(index, seq, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, seq, depth=3) == [0] * len(seq)
        _check(al, index, seq)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ec_first", [False, True])
def test_reset_enable_order_and_off(case, hip_lib, monkeypatch, ec_first):
    """reset between runs; enabled after ec_enable and before it; switched off again: nothing is launched and the stats stay zero"""
    index, batches = case
    b0, b2 = batches[0].take(np.arange(2500), "2500"), batches[2].take(np.arange(2500), "2500'")
    _stage(monkeypatch, "path_first")
    al = _open(index, [b0, b2], ec_first=ec_first)
    try:
        assert al.ec_stats()["reads"] == 0                  # assigned coverage switched equivalence classes on
        _feed(al, [b0])
        _check(al, index, [b0])
        al.acov_reset()                                     # the tuples go, the ECs stay
        st = al.acov_stats()
        assert st["records"] == st["tuples"] == 0 and al.ec_stats()["reads"] > 0
        al.ec_reset()                                       # both empty: the serials start again
        _feed(al, [b2, b0])
        _check(al, index, [b2, b0])
        al.acov_enable(False)
        before = al.acov_stats()
        assert before["records"] == before["tuples"] == before["slots"] == 0 and before["launches"] > 0
        _feed(al, [b0])
        assert al.acov_stats() == before                    # no launch while off
        with pytest.raises(host.GrootError):
            al.acov()
        assert al.ec_stats()["reads"] > 0                   # equivalence classes stayed on
        al.ec_reset()
        al.acov_enable()
        _feed(al, [b2])
        _check(al, index, [b2])
        al.pairs_enable(False)
        with pytest.raises(host.GrootError):
            al.pairs_enable(True)                           # units of two mates have no weight rule yet
    finally:
        al.close()


@pytest.mark.gpu
def test_two_contexts_merge_to_the_table_of_one(case, hip_lib, monkeypatch):
    index, batches = case
    parts = [batches[0].take(np.arange(0, 3000), "a"), batches[1].take(np.arange(0, 4000), "b"), batches[0].take(np.arange(3000, 6000), "c"),
             batches[2].take(np.arange(0, 3000), "d")]
    _stage(monkeypatch, "path_first")
    exports = []
    for mine in (parts[0::2], parts[1::2]):
        al = _open(index, parts)
        try:
            _feed(al, mine)
            exports.append(al.acov())
        finally:
            al.close()
    al = _open(index, parts)
    try:
        _feed(al, parts)
        one, _ = _check(al, index, parts)
    finally:
        al.close()
    off, ids, cnt, rows, n = host.acov_merge(index.view.n_paths, exports)
    w_off, w_ids, w_cnt, w_rows, w_n = one.arrays()
    assert np.array_equal(off, w_off) and np.array_equal(ids, w_ids) and np.array_equal(cnt, w_cnt)
    assert np.array_equal(rows, w_rows) and np.array_equal(n, w_n)
    assert len(exports[0][4]) + len(exports[1][4]) > len(w_n)          # tuples both contexts hold
