"""Assignment (`align --assignFrom`): each read to its best allele by EM posterior.  The definition, quoted from include/groot_hip.h:

  Input: alpha[n_paths] (global path = BAM reference order), every value finite and 0 <= alpha[p] <= 1e300; min_post in [0, 1].
  S(r) exactly as for --sharedReads: the global paths carrying at least one record of read r.
  For a read r with records, double precision, no FMA contraction, p running over S(r) in ASCENDING global ID:
      denom = 0.0;  denom = denom + alpha[p]
      best  = the p of S(r) with the largest alpha[p]; among equal values the lowest ID
    unassigned:  denom == 0.0.                                   No record of r is kept.
    below:       not (alpha[best] >= min_post * denom)           (one product, one comparison, no division).  No record of r is kept.
    assigned:    otherwise.  Every record of r on `best` is kept (every traversal whose path set holds best; both strands), nothing else.
      rest = denom - alpha[best]                                 (>= 0: a sum of non-negative terms is never below one of them)
      j    = the number of k in 1..20 with ldexp(rest, k) <= denom   (a product by 2^k is exact; rest == 0 gives 20)
      mapq = 3 * j                                               (0, 3, .., 60: one step per halving of the posterior mass elsewhere)
  What happens to the batch's traversal records, in place, BEFORE anything else reads them:
    the number of traversals, their order, read_id, graph_id, node, offset, ord and the RC / clip flags do not change;
    a kept traversal's path set becomes {best} (every other bit of all its words cleared); a traversal that is not kept gets the EMPTY
    path set (it expands to no record), loses GROOT_TRAV_FIRST and has reserved = 0;
    GROOT_TRAV_FIRST is cleared on all of r's traversals and set on the first kept one in (read, ord) order: an assigned read has exactly
    one primary record, its further records on `best` are secondary;
    kept traversals get GROOT_TRAV_MAPQ (16u, new) and reserved = mapq.
  Per read (batch position): best[r] = the global path, 0xFFFFFFFF when r keeps no record; mapq[r], 0 then.
  groot_counts (mapped, multimapped, alignments, travs, ...), call counts, weights and the GFA are those of the unfiltered run.

Everything below restates that in plain Python (assign_py, filter_py) on expanded records -- the CPU oracle's for the device tests -- and
compares exactly: the filtered traversals and masks as bytes, host.expand_alns of them as arrays, best, mapq and the eight stats.  No
tolerance anywhere.  The oracle yields records, not traversals, so a batch's unfiltered traversal list comes from a run with assignment
off whose expansion is first asserted equal to the oracle's records; which record belongs to which traversal follows from the path sets'
popcounts."""
import math
import os

import numpy as np
import pytest

from bamread import read_bam
from conftest import DATA
from groot_amd import device, host
from test_counter_edges import L, NP, THR, _bad_batch, _Batch, _build_case, _of_reads, _CODE
from test_coverage import STAGES, _stage, expand_coverage
from test_path_pass import _gfa, _reads_from, _seq

NONE = 0xFFFFFFFF
STAT_KEYS = ("reads", "assigned", "unassigned", "below", "ties", "records_in", "records_kept", "travs_emptied")


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def assign_py(alns, alpha, min_post, n_reads, first=0):
    """per read, in record order -> (best[n_reads], mapq[n_reads], per-record `kept`, the stats the records alone determine)"""
    alpha = [float(x) for x in alpha]
    best, mapq = [NONE] * n_reads, [0] * n_reads
    kept = np.zeros(len(alns), dtype=bool)
    st = dict.fromkeys(STAT_KEYS[:6], 0)
    rid, ref = alns["read_id"].tolist(), alns["ref_id"].tolist()
    i = 0
    while i < len(rid):
        j = i
        while j < len(rid) and rid[j] == rid[i]:
            j += 1
        refs = sorted(set(ref[i:j]))                       # ascending unique ref_id
        denom = 0.0
        for p in refs:
            denom = denom + alpha[p]
        b = refs[0]
        for p in refs:
            if alpha[p] > alpha[b]:
                b = p
        st["reads"] += 1
        st["records_in"] += j - i
        if denom == 0.0:
            st["unassigned"] += 1
        elif not (alpha[b] >= min_post * denom):
            st["below"] += 1
        else:
            st["assigned"] += 1
            st["ties"] += sum(1 for p in refs if alpha[p] == alpha[b]) >= 2
            rest = denom - alpha[b]
            jj = sum(1 for k in range(1, 21) if math.ldexp(rest, k) <= denom)
            r = (rid[i] - first) & 0xFFFFFFFF
            best[r], mapq[r] = b, 3 * jj
            for x in range(i, j):
                kept[x] = ref[x] == b
        i = j
    return np.array(best, dtype=np.uint32), np.array(mapq, dtype=np.uint8), kept, st


def _rec_trav(masks):
    """the traversal of every expanded record: one record per set bit, traversal after traversal"""
    pop = np.array([sum(bin(int(w)).count("1") for w in row) for row in masks], dtype=np.int64) if len(masks) else np.zeros(0, dtype=np.int64)
    return np.repeat(np.arange(len(masks)), pop)


def filter_py(index, travs, masks, alns, alpha, min_post, n_reads, first=0):
    """the definition applied to a traversal list whose expansion is `alns` -> (travs, masks, alns, best, mapq, stats)"""
    gpo = index.arrays["graph_path_off"].astype(np.int64)
    best, mapq, kept, st = assign_py(alns, alpha, min_post, n_reads, first)
    rt = _rec_trav(masks)
    assert len(rt) == len(alns)
    t, m = travs.copy(), np.zeros_like(masks)
    trav_kept = np.zeros(len(t), dtype=bool)
    trav_kept[rt[kept]] = True
    seen = set()
    for i in range(len(t)):
        fl = int(t["flags"][i]) & ~(device.TRAV_FIRST | device.TRAV_MAPQ)
        res = 0
        if trav_kept[i]:
            r = (int(t["read_id"][i]) - first) & 0xFFFFFFFF
            l = int(best[r]) - int(gpo[int(t["graph_id"][i])])
            m[i, l >> 6] = np.uint64(1) << np.uint64(l & 63)
            fl |= device.TRAV_MAPQ
            if r not in seen:
                fl |= device.TRAV_FIRST
                seen.add(r)
            res = int(mapq[r])
        t["flags"][i], t["reserved"][i] = fl, res
    out = alns[kept].copy()
    if len(out):
        out["secondary"] = np.r_[False, out["read_id"][1:] == out["read_id"][:-1]].astype(np.uint8)
    st["records_kept"] = int(trav_kept.sum())
    st["travs_emptied"] = int(len(t) - trav_kept.sum())
    assert st["records_kept"] == int(kept.sum())           # a kept traversal holds exactly one record on best
    return t, m, out, best, mapq, st


def _same_alns(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in device.ALN_DTYPE.names)


def _check_host(index, travs, masks, alpha, min_post, n_reads, first=0):
    """host.assign_travs == filter_py on the host library's own expansion of the list; returns what filter_py gives"""
    alns = device.expand_alns(index, travs, masks)
    want = filter_py(index, travs, masks, alns, alpha, min_post, n_reads, first)
    t, m, best, mapq, st = host.assign_travs(index, alpha, min_post, travs, masks, first, n_reads)
    assert t.tobytes() == want[0].tobytes() and m.tobytes() == want[1].tobytes()
    assert _same_alns(device.expand_alns(index, t, m), want[2])
    assert np.array_equal(best, want[3]) and np.array_equal(mapq, want[4]) and st == want[5], (st, want[5])
    return want


# ---- host: hand-made traversal lists ----------------------------------------------------------------------------------------------

def _node_on(index, g, paths):
    """a node of graph g that every path of `paths` (local ids) passes"""
    a = index.arrays
    for n in range(int(a["graph_node_off"][g]), int(a["graph_node_off"][g + 1])):
        here = set(a["np_path"][int(a["node_np_off"][n]):int(a["node_np_off"][n + 1])].tolist())
        if set(paths) <= here:
            return n
    raise AssertionError("no such node")


def _list(index, rows, first=0):
    """rows: (read, graph, [local paths], flags) in (read, ord) order -> (travs, masks)"""
    pw = index.view.path_words
    t = np.zeros(len(rows), dtype=device.TRAV_DTYPE)
    m = np.zeros((len(rows), pw), dtype=np.uint64)
    ords = {}
    for i, (r, g, paths, fl) in enumerate(rows):
        t[i] = ((first + r) & 0xFFFFFFFF, g, _node_on(index, g, paths), 0, ords.get(r, 0), fl, 0)
        ords[r] = ords.get(r, 0) + 1
        for p in paths:
            m[i, p >> 6] |= np.uint64(1) << np.uint64(p & 63)
    return t, m


@pytest.fixture(scope="module")
def two_graphs():
    """test.gfa twice: two graphs of 6 paths (the hand-made lists that need a second graph)"""
    f = os.path.join(DATA, "test.gfa")
    return host.Index.from_gfa_files([f, f], host.index_params(k=7, s=10, w=30))


F, RC = device.TRAV_FIRST, device.TRAV_RC


def test_host_two_kept_traversals_on_one_path(testgfa_index):
    """both strands of a read on `best`: the second is secondary, both carry the MAPQ (cannot occur on the device: the RC strand is tried
    only when the forward one fails)"""
    idx = testgfa_index
    assert idx.view.n_paths == 6
    t, m = _list(idx, [(0, 0, [0, 1, 2], F), (0, 0, [1, 3], RC)])
    alpha = [0.25, 1.0, 0.25, 0.5, 0, 0]
    ft, fm, al, best, mapq, st = _check_host(idx, t, m, alpha, 0.0, 1)
    assert best.tolist() == [1] and mapq.tolist() == [3]                    # denom = 2.0, rest = 1.0: 2 * rest <= denom < 4 * rest
    assert ft["flags"].tolist() == [F | device.TRAV_MAPQ, RC | device.TRAV_MAPQ] and al["secondary"].tolist() == [0, 1] and al["rc"].tolist() == [0, 1]
    assert fm[:, 0].tolist() == [2, 2] and st["records_in"] == 5 and st["records_kept"] == 2 and st["travs_emptied"] == 0


def test_host_first_traversal_dies(two_graphs):
    """the read's first traversal dies; a later one of the same graph and one of another graph live (reads 0 and 1)"""
    idx = two_graphs
    assert idx.view.n_graphs == 2 and idx.view.n_paths == 12
    rows = [(0, 0, [0, 1], F), (0, 0, [2], 0), (0, 1, [0], F),               # best = path 2: second traversal of graph 0
            (1, 0, [0, 1], F), (1, 0, [2], 0), (1, 1, [3], F | RC),            # best = path 9: graph 1
            (3, 1, [5], F)]
    t, m = _list(idx, rows, first=7)
    alpha = [0.5, 0.5, 4.0, 0, 0, 0, 1.0, 0, 0, 0, 0, 0.125]
    alpha2 = list(alpha)
    alpha2[9] = 64.0
    ft, fm, al, best, mapq, st = _check_host(idx, t, m, alpha, 0.0, 4, first=7)
    assert best.tolist() == [2, 2, NONE, 11] and ft["flags"].tolist() == [0, F | 16, 0, 0, F | 16, RC, F | 16]
    assert mapq.tolist() == [3, 6, 0, 60] and st["travs_emptied"] == 4       # read 0: rest 2 of 6; read 1: rest 1 of 5
    ft, fm, al, best, mapq, st = _check_host(idx, t, m, alpha2, 0.0, 4, first=7)
    assert best.tolist() == [2, 9, NONE, 11] and ft["flags"].tolist() == [0, F | 16, 0, 0, 0, F | RC | 16, F | 16]
    assert fm[5].tolist()[0] == 8 and al["graph_id"].tolist() == [0, 1, 1]


def test_host_threshold_exact_and_one_ulp_below(testgfa_index):
    """alpha[best] == min_post * denom exactly is kept; the next double above that min_post drops the read"""
    idx = testgfa_index
    t, m = _list(idx, [(0, 0, [0, 1], F)])
    alpha = [3.0, 1.0, 0, 0, 0, 0]
    assert 0.75 * 4.0 == 3.0
    _, _, _, best, _, st = _check_host(idx, t, m, alpha, 0.75, 1)
    assert best.tolist() == [0] and st["assigned"] == 1
    _, _, al, best, mapq, st = _check_host(idx, t, m, alpha, math.nextafter(0.75, 1.0), 1)
    assert best.tolist() == [NONE] and mapq.tolist() == [0] and st["below"] == 1 and len(al) == 0
    # ... and alpha[best] one ulp below the product
    alpha[0] = math.nextafter(3.0, 0.0)
    _check_host(idx, t, m, alpha, 0.75, 1)


def test_host_ties_rest_zero_tiny_and_denormal(testgfa_index):
    idx = testgfa_index
    rows = [(0, 0, [1, 4], F),            # a tie at the top: the lowest ID, MAPQ 3 for two equal paths
            (1, 0, [2], F),               # rest == 0: 60
            (2, 0, [2, 3], F),            # 2^-60 beside 1.0: 1 + 2^-60 rounds to 1, rest = 0
            (3, 0, [5], F),               # a denormal alone
            (4, 0, [3, 5], F),            # a denormal beside 2^-60
            (6, 0, [0], F)]               # all-zero S(r); reads 5 and 7 have no records
    t, m = _list(idx, rows)
    den = 5e-324
    alpha = [0.0, 0.5, 1.0, 2.0 ** -60, 0.5, den]
    ft, fm, al, best, mapq, st = _check_host(idx, t, m, alpha, 0.0, 8)
    assert best.tolist() == [1, 2, 2, 5, 3, NONE, NONE, NONE] and mapq.tolist() == [3, 60, 60, 60, 60, 0, 0, 0]
    assert st == {"reads": 6, "assigned": 5, "unassigned": 1, "below": 0, "ties": 1, "records_in": 9, "records_kept": 5, "travs_emptied": 1}
    _check_host(idx, t, m, alpha, 1.0, 8)
    # a denormal rest: products by 2^k of a denormal are exact
    alpha = [0.0, 0.0, 0.0, den * 3, 0.0, den * 5]
    _, _, _, best, mapq, _ = _check_host(idx, t[4:5], m[4:5], alpha, 0.0, 8)
    assert best[4] == 5 and mapq[4] == 3 * sum(1 for k in range(1, 21) if math.ldexp(den * 3, k) <= den * 8) == 3


def test_host_empty_list_and_bad_arguments(testgfa_index):
    idx = testgfa_index
    t, m = _list(idx, [])
    ft, fm, best, mapq, st = host.assign_travs(idx, [1.0] * 6, 0.0, t, m, 0, 3)
    assert len(ft) == 0 and best.tolist() == [NONE] * 3 and mapq.tolist() == [0] * 3 and not any(st.values())
    t, m = _list(idx, [(0, 0, [0], F)])
    for bad in (float("nan"), -1e-300, 2e300, float("inf")):
        with pytest.raises(host.GrootError) as e:
            host.assign_travs(idx, [1.0, bad, 0, 0, 0, 0], 0.0, t, m, 0, 1)
        assert e.value.code == -1
    for mp in (-0.1, 1.5, float("nan")):
        with pytest.raises(host.GrootError):
            host.assign_travs(idx, [1.0] * 6, mp, t, m, 0, 1)
    with pytest.raises(host.GrootError):
        host.assign_travs(idx, [1.0] * 6, 0.0, t, m, 1, 1)                  # a read outside the batch
    assert host.assign_travs(idx, [1e300] * 6, 1.0, t, m, 0, 1)[2].tolist() == [0]
    # not in (read, ord) order: a read in two runs, reads in falling batch position (also across the wrap of the read id) -- refused, not
    # taken for two reads
    for rows, first in (([(0, 0, [0], F), (1, 0, [1], F), (0, 0, [2], 0)], 0), ([(1, 0, [0], F), (0, 0, [1], F)], 0), ([(1, 0, [0], F), (0, 0, [1], F)], 2 ** 32 - 1)):
        t, m = _list(idx, rows, first=first)
        with pytest.raises(host.GrootError) as e:
            host.assign_travs(idx, [1.0] * 6, 0.0, t, m, first, 2)
        assert e.value.code == -1
    t, m = _list(idx, [(0, 0, [0], F), (1, 0, [1], F)], first=2 ** 32 - 1)      # in order across the wrap: read ids 2^32 - 1, 0
    assert host.assign_travs(idx, [1.0] * 6, 0.0, t, m, 2 ** 32 - 1, 2)[2].tolist() == [0, 1]


# ---- host: the abundance file read back ----------------------------------------------------------------------------------------------

def test_abundance_read(testgfa_index, tmp_path):
    idx = testgfa_index
    names = [idx.path_name(p).lstrip("*") for p in range(6)]
    off, ids, cnt = np.array([0, 2, 3, 6], dtype=np.uint64), np.array([0, 1, 2, 3, 4, 5], dtype=np.uint32), np.array([700, 40, 9], dtype=np.uint64)
    f4, f8 = str(tmp_path / "a4.tsv"), str(tmp_path / "a8.tsv")
    rows = host.abundance_from_ecs(idx, off, ids, cnt, min_reads=2.0, out_path=f4)
    rows8 = host.abundance_boot_from_ecs(idx, off, ids, cnt, 5, min_reads=2.0, out_path=f8)
    assert 0 < len(rows) < 7 and [r[:4] for r in rows8] == rows
    for f in (f4, f8):
        alpha, n = host.abundance_read(idx, f)
        want = [0.0] * 6
        for ln in open(f):
            c = ln.rstrip("\n").split("\t")
            want[names.index(c[0])] = float(c[2])
        assert n == len(rows) and alpha.tolist() == want and sum(1 for x in want if x) == len(rows)
    good = open(f4).read().splitlines()
    bad = {"unknown": ["nobody\t1\t1.00\t0.1"], "twice": good[:1] + good[:1], "short": [good[0].split("\t")[0] + "\t5"],
           "negative": [names[0] + "\t1\t-1.00\t0.1"], "nan": [names[0] + "\t1\tnan\t0.1"], "huge": [names[0] + "\t1\t2e300\t0.1"],
           "text": [names[0] + "\t1\t1.0x\t0.1"], "empty value": [names[0] + "\t1\t\t0.1"]}
    for kind, lines in bad.items():
        p = str(tmp_path / "bad.tsv")
        open(p, "w").write("\n".join(lines) + "\n")
        with pytest.raises(host.GrootError) as e:
            host.abundance_read(idx, p)
        assert e.value.code == -3, kind
    with pytest.raises(host.GrootError) as e:
        host.abundance_read(idx, str(tmp_path / "missing.tsv"))
    assert e.value.code == -2


def test_abundance_read_shared_name(tmp_path):
    """two paths with one name after the '*' is stripped: naming it is an error, leaving it out is not"""
    rng = np.random.default_rng(3)
    nodes = {1: _seq(rng, 40), 2: _seq(rng, 40), 3: _seq(rng, 40), 4: _seq(rng, 40)}
    f = _gfa(tmp_path / "g.gfa", nodes, [(1, 2), (1, 3), (1, 4)], [("*x", [1, 2]), ("x", [1, 3]), ("y", [1, 4])])
    idx = host.Index.from_gfa_files([f], host.index_params(k=7, s=10, w=30))
    open(tmp_path / "ok.tsv", "w").write("y\t3\t2.50\t1.0\n")
    assert host.abundance_read(idx, str(tmp_path / "ok.tsv"))[0].tolist() == [0.0, 0.0, 2.5]
    open(tmp_path / "amb.tsv", "w").write("x\t3\t2.50\t1.0\n")
    with pytest.raises(host.GrootError) as e:
        host.abundance_read(idx, str(tmp_path / "amb.tsv"))
    assert e.value.code == -3


# ---- host: a BAM written from filtered traversals ----------------------------------------------------------------------------------

def _read_batch(n, length=40):
    rng = np.random.default_rng(9)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n * length)].copy()
    names = [b"read%d" % i for i in range(n)]
    noff = np.zeros(n + 1, dtype=np.uint64)
    noff[1:] = np.cumsum([len(x) for x in names])
    return {"seq": seq, "qual": np.full(n * length, 50, dtype=np.uint8), "seq_off": np.arange(n + 1, dtype=np.uint64) * length,
            "names": np.frombuffer(b"".join(names), dtype=np.uint8).copy(), "name_off": noff}


@pytest.mark.parametrize("level", [-1, -2])
def test_bam_from_filtered_traversals(two_graphs, tmp_path, level):
    idx = two_graphs
    rows = [(0, 0, [0, 1], F), (0, 0, [2], 0), (0, 1, [0], F), (1, 0, [0, 1, 3, 4, 5], F), (1, 0, [1, 3], RC), (2, 1, [4, 5], F | RC), (3, 0, [5], F)]
    t, m = _list(idx, rows, first=11)
    alpha = [0.5, 1.0, 4.0, 0, 0, 0, 1.0, 0, 0, 0, 0, 0]
    batch = _read_batch(4)
    names = [idx.path_name(p) for p in range(12)]

    def write(tt, mm, name):
        w = host.BamWriter(str(tmp_path / name), idx, date="2020-01-01T00:00:00Z")
        w.set_level(level)
        n = w.write_travs(tt, mm, batch, first_read_id=11)
        w.close()
        return n, read_bam(str(tmp_path / name))[2]

    # unflagged traversals: MAPQ 30 everywhere, as before
    n, recs = write(t, m, "plain.bam")
    assert n == len(recs) == 14 and {r["mapq"] for r in recs} == {30}
    ft, fm, al, best, mapq, st = _check_host(idx, t, m, alpha, 0.0, 4, first=11)
    n, recs = write(ft, fm, "assigned.bam")
    # read 0 -> path 2 (second traversal), read 1 -> path 1 on both strands, reads 2 and 3 -> nothing
    assert best.tolist() == [2, 1, NONE, NONE] and n == len(recs) == len(al) == 3
    assert [(r["name"], r["ref"], r["flag"], r["mapq"]) for r in recs] == [("read0", names[2], 0, int(mapq[0])), ("read1", names[1], 0, int(mapq[1])),
                                                                          ("read1", names[1], 0x110, int(mapq[1]))]
    assert [r["pos"] for r in recs] == al["pos"].tolist() and [r["ref_id"] for r in recs] == [2, 1, 1] and mapq.tolist() == [3, 3, 0, 0]
    # every traversal emptied: a BAM without records
    ft, fm, al, *_ = _check_host(idx, t, m, [0.0] * 12, 0.0, 4, first=11)
    assert write(ft, fm, "none.bam") == (0, [])


# ---- the seven-graph case (tests/test_counter_edges.py) -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    return _build_case(tmp_path_factory.mktemp("assign"))


def _alpha7(index):
    """the issue's alpha: (0, 2^-12, 2^-6, 0, 2^-9)[p % 5], then per graph local paths 0, 1, 2 -> 1, 0, 1 and the values below"""
    gpo = index.arrays["graph_path_off"].astype(np.int64)
    a = np.array([(0.0, 2.0 ** -12, 2.0 ** -6, 0.0, 2.0 ** -9)[p % 5] for p in range(index.view.n_paths)])
    for g in range(7):
        k = min(3, NP[g])
        a[gpo[g]:gpo[g] + k] = (1.0, 0.0, 1.0)[:k]
    for g, l, v in ((0, 69, 8.0), (1, 10, 8.0), (1, 63, 8.0), (2, 64, 64.0), (3, 128, 2.0), (4, 0, 0.0), (5, 127, 512.0), (6, 5, 1.0)):
        a[gpo[g] + l] = v
    return a


FLOOR = {"assigned": 2500, "unassigned": 150, "ties": 500, "word1": 1000, "word2": 250, "first_graph_dies": 400, "wide": 200, "mapq_values": 8, "below": 800}


def _classes(index, b):
    """the classes of the issue's table from the oracle's records of batch b (cached on the batch)"""
    if getattr(b, "_assign_classes", None) is None:
        w = b.want(index)
        gpo = index.arrays["graph_path_off"].astype(np.int64)
        alpha = _alpha7(index)
        best, mapq, _, st = assign_py(w.alns, alpha, 0.0, b.n)
        ok = best != NONE
        g_best = np.searchsorted(gpo, best[ok].astype(np.int64), side="right") - 1
        local = best[ok].astype(np.int64) - gpo[g_best]
        first_graph = np.full(b.n, -1, dtype=np.int64)
        rid = w.alns["read_id"].astype(np.int64)
        firsts = np.flatnonzero(np.r_[True, rid[1:] != rid[:-1]])
        first_graph[rid[firsts]] = w.alns["graph_id"][firsts]
        c = {"assigned": st["assigned"], "unassigned": st["unassigned"], "ties": st["ties"], "word1": int(((local >= 64) & (local < 128)).sum()),
             "word2": int((local >= 128).sum()), "first_graph_dies": int((g_best != first_graph[ok]).sum()), "wide": int((w.graphs[ok] > 4).sum()),
             "mapq_values": len(set(mapq[ok].tolist())), "below": assign_py(w.alns, alpha, 0.5, b.n)[3]["below"]}
        b._assign_classes = (c, set(mapq[ok].tolist()))
    return b._assign_classes


def _assert_classes(index, batches):
    for b in batches:
        c, mq = _classes(index, b)
        assert all(c[k] >= FLOOR[k] for k in FLOOR) and {0, 3, 60} <= mq, (b.name, c, sorted(mq))


def test_inputs_hold_every_class(case):
    index, batches = case
    for b in batches:
        print(b.name, _classes(index, b))
    _assert_classes(index, batches)
    # (every (read, graph) pair yields at least one traversal: with more than 256 such pairs in every batch and thousands of multi-graph
    # reads some read is bound to straddle a multiple of 256 in the list.  The oracle yields no traversals, so the straddle itself is asserted
    # on the list, at the top of every GPU test of this case: _assert_inputs)
    assert all(len(b.want(index).read_graph) > 2048 for b in batches)


# ---- the device ----------------------------------------------------------------------------------------------------------------------

def _open(index, batches, alpha=None, min_post=0.0, thr=THR, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    al = device.Aligner(index, threshold=thr, max_batch_reads=max(1024, max(b.n for b in batches)), **kw)
    if alpha is not None:
        al.assign_enable(alpha, min_post)
    return al


_UNF = {}


def _unfiltered(index, b, thr=THR):
    """the batch's traversal list with assignment off (cached; read ids from 0), its expansion asserted equal to the oracle's records"""
    key = (id(index), b.name, b.n, hash(b.seq.tobytes()))
    if key not in _UNF:
        with pytest.MonkeyPatch.context() as mp:            # (the shipped stage, full-size buffers, whatever the calling test has set)
            for k in [k for k in os.environ if k.startswith("GROOT_TEST_") or k in ("GROOT_LEAN", "GROOT_NO_PATH_PASS")]:
                mp.delenv(k)
            al = _open(index, [b], thr=thr)
            try:
                al.submit(b.seq, b.off)
                c = al.wait()
                t, m = al.travs()
                assert al.assign_stats() == dict.fromkeys(STAT_KEYS + ("launches",), 0)
            finally:
                al.close()
        assert _same_alns(device.expand_alns(index, t, m), b.want(index).alns) and c["travs"] == len(t)
        _UNF[key] = (t, m, c, index)                        # (the index is held: its id stays its own while the entry lives)
    return _UNF[key][:3]


def _assert_inputs(case):
    """ahead of every GPU run on the seven graphs: the issue's floors on the CPU oracle's records of all three batches, and in every batch's
    traversal list a read whose traversals straddle a multiple of 256 (the oracle yields records, not traversals: the list is the device's
    own with assignment off, whose expansion _unfiltered has asserted equal to the oracle's records)"""
    index, batches = case
    _assert_classes(index, batches)
    assert all(_straddles(_unfiltered(index, b)[0]) for b in batches)


def _want(index, b, alpha, min_post, first=0):
    t, m, c = _unfiltered(index, b)
    t = t.copy()
    t["read_id"] = (t["read_id"].astype(np.int64) + first).astype(np.uint32)
    alns = b.want(index).alns.copy()
    alns["read_id"] = (alns["read_id"].astype(np.int64) + first).astype(np.uint32)
    return filter_py(index, t, m, alns, alpha, min_post, b.n, first & 0xFFFFFFFF)


def _assert_batch(index, got, want, counts=None, unf_counts=None):
    t, m, best, mapq = got
    wt, wm, wal, wbest, wmapq, _ = want
    assert t.tobytes() == wt.tobytes(), np.flatnonzero(t != wt)[:10]
    assert m.tobytes() == wm.tobytes(), np.flatnonzero((m != wm).any(axis=1))[:10]
    assert _same_alns(device.expand_alns(index, t, m), wal)
    assert np.array_equal(best, wbest) and np.array_equal(mapq, wmapq)
    if counts is not None:                                  # groot_counts are those of the unfiltered run
        for k in ("received", "mapped", "multimapped", "alignments", "seeds", "travs"):
            assert counts[k] == unf_counts[k], k


def _sum_stats(wants):
    return {k: sum(w[5][k] for w in wants) for k in STAT_KEYS}


def _stats(al):
    st = al.assign_stats()
    return {k: st[k] for k in STAT_KEYS}, st["launches"]


def _feed_check(al, index, batches, alpha, min_post, first=0):
    """one batch at a time through wait(): every batch's records, best and mapq against the restatement -> the wants"""
    wants = []
    for b in batches:
        al.submit(b.seq, b.off, first_read_id=first & 0xFFFFFFFF)
        c = al.wait()
        got = al.travs() + al.assign_batch(b.n)
        wants.append(_want(index, b, alpha, min_post, first))
        _assert_batch(index, got, wants[-1], c, _unfiltered(index, b)[2])
        first += b.n
    return wants


def _straddles(t):
    rid = t["read_id"].astype(np.int64)
    idx = np.arange(256, len(t), 256)
    return bool(len(idx) and (rid[idx] == rid[idx - 1]).any())


@pytest.mark.gpu
@pytest.mark.parametrize("min_post", [0.0, 0.5])
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_device_equals_the_definition(case, hip_lib, monkeypatch, stage, rod, min_post):
    """three batches (unclipped, clipped, unclipped) through one ctx under each align stage, results in HBM or copied out, both values of
    min_post: records, path sets, best, mapq and stats are the restatement's"""
    _assert_inputs(case)
    index, batches = case
    alpha = _alpha7(index)
    _stage(monkeypatch, stage)
    al = _open(index, batches, alpha, min_post, results_on_device=rod)
    try:
        wants = _feed_check(al, index, batches, alpha, min_post)
        st, launches = _stats(al)
        assert st == _sum_stats(wants) and launches >= len(batches), (st, _sum_stats(wants))
        assert st["below" if min_post else "assigned"] > 0
    finally:
        al.close()


@pytest.mark.gpu
def test_alpha_in_global_memory(case, hip_lib, monkeypatch):
    """GROOT_TEST_ASSIGN_GLOBAL: alpha is read from global memory although it would fit in LDS"""
    _assert_inputs(case)
    index, batches = case
    alpha = _alpha7(index)
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_ASSIGN_GLOBAL", "1")
    al = _open(index, batches[:2], alpha, 0.0)
    try:
        wants = _feed_check(al, index, batches[:2], alpha, 0.0)
        assert _stats(al)[0] == _sum_stats(wants)
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
def test_redone_batches_count_once(case, hip_lib, monkeypatch, rod):
    """GROOT_TEST_SMALL_BUFFERS: every buffer starts too small, collect redoes the batch; the skipped pass filters and counts nothing"""
    _assert_inputs(case)
    index, batches = case
    alpha = _alpha7(index)
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SMALL_BUFFERS", "1")
    al = _open(index, batches[:2], alpha, 0.0, results_on_device=rod)
    try:
        wants = _feed_check(al, index, batches[:2], alpha, 0.0)
        st, launches = _stats(al)
        assert st == _sum_stats(wants) and launches > 2, (st, launches)       # (more launches than batches: passes were redone)
    finally:
        al.close()


def _collect_check(al, index, seq, alpha, min_post, depth=3, codes=None, skip=()):
    """`depth` batches in flight; every collected batch's records, best and mapq against the restatement -> the wants"""
    wants, pending, first = [], [], 0

    def collect():
        b, f = pending.pop(0)
        r = al.collect(check=False)
        assert r["status"] == (codes or {}).get(b.name, 0), (b.name, r["status"])
        if b.name not in skip:
            got = (r["travs"], r["masks"]) + al.assign_batch(b.n, r["ticket"])
            wants.append(_want(index, b, alpha, min_post, f))
            _assert_batch(index, got, wants[-1], r["counts"], _unfiltered(index, b)[2])
        al.release(r["ticket"])

    for b in seq:
        if len(pending) == depth:
            collect()
        al.submit(b.seq, b.off, first_read_id=first)
        pending.append((b, first))
        first += b.n
    while pending:
        collect()
    return wants


@pytest.mark.gpu
@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("kind", sorted(_CODE))
def test_failing_batch(case, hip_lib, monkeypatch, kind, pipelined):
    """a batch that fails with GROOT_E_NOSPACE is neither filtered nor counted; one that fails with GROOT_E_SHORT_READ or GROOT_E_REVCOMP
    is, through its other reads.  Collected alone, and with three batches in flight and good batches on both sides of it."""
    _assert_inputs(case)
    index, (b0, b1, b2) = case
    alpha = _alpha7(index)
    good = [b0.take(np.arange(3000), "good 0"), b2.take(np.arange(3000), "good 1"), b0.take(np.arange(3000, 6000), "good 2")]
    bad, bad_wants = _bad_batch(index, b1.take(np.arange(2000), "bad"), kind)
    # what the bad batch adds to the stats the records determine: the records _bad_batch names as its expectation
    extra = dict.fromkeys(STAT_KEYS[:6], 0)
    if bad_wants:
        extra = assign_py(bad_wants[0].alns, alpha, 0.0, bad.n)[3]
        assert extra["assigned"] > 500
    _stage(monkeypatch, "path_first")
    seq = good[:2] + [bad] + good[2:]
    al = _open(index, seq, alpha, 0.0, max_read_len=64, pipeline_depth=3 if pipelined else 0)
    try:
        if pipelined:
            wants = _collect_check(al, index, seq, alpha, 0.0, codes={bad.name: _CODE[kind]}, skip={bad.name})
        else:
            wants = _feed_check(al, index, good[:1], alpha, 0.0)
            al.submit(bad.seq, bad.off, first_read_id=good[0].n)
            with pytest.raises(host.GrootError) as e:
                al.wait()
            assert e.value.code == _CODE[kind]
            t, m = al.travs()
            best, mapq = al.assign_batch(bad.n)
            if kind == "long":                              # unfiltered: no flag, no MAPQ, nothing assigned
                assert not (t["flags"] & device.TRAV_MAPQ).any() and (best == NONE).all() and not mapq.any() and not t["reserved"].any()
            else:
                assert ((t["flags"] & device.TRAV_MAPQ) != 0).sum() == (best != NONE).sum() == extra["assigned"]
            wants += _feed_check(al, index, good[1:], alpha, 0.0, first=good[0].n + bad.n)
        st, _ = _stats(al)
        want = _sum_stats(wants)
        assert {k: st[k] for k in STAT_KEYS[:6]} == {k: want[k] + extra[k] for k in STAT_KEYS[:6]}, (st, want, extra)
        assert st["records_kept"] == want["records_kept"] + extra["assigned"]     # (one kept traversal per assigned read: no read of these batches has two on one path)
    finally:
        al.close()


@pytest.mark.gpu
def test_depth_three_with_empty_and_one_read_batches(case, hip_lib, monkeypatch):
    _assert_inputs(case)
    index, (b0, b1, b2) = case
    alpha = _alpha7(index)
    w0 = b0.want(index)
    rng = np.random.default_rng(5)
    noise = _of_reads("noise", ["".join(rng.choice(list("ACGT"), L)).encode() for _ in range(500)])
    empty = _of_reads("no reads", [])
    one_wide = b0.take([int(np.flatnonzero(w0.graphs > 4)[0])], "one wide read")
    one = b0.take([int(np.flatnonzero(w0.graphs == 1)[0])], "one read")
    seq = [b0, empty, one_wide, noise, one, empty, b1, one]
    assert len(noise.want(index).alns) == 0 and empty.n == 0
    _stage(monkeypatch, "path_first")
    al = _open(index, seq, alpha, 0.0, pipeline_depth=3)
    try:
        wants = _collect_check(al, index, seq, alpha, 0.0)
        st, launches = _stats(al)
        assert st == _sum_stats(wants) and launches >= len(seq) - 2
    finally:
        al.close()


@pytest.mark.gpu
def test_odd_first_read_id_and_ids_up_to_the_last(case, hip_lib, monkeypatch):
    _assert_inputs(case)
    index, (b0, b1, b2) = case
    alpha = _alpha7(index)
    sub = [b0.take(np.arange(2001), "2001"), b1.take(np.arange(3000), "3000")]
    _stage(monkeypatch, "path_first")
    al = _open(index, sub, alpha, 0.0)
    try:
        first = 2 ** 32 - 5001                              # odd; the second batch ends on read id 2^32 - 1
        wants = _feed_check(al, index, sub, alpha, 0.0, first=first)
        assert int(wants[1][0]["read_id"].max()) > 2 ** 32 - 30 and _stats(al)[0] == _sum_stats(wants)
    finally:
        al.close()


@pytest.mark.gpu
def test_coverage_counts_the_kept_records(case, hip_lib, monkeypatch):
    """report coverage beside assignment: the export equals the pileup of the kept records"""
    _assert_inputs(case)
    index, batches = case
    alpha = _alpha7(index)
    _stage(monkeypatch, "path_first")
    al = _open(index, batches[:2], alpha, 0.0)
    try:
        al.coverage_enable()
        wants = _feed_check(al, index, batches[:2], alpha, 0.0)
        records, depth = al.coverage()
        w_rec, w_depth = np.zeros_like(records), np.zeros_like(depth)
        first = 0
        for b, w in zip(batches[:2], wants):
            kept = w[2].copy()
            kept["read_id"] -= np.uint32(first)
            r, d = expand_coverage(index, kept, b.off)
            w_rec += r
            w_depth += d
            first += b.n
        assert np.array_equal(records, w_rec) and np.array_equal(depth, w_depth) and int(records.sum()) == _sum_stats(wants)["records_kept"] > 0
    finally:
        al.close()


@pytest.mark.gpu
def test_alpha_replaced_refused_in_flight_and_off_again(case, hip_lib, monkeypatch):
    _assert_inputs(case)
    index, (b0, b1, b2) = case
    alpha = _alpha7(index)
    other = alpha[::-1].copy()
    sub = [b0.take(np.arange(2500), "2500"), b2.take(np.arange(2500), "2500'")]
    _stage(monkeypatch, "path_first")
    al = _open(index, sub, pipeline_depth=2)
    try:
        assert _stats(al) == (dict.fromkeys(STAT_KEYS, 0), 0)
        with pytest.raises(host.GrootError) as e:
            al.assign_batch(0)
        assert e.value.code == -9
        for bad in (alpha[:-1], np.r_[alpha[:-1], np.nan], np.r_[alpha[:-1], -1.0], np.r_[alpha[:-1], 2e300]):
            with pytest.raises(host.GrootError) as e:
                al.assign_enable(bad, 0.0)
            assert e.value.code == -1
        with pytest.raises(host.GrootError):
            al.assign_enable(alpha, 1.5)
        assert _stats(al)[1] == 0
        al.assign_enable(alpha, 0.0)
        wants = _feed_check(al, index, sub[:1], alpha, 0.0)
        al.assign_enable(other, 0.5)                        # replaced between batches: the stats run on
        wants += _feed_check(al, index, sub[1:], other, 0.5, first=sub[0].n)
        assert _stats(al)[0] == _sum_stats(wants)
        al.submit(sub[0].seq, sub[0].off)                   # refused with a batch in flight
        with pytest.raises(host.GrootError) as e:
            al.assign_enable(alpha, 0.0)
        assert e.value.code == -9
        with pytest.raises(host.GrootError):
            al.assign_enable(None)
        al.wait()
        al.assign_reset()
        launches = _stats(al)[1]
        assert _stats(al)[0] == dict.fromkeys(STAT_KEYS, 0) and launches >= 3
        # off again: the unfiltered run's outputs, no launch
        al.assign_enable(None)
        al.submit(sub[1].seq, sub[1].off)
        c = al.wait()
        t, m = al.travs()
        ut, um, uc = _unfiltered(index, sub[1])
        assert t.tobytes() == ut.tobytes() and m.tobytes() == um.tobytes() and {k: c[k] for k in ("alignments", "travs", "mapped")} == {k: uc[k] for k in ("alignments", "travs", "mapped")}
        assert _stats(al) == (dict.fromkeys(STAT_KEYS, 0), launches)        # no launch while off
        with pytest.raises(host.GrootError):
            al.assign_batch(sub[1].n)
    finally:
        al.close()


@pytest.mark.gpu
def test_not_with_the_counters_of_s_of_r(case, hip_lib):
    """shared reads, equivalence classes, assigned coverage and pairing count S(r), which assignment collapses: GROOT_E_UNSUPPORTED from
    whichever enable comes second"""
    _assert_inputs(case)
    index, batches = case
    alpha = _alpha7(index)
    al = _open(index, batches[:1])
    try:
        for name in ("shared_enable", "ec_enable", "acov_enable", "pairs_enable"):
            getattr(al, name)(True)
            with pytest.raises(host.GrootError) as e:
                al.assign_enable(alpha, 0.0)
            assert e.value.code == -10, name
            getattr(al, name)(False)
            if name == "acov_enable":
                al.ec_enable(False)
        al.assign_enable(alpha, 0.0)
        for name in ("shared_enable", "ec_enable", "acov_enable", "pairs_enable"):
            with pytest.raises(host.GrootError) as e:
                getattr(al, name)(True)
            assert e.value.code == -10, name
        al.coverage_enable()                                # coverage is allowed
        al.assign_enable(None)
        al.shared_enable()
    finally:
        al.close()


@pytest.mark.gpu
def test_two_contexts_against_one(case, hip_lib, monkeypatch):
    _assert_inputs(case)
    index, batches = case
    alpha = _alpha7(index)
    parts = [batches[0].take(np.arange(0, 3000), "a"), batches[1].take(np.arange(0, 4000), "b"), batches[0].take(np.arange(3000, 6000), "c"),
             batches[2].take(np.arange(0, 3000), "d")]
    firsts = np.r_[0, np.cumsum([p.n for p in parts])].tolist()
    _stage(monkeypatch, "path_first")
    total = dict.fromkeys(STAT_KEYS, 0)
    als = [_open(index, parts, alpha, 0.0) for _ in range(2)]
    try:
        for i, p in enumerate(parts):                       # the batches alternate between the ctxs, read ids as in one run
            wants = _feed_check(als[i % 2], index, [p], alpha, 0.0, first=firsts[i])
        for al in als:
            for k, v in _stats(al)[0].items():
                total[k] += v
    finally:
        for al in als:
            al.close()
    al = _open(index, parts, alpha, 0.0)
    try:
        wants = _feed_check(al, index, parts, alpha, 0.0)
        assert _stats(al)[0] == _sum_stats(wants) == total
    finally:
        al.close()


# ---- a built graph with identical alleles ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twins(tmp_path_factory, native_libs):
    """two identical alleles on different nodes: two paths with one text"""
    tmp = tmp_path_factory.mktemp("twins")
    rng = np.random.default_rng(21)
    nodes = {1: _seq(rng, 40), 2: "GCATTGCA", 3: "GCATTGCA", 4: _seq(rng, 40)}
    paths = [("p0", [1, 2, 4]), ("p1", [1, 3, 4])]
    f = _gfa(tmp / "g.gfa", nodes, [(1, 2), (1, 3), (2, 4), (3, 4)], paths)
    index = host.Index.from_gfa_files([f], host.index_params(k=7, s=10, w=30))
    text = nodes[1] + nodes[2] + nodes[4]
    return index, _Batch("twins", *_reads_from(rng, [text], 600, L))


def _through(index, b):
    """the reads with one record on each path -> {read: the path of its first record}"""
    al = b.want(index).alns
    per = {}
    for r, p in zip(al["read_id"].tolist(), al["ref_id"].tolist()):
        per.setdefault(r, []).append(p)
    return {r: s[0] for r, s in sorted(per.items()) if sorted(s) == [0, 1]}


def test_twins_inputs(twins):
    index, b = twins
    both = _through(index, b)
    # either path comes first in at least 20 reads: each alpha lets the first traversal die in some reads and the second in others
    assert index.view.n_paths == 2 and min(sum(1 for p in both.values() if p == q) for q in (0, 1)) >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [(1.0, 3.0), (3.0, 1.0)])
def test_twin_alleles(twins, hip_lib, monkeypatch, alpha):
    """every read through the allele has two traversals in one graph with disjoint path sets; which of the two lies on path 0 differs from
    read to read (test_twins_inputs).  With alpha = (1, 3) the traversal on path 0 dies -- the first one of some reads, and the second gets
    FIRST -- and with (3, 1) the other one"""
    index, b = twins
    both = _through(index, b)
    assert min(sum(1 for p in both.values() if p == q) for q in (0, 1)) >= 20
    t, m, _ = _unfiltered(index, b)
    two = [r for r in both if (t["read_id"] == r).sum() == 2 and not (m[t["read_id"] == r][0] & m[t["read_id"] == r][1]).any()]
    assert len(two) >= 20, len(two)
    _stage(monkeypatch, "path_first")
    al = _open(index, [b], alpha, 0.0)
    try:
        (want,) = _feed_check(al, index, [b], alpha, 0.0)
        ft = want[0]
        best = 1 if alpha[1] > alpha[0] else 0
        dies_first = 0
        for r in two:
            fl = ft["flags"][ft["read_id"] == r].tolist()
            alive = 0 if both[r] == best else 1            # the traversal on `best`: the read's first record lies on path both[r]
            dies_first += alive
            assert fl[alive] & device.TRAV_FIRST and fl[alive] & device.TRAV_MAPQ and not fl[1 - alive] & (device.TRAV_FIRST | device.TRAV_MAPQ)
        print("first traversal dies in", dies_first, "reads, the second in", len(two) - dies_first)
        assert max(dies_first, len(two) - dies_first) >= 20
        assert _stats(al)[0] == _sum_stats([want])
    finally:
        al.close()
