"""The three counters behind the order stage -- report coverage (kernels_cov.hpp), shared reads (kernels_shared.hpp) and equivalence
classes (kernels_ec.hpp + the host fold ec_collect / ec_set_of / ec_gather) -- on an index built so that reads reach the branches the
arg-annot / resfinder reads of test_coverage.py, test_shared_reads.py and test_abundance.py never do: reads in exactly kSharedSegs = 4
graphs (a used fourth segment, keys that differ in it alone), reads in 5 and 7 graphs (the slow path for the reason it exists, with sets
of several hundred paths over three mask words), fast-path reads next to them in one batch, graphs of 1, 64, 65, 128 and 129 paths (both
sides of both mask-word edges), read ids near 2^32, empty and one-read batches, batches that fail.

Seven graphs share named segments: a read inside a segment has records in every graph that holds it, on all paths of each.  The
expectation of every batch is recomputed in numpy / plain Python from the CPU oracle's records of that batch, never from device output;
each GPU test first asserts, from those records, the property it was written for."""
import ctypes as C

import numpy as np
import pytest

from groot_amd import _ffi, device, host
from oracle import oracle_py as O
from test_abundance import _dev_ecs, ecs_of_alns
from test_coverage import STAGES, _stage, expand_coverage
from test_path_pass import _gfa, _reads_from, _seq
from test_shared_reads import _dev_pairs, pairs_of_alns

L, THR = 28, 0.9
NP = [70, 64, 65, 129, 1, 128, 20]                       # paths per graph: 477 in all, three mask words
SEGS = [("A", (0, 1, 2, 3)), ("B", (0, 1, 2, 4)), ("C", (0, 1, 2, 3, 4)), ("D", (0, 1, 2, 3, 4, 5, 6)), ("E", (5, 6)), ("F", (4, 5, 6))]
N_READS = {"plain": 6000, "clip": 14000, "plain2": 6000}  # (clipped reads map less often: more of them, so that every bin clears its floor)


# ---- the graphs ---------------------------------------------------------------------------------------------------------------

def _graph(rng, path, g, shared):
    """graph g: a unique 35-base head, every shared segment that holds g (45 bases, verbatim in each of its graphs) followed by a unique
    30-base spacer, a fan of NP[g] alleles of 3..5 bases, a unique 35-base tail; path p = the chain + allele p + the tail"""
    chain = [_seq(rng, 35)]
    for name, members in SEGS:
        if g in members:
            chain += [shared[name], _seq(rng, 30)]
    alleles = []
    while len(alleles) < NP[g]:
        a = _seq(rng, int(rng.integers(3, 6)))
        if a not in alleles:
            alleles.append(a)
    tail = _seq(rng, 35)
    nodes = {i + 1: s for i, s in enumerate(chain + alleles + [tail])}
    m, t = len(chain), len(chain) + len(alleles) + 1
    edges = [(i, i + 1) for i in range(1, m)]
    for a in range(m + 1, t):
        edges += [(m, a), (a, t)]
    paths = [("g%dp%d" % (g, p), list(range(1, m + 1)) + [m + 1 + p, t]) for p in range(NP[g])]
    return _gfa(path, nodes, edges, paths), ["".join(chain) + a + tail for a in alleles[:3]]


class _Want:
    """what one batch adds to the counters, from the oracle's records of it"""

    def __init__(self, index, seq, off):
        run = O.Run(index, THR)
        run.batch(seq, off)
        al = self.alns = run.alns().astype(device.ALN_DTYPE)
        n, P = len(off) - 1, index.view.n_paths
        assert P < 1024 and index.view.n_graphs < 64
        self.records, self.depth = expand_coverage(index, al, off)
        rid = al["read_id"].astype(np.int64)
        self.read_graph = np.unique(rid * 64 + al["graph_id"])                     # (read, graph), each once
        self.graphs = np.bincount(self.read_graph >> 6, minlength=n)               # graphs per read
        self.read_ref = np.unique(rid * 1024 + al["ref_id"])
        self.size = np.bincount(self.read_ref >> 10, minlength=n)                  # |S(r)|
        self.ecs = dict(ecs_of_alns(al))
        self.tri = _tri_of_ecs(self.ecs, P)

    def graph_sets(self, k):
        """the graph sets of the reads in exactly k graphs"""
        out = set()
        r, g = self.read_graph >> 6, self.read_graph & 63
        starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
        for s, e in zip(starts, np.r_[starts[1:], len(r)]):
            if e - s == k:
                out.add(tuple(g[s:e].tolist()))
        return out

    def fast_sets(self, max_segs):
        """the distinct S(r) among the reads in at most max_segs graphs: one slot each in the batch's table"""
        r, p = self.read_ref >> 10, self.read_ref & 1023
        starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]]) if len(r) else np.zeros(0, dtype=np.int64)
        return {p[s:e].tobytes() for s, e in zip(starts, np.r_[starts[1:], len(r)]) if self.graphs[r[s]] <= max_segs}


def _tri_of_ecs(ecs, n_paths):
    """pairs per distinct set, not per read: every (a, b), a <= b, of a set gets the set's reads"""
    tri = np.zeros((n_paths, n_paths), dtype=np.int64)
    for ids, c in ecs.items():
        i = np.array(ids, dtype=np.int64)
        tri[np.ix_(i, i)] += c
    return np.triu(tri)


class _Batch:
    def __init__(self, name, seq, off):
        self.name, self.seq, self.off, self.n = name, seq, np.asarray(off, dtype=np.uint64), len(off) - 1
        self._want = None

    def want(self, index):
        if self._want is None:
            self._want = _Want(index, self.seq, self.off)
        return self._want

    def take(self, idx, name):
        """the reads idx (every read of these batches has L bases)"""
        assert len(self.seq) == self.n * L
        idx = np.asarray(idx, dtype=np.int64)
        return _Batch(name, self.seq.reshape(self.n, L)[idx].reshape(-1).copy(), np.arange(len(idx) + 1, dtype=np.uint64) * L)


def _of_reads(name, reads):
    return _Batch(name, *O.pack_reads(reads))


def _build_case(tmp):
    rng = np.random.default_rng(13)
    shared = {name: _seq(rng, 45) for name, _ in SEGS}
    files, texts = [], []
    for g in range(len(NP)):
        f, t = _graph(rng, tmp / ("g%d.gfa" % g), g, shared)
        files.append(f)
        texts += t
    index = host.Index.from_gfa_files(files, host.index_params(k=7, s=10, w=30))
    batches = [_Batch(name, *_reads_from(np.random.default_rng(seed), texts, N_READS[name], L, clip=name == "clip"))
               for name, seed in (("plain", 131), ("clip", 132), ("plain2", 133))]
    return index, batches


@pytest.fixture(scope="module")
def case(tmp_path_factory, native_libs):
    """(the index of the seven graphs, [unclipped, clipped, unclipped with another seed])"""
    return _build_case(tmp_path_factory.mktemp("counter_edges"))


def _assert_edges(w, clip=False):
    """the floors every batch of the GPU tests must clear (conditions on the generator, not measurements)"""
    per = np.bincount(w.graphs, minlength=8)
    assert all(per[k] >= 100 for k in (1, 2, 3, 4, 5)) and per[6:].sum() >= 50, per
    assert {(0, 1, 2, 3), (0, 1, 2, 4)} <= w.graph_sets(4), w.graph_sets(4)      # keys that agree on three segments, differ in the fourth
    assert int(((w.graphs > 4) & (w.size > 64)).sum()) >= 100 and w.size.max() > 256
    if clip:
        a = w.alns
        assert (a["start_clip"] == 1).sum() > 100 and (a["end_clip"] == 1).sum() > 100 and (a["pos"] == 0).sum() > 100


# ---- CPU: the inputs are what the GPU tests need -------------------------------------------------------------------------------------

def test_inputs_reach_every_edge(case):
    index, batches = case
    assert index.view.path_words == 3 and index.view.n_paths == sum(NP)
    per_graph = np.diff(index.arrays["graph_path_off"].astype(np.int64)).tolist()
    assert per_graph == NP and {1, 64, 65, 128, 129} <= set(per_graph)
    for b in batches:
        w = b.want(index)
        print(b.name, "graphs/read", np.bincount(w.graphs, minlength=8).tolist(), "slow and wide", int(((w.graphs > 4) & (w.size > 64)).sum()),
              "max |S|", int(w.size.max()), "4-graph sets", sorted(w.graph_sets(4)), "ECs", len(w.ecs))
        _assert_edges(w, clip=b.name == "clip")
        # bit 63 of a word and bit 0 of the next, in one set
        assert any({63, 64} <= set(i) for i in w.ecs) and any(len(i) == 1 for i in w.ecs)


def test_expectation_per_distinct_set_equals_per_read(case):
    """the pair counts built per distinct set == test_shared_reads.pairs_of_alns (per read) on a slice with wide sets in it"""
    index, batches = case
    sub = batches[0].take(np.arange(300), "slice")
    w = sub.want(index)
    assert (w.graphs > 4).sum() > 5 and w.size.max() > 256
    a, b = np.nonzero(w.tri)
    assert {(int(x), int(y)): int(w.tri[x, y]) for x, y in zip(a, b)} == pairs_of_alns(w.alns)
    assert sum(w.ecs.values()) == int((w.graphs > 0).sum()) == len(np.unique(w.alns["read_id"]))


# ---- the device side -----------------------------------------------------------------------------------------------------------------

class _Total:
    """the sum of the given batches' expectations"""

    def __init__(self, index, wants, max_segs=4):
        P = index.view.n_paths
        self.records = np.zeros(P, dtype=np.uint64)
        self.depth = np.zeros(int(index.arrays["path_len"].astype(np.int64).sum()), dtype=np.uint64)
        self.tri = np.zeros((P, P), dtype=np.int64)
        self.ecs = {}
        self.reads = self.slow = self.fast_sets = 0
        for w in wants:
            self.records += w.records
            self.depth += w.depth
            self.tri += w.tri
            for i, c in w.ecs.items():
                self.ecs[i] = self.ecs.get(i, 0) + c
            self.reads += int((w.graphs > 0).sum())
            self.slow += int((w.graphs > max_segs).sum())
            self.fast_sets += len(w.fast_sets(max_segs))

    def pairs(self):
        a, b = np.nonzero(self.tri)
        return {(int(x), int(y)): int(self.tri[x, y]) for x, y in zip(a, b)}


def _open(index, batches, cov=True, sh=True, ec=True, **kw):
    kw.setdefault("memo_budget_mb", device.MEMO_OFF)
    kw.setdefault("max_read_len", 256)
    al = device.Aligner(index, threshold=THR, max_batch_reads=max(1024, max(b.n for b in batches)), **kw)
    if cov:
        al.coverage_enable()
    if sh:
        al.shared_enable()
    if ec:
        al.ec_enable()
    return al


def _feed(al, batches, first=0):
    """one batch at a time, first_read_id running on"""
    for b in batches:
        al.submit(b.seq, b.off, first_read_id=first)
        c = al.wait()
        assert c["received"] == b.n
        first += b.n
    return first


def _feed_pipelined(al, batches, first=0, depth=3):
    """`depth` batches in flight, collected oldest first -> the status of every batch"""
    status, pending = [], 0

    def collect():
        r = al.collect(check=False)
        status.append(r["status"])
        al.release(r["ticket"])

    for b in batches:
        if pending == depth:
            collect()
            pending -= 1
        al.submit(b.seq, b.off, first_read_id=first)
        pending += 1
        first += b.n
    for _ in range(pending):
        collect()
    return status


def _first_diff(got, want):
    keys = sorted(set(got) | set(want))
    bad = [(k, got.get(k), want.get(k)) for k in keys if got.get(k) != want.get(k)]
    return "%d differ, first (key, device, oracle): %s" % (len(bad), bad[:5])


def _check(al, index, wants, max_segs=4, cov=True, sh=True, ec=True):
    """all three counters and all stats == the sum of the batches' expectations"""
    t = _Total(index, wants, max_segs)
    if cov:
        records, depth = al.coverage()
        assert np.array_equal(records, t.records), np.flatnonzero(records != t.records)[:10]
        assert np.array_equal(depth, t.depth), np.flatnonzero(depth != t.depth)[:10]
    if sh:
        got, want = _dev_pairs(al), t.pairs()
        assert got == want, _first_diff(got, want)
        st = al.shared_stats()
        print("shared", st)
        assert st["reads"] == t.reads and st["slow_reads"] == t.slow and st["distinct_sets"] == t.fast_sets, (st, t.reads, t.slow, t.fast_sets)
    if ec:
        got, want = dict(_dev_ecs(al)), t.ecs
        assert got == want, _first_diff(got, want)
        st = al.ec_stats()
        print("ec", st)
        assert st["reads"] == t.reads and st["distinct"] == len(t.ecs) and st["slow_reads"] == t.slow, (st, t.reads, len(t.ecs), t.slow)
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
@pytest.mark.parametrize("stage", sorted(STAGES))
def test_every_edge_at_once(case, hip_lib, monkeypatch, stage, rod):
    """three batches (unclipped, clipped, unclipped) through one ctx, all three counters on, the real max_segs: reads of 1..4 graphs on
    the fast path next to reads of 5 and 7 graphs on the slow one, under each align stage, results in HBM or copied out"""
    index, batches = case
    wants = [b.want(index) for b in batches]
    for b, w in zip(batches, wants):
        _assert_edges(w, clip=b.name == "clip")
    _stage(monkeypatch, stage)
    al = _open(index, batches, results_on_device=rod)
    try:
        _feed(al, batches)
        t = _check(al, index, wants)
        assert t.slow == sum(int((w.graphs > 4).sum()) for w in wants) > 0
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("on", ["ec_only", "shared_only"])
def test_one_of_shared_and_ec(case, hip_lib, monkeypatch, on):
    """ECs without shared reads (expand only clears the table, the slow kernel is not launched) and shared reads without ECs"""
    index, batches = case
    wants = [b.want(index) for b in batches]
    assert all((w.graphs > 4).sum() > 32 and (w.graphs == 4).sum() >= 100 for w in wants)
    _stage(monkeypatch, "path_first")
    al = _open(index, batches, sh=on == "shared_only", ec=on == "ec_only")
    try:
        _feed(al, batches)
        _check(al, index, wants, sh=on == "shared_only", ec=on == "ec_only")
        with pytest.raises(host.GrootError):
            al.shared() if on == "ec_only" else al.ecs()
    finally:
        al.close()


@pytest.mark.gpu
def test_few_many_and_no_slow_reads(case, hip_lib, monkeypatch):
    """ec_collect fetches the records of up to 32 slow reads one by one and of more in one span: a batch with 7 slow reads among fast
    ones, one with hundreds, one with none, through one ctx"""
    index, batches = case
    w0 = batches[0].want(index)
    slow, fast = np.flatnonzero(w0.graphs > 4), np.flatnonzero(w0.graphs <= 4)
    few = batches[0].take(np.sort(np.r_[fast[:3000], slow[[0, 1, 2, len(slow) // 2, -3, -2, -1]]]), "few")
    none = batches[0].take(fast, "none")
    seq = [few, batches[0], none]
    wants = [b.want(index) for b in seq]
    n_slow = [int((w.graphs > 4).sum()) for w in wants]
    assert n_slow[0] == 7 and n_slow[1] > 32 and n_slow[2] == 0, n_slow
    assert max(w.size[w.graphs > 4].max() for w in wants[:2]) > 256 and (wants[2].graphs == 4).sum() >= 100
    _stage(monkeypatch, "path_first")
    al = _open(index, seq)
    try:
        first = 0
        for i, b in enumerate(seq):
            first = _feed(al, [b], first)
            _check(al, index, wants[:i + 1])
    finally:
        al.close()


@pytest.mark.gpu
def test_forced_slow_mode(case, hip_lib, monkeypatch):
    """GROOT_TEST_SHARED_SLOW on this index: the reads of 2..4 graphs join the reads of 5 and 7 on the slow path"""
    index, batches = case
    wants = [b.want(index) for b in batches[:2]]
    assert all((w.graphs > 4).sum() > 32 and ((w.graphs > 1) & (w.graphs <= 4)).sum() >= 300 for w in wants)
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_SHARED_SLOW", "1")
    al = _open(index, batches[:2])
    try:
        _feed(al, batches[:2])
        t = _check(al, index, wants, max_segs=1)
        assert t.slow == sum(int((w.graphs > 1).sum()) for w in wants)
    finally:
        al.close()


@pytest.mark.gpu
def test_table_growth_with_slow_reads_in_flight(case, hip_lib, monkeypatch):
    """GROOT_TEST_EC_SLOTS=64, three batches in flight, seven batches of rising size (ec_reserve sizes the table by the reads in
    flight): the table grows while batches with slow reads are between their merge and their collect"""
    index, (b0, b1, b2) = case
    seq = [b0.take(np.arange(500), "500"), b0.take(np.arange(500, 2500), "2000"), b2, b1, b0, b2.take(np.arange(3000), "3000"),
           b1.take(np.arange(1000), "1000")]
    wants = [b.want(index) for b in seq]
    assert all((w.graphs > 4).sum() > 0 and (w.graphs == 4).sum() > 0 for w in wants)
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_EC_SLOTS", "64")
    al = _open(index, seq, pipeline_depth=3)
    try:
        assert _feed_pipelined(al, seq) == [0] * len(seq)
        _check(al, index, wants)
        assert al.ec_stats()["grows"] >= 2
    finally:
        al.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rod", [False, True])
def test_large_read_ids(case, hip_lib, monkeypatch, rod):
    """read ids from 4 000 000 000 on (read_id - first_read_id in the kernels): the counters hold no ids, so the same totals"""
    index, batches = case
    wants = [b.want(index) for b in batches]
    first = 4_000_000_000
    assert first + sum(b.n for b in batches) < 1 << 32 and all((w.graphs > 4).sum() > 32 for w in wants)
    _stage(monkeypatch, "path_first")
    al = _open(index, batches, results_on_device=rod)
    try:
        assert _feed(al, batches, first) == first + sum(b.n for b in batches)
        _check(al, index, wants)
        al.submit(batches[0].seq, batches[0].off, first_read_id=first)
        al.wait()
        t, _ = al.travs()
        assert len(t) and t["read_id"].min() >= first and t["read_id"].max() < first + batches[0].n
    finally:
        al.close()


@pytest.mark.gpu
def test_empty_and_one_read_batches_between_full_ones(case, hip_lib, monkeypatch):
    """a batch without a record (n_trav == 0), a batch of one mapped read (a slow one), a batch of one unmapped read, between two full
    batches"""
    index, (b0, b1, b2) = case
    w0 = b0.want(index)
    rng = np.random.default_rng(5)
    noise = _of_reads("noise", ["".join(rng.choice(list("ACGT"), L)).encode() for _ in range(2000)])
    one = b0.take([int(np.flatnonzero(w0.graphs > 4)[0])], "one mapped")
    lost = noise.take([0], "one unmapped")
    seq = [b0, noise, one, lost, b2]
    wants = [b.want(index) for b in seq]
    assert len(wants[1].alns) == 0 and len(wants[3].alns) == 0 and wants[2].graphs[0] > 4 and wants[2].size[0] > 256
    _stage(monkeypatch, "path_first")
    al = _open(index, seq)
    try:
        _feed(al, seq)
        t = _check(al, index, wants)
        assert t.reads == int((w0.graphs > 0).sum()) + int((wants[4].graphs > 0).sum()) + 1
    finally:
        al.close()


# ---- keys that differ in the fourth segment alone, met in one probe run of the run-wide table --------------------------------------------
# The table is kept at most half full and the hash covers all four segments, so on a batch of thousands of reads two such keys never
# share a probe run and ec_same is never asked to tell them apart.  Here the run is arranged: ec_hash is restated, a table of a few
# slots is requested (GROOT_TEST_EC_SLOTS) and one-read batches are chosen so that the second key's probe walks over the first key's slot.
_M64 = (1 << 64) - 1


def _ec_hash(graphs, masks):
    """kernels_ec.hpp ec_hash over the used segments: graphs [n], masks [n][pw]"""
    h = 0x2545F4914F6CDD1D
    for g, m in zip(graphs, masks):
        h ^= (g + 0x9E3779B97F4A7C15 + (h << 6) + (h >> 2)) & _M64
        for w in m:
            h ^= (w + 0x9E3779B97F4A7C15 + (h << 6) + (h >> 2)) & _M64
            h ^= h >> 31
            h = h * 0xBF58476D1CE4E5B9 & _M64
            h ^= h >> 29
    h ^= h >> 33
    h = h * 0xFF51AFD7ED558CCD & _M64
    h ^= h >> 33
    return h


def _key_of(index, ids):
    """the table key of S(r) = ids: (graphs ascending, the path set of each as path_words words)"""
    gpo = index.arrays["graph_path_off"].astype(np.int64)
    pw = index.view.path_words
    graphs, masks = [], []
    for p in ids:
        g = int(np.searchsorted(gpo, p, side="right")) - 1
        if not graphs or graphs[-1] != g:
            graphs.append(g)
            masks.append([0] * pw)
        q = p - int(gpo[g])
        masks[-1][q >> 6] |= 1 << (q & 63)
    return tuple(graphs), tuple(tuple(m) for m in masks)


def _probe(table, cap, key):
    """linear probing as ec_add does it -> (the keys of the occupied slots met, the slot taken or found)"""
    met, s = [], _ec_hash(*key) & (cap - 1)
    while s in table and table[s] != key:
        met.append(table[s])
        s = (s + 1) & (cap - 1)
    return met, s


def _colliding_order(keys, x, y):
    """(table size, an order of one-key batches ending in the second of x / y) in which that key's probe meets the slot of the other, or None"""
    for cap in (4, 8, 16, 32, 64):
        for first, second in ((x, y), (y, x)):
            s1, s2 = _ec_hash(*first) & (cap - 1), _ec_hash(*second) & (cap - 1)
            gap = (s1 - s2) & (cap - 1)                          # slots second walks over before it reaches first
            if gap + 2 > cap // 2:                               # (the table stays at most half full: no growth, no rehash)
                continue
            table, order = {s1: first}, [first]
            for t in range(gap):                                 # fill s2, s2 + 1, ... s1 - 1 with other keys, in this order
                slot = (s2 + t) & (cap - 1)
                pad = next((k for k in keys if k not in order and k != second and _probe(table, cap, k)[1] == slot), None)
                if pad is None:
                    break
                table[slot] = pad
                order.append(pad)
            else:
                return cap, order + [second]
    return None


@pytest.mark.gpu
def test_keys_that_differ_in_the_fourth_segment_share_a_probe_run(case, hip_lib, monkeypatch):
    """S(r) over graphs (0, 1, 2, 3) and over (0, 1, 2, 4) with the same paths in 0, 1, 2: two keys of the run-wide table that agree on
    three segments.  One-read batches in an order in which the probe of the second walks over the slot of the first: two ECs, not one."""
    index, (b0, b1, b2) = case
    w0 = b0.want(index)
    reads = {}                                                   # S(r) -> a read with it, fast-path reads only
    r, p = w0.read_ref >> 10, w0.read_ref & 1023
    starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
    for s, e in zip(starts, np.r_[starts[1:], len(r)]):
        if w0.graphs[r[s]] <= 4:
            reads.setdefault(tuple(p[s:e].tolist()), int(r[s]))
    keys = {_key_of(index, ids): ids for ids in reads}
    all_of = lambda gs: next(k for k in keys if k[0] == gs and all(sum(bin(w).count("1") for w in m) == NP[g] for g, m in zip(gs, k[1])))
    x, y = all_of((0, 1, 2, 3)), all_of((0, 1, 2, 4))
    assert x[1][:3] == y[1][:3] and x[0][:3] == y[0][:3] and x[0][3] != y[0][3]
    found = _colliding_order(sorted(keys), x, y)
    assert found, "no order of one-read batches brings the two keys into one probe run: ec_hash changed? restate it above"
    cap, order = found
    table = {}
    for k in order[:-1]:
        met, s = _probe(table, cap, k)
        table[s] = k
    met, s = _probe(table, cap, order[-1])
    assert (x in met or y in met) and 2 * len(order) <= cap, (cap, len(order), len(met))
    print("table of %d slots, %d one-read batches, the last probes over %d occupied slots" % (cap, len(order), len(met)))
    seq = [b0.take([reads[keys[k]]], "one read") for k in order]
    wants = [b.want(index) for b in seq]
    assert all(tuple(sorted(w.ecs)) == (keys[k],) for w, k in zip(wants, order))
    _stage(monkeypatch, "path_first")
    monkeypatch.setenv("GROOT_TEST_EC_SLOTS", str(cap))
    al = _open(index, seq)
    try:
        _feed(al, seq)
        _check(al, index, wants)
        st = al.ec_stats()
        assert st["grows"] == 0 and st["distinct"] == len(order) and st["slow_reads"] == 0, st
    finally:
        al.close()


def _shared_hash(graphs, masks):
    """kernels_shared.hpp shared_hash over the used segments"""
    h = 0x9E3779B97F4A7C15
    for g, m in zip(graphs, masks):
        for v in (g,) + tuple(m):
            h ^= (v + 0x9E3779B97F4A7C15 + (h << 6) + (h >> 2)) & _M64
            h ^= h >> 31
            h = h * 0xBF58476D1CE4E5B9 & _M64
            h ^= h >> 29
    return h


@pytest.mark.gpu
def test_sets_that_differ_in_the_fourth_segment_share_a_slot_of_the_batch_table(case, hip_lib, monkeypatch):
    """the same two sets in the per-batch table of shared_insert_kernel (2^k >= 2 n_reads slots): a batch so small that both hash to one
    slot, so that whichever read comes second is compared with the owner by same_set -- through the fourth segment"""
    index, (b0, b1, b2) = case
    w0 = b0.want(index)
    full = lambda gs: tuple(p for g in gs for p in range(sum(NP[:g]), sum(NP[:g + 1])))
    ids_x, ids_y = full((0, 1, 2, 3)), full((0, 1, 2, 4))
    assert ids_x in w0.ecs and ids_y in w0.ecs
    x, y = _key_of(index, ids_x), _key_of(index, ids_y)
    tab = next((t for t in (4, 8, 16, 32, 64, 128) if (_shared_hash(*x) ^ _shared_hash(*y)) & (t - 1) == 0), None)
    assert tab, "the two sets share a slot in no small table: shared_hash or the graphs changed? pick another pair / restate the hash above"
    r, p = w0.read_ref >> 10, w0.read_ref & 1023
    starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]])
    first = {}
    for s, e in zip(starts, np.r_[starts[1:], len(r)]):
        first.setdefault(tuple(p[s:e].tolist()), int(r[s]))
    rng = np.random.default_rng(7)
    reads = [bytes(b0.seq[i * L:(i + 1) * L]) for i in (first[ids_x], first[ids_y])]
    reads += ["".join(rng.choice(list("ACGT"), L)).encode() for _ in range(tab // 2 - 2)]      # (records of none: they only size the table)
    b = _of_reads("two sets, %d slots" % tab, reads)
    w = b.want(index)
    assert w.ecs == {ids_x: 1, ids_y: 1} and b.n == tab // 2
    _stage(monkeypatch, "path_first")
    for sh, ec in ((True, True), (True, False), (False, True)):
        al = _open(index, [b], sh=sh, ec=ec)
        try:
            _feed(al, [b, b])
            _check(al, index, [w, w], sh=sh, ec=ec)
        finally:
            al.close()


def _bad_batch(index, good, kind):
    """reads of `good` with one bad read in the middle -> (the batch, what it must add to the counters)"""
    reads = [bytes(good.seq[i * L:(i + 1) * L]) for i in range(good.n)]
    mid = good.n // 2
    if kind == "long":            # longer than the ctx's max_read_len: GROOT_E_NOSPACE, the batch is not counted
        reads[mid] = reads[mid] + reads[mid + 1] + reads[mid + 2]
        return _of_reads(kind, reads), []
    if kind == "short":           # shorter than k: GROOT_E_SHORT_READ; the oracle refuses such a batch, so its other reads stand for it
        rest = _of_reads("short, rest", reads[:mid] + reads[mid + 1:]).want(index)
        reads[mid] = reads[mid][:5]
        return _of_reads(kind, reads), [rest]
    if kind == "lower":           # a lower-case read: GROOT_E_REVCOMP; the oracle runs the batch and counts the panic
        w = good.want(index)
        mid = int(np.flatnonzero((w.graphs > 0) & (np.arange(good.n) >= mid))[0])
        reads[mid] = reads[mid].lower()
        b = _of_reads(kind, reads)
        return b, [b.want(index)]
    raise ValueError(kind)


_CODE = {"long": -6, "short": -7, "lower": -8}


@pytest.mark.gpu
@pytest.mark.parametrize("pipelined", [False, True])
@pytest.mark.parametrize("kind", sorted(_CODE))
def test_failing_batch(case, hip_lib, monkeypatch, kind, pipelined):
    """include/groot_hip.h: a batch that fails with GROOT_E_NOSPACE is not counted; one that fails with GROOT_E_SHORT_READ or
    GROOT_E_REVCOMP is counted whole (the records of its other reads, which remain readable).  Collected alone, and with three batches
    in flight and good batches on both sides of it."""
    index, (b0, b1, b2) = case
    good = [b0.take(np.arange(3000), "good 0"), b2.take(np.arange(3000), "good 1"), b0.take(np.arange(3000, 6000), "good 2"),
            b2.take(np.arange(3000, 6000), "good 3")]
    bad, bad_wants = _bad_batch(index, b1.take(np.arange(2000), "bad"), kind)
    gw = [b.want(index) for b in good]
    assert all((w.graphs > 4).sum() > 32 and (w.graphs == 4).sum() > 20 for w in gw)
    if bad_wants:
        assert (bad_wants[0].graphs > 4).sum() > 0 and len(bad_wants[0].alns) > 1000
    _stage(monkeypatch, "path_first")
    seq = good[:2] + [bad] + good[2:]
    al = _open(index, seq, max_read_len=64, pipeline_depth=3 if pipelined else 0)
    try:
        if pipelined:
            assert _feed_pipelined(al, seq) == [0, 0, _CODE[kind], 0, 0]
            _check(al, index, gw[:2] + bad_wants + gw[2:])
        else:
            first = _feed(al, good[:1])
            al.submit(bad.seq, bad.off, first_read_id=first)
            with pytest.raises(host.GrootError) as e:
                al.wait()
            assert e.value.code == _CODE[kind]
            _check(al, index, gw[:1] + bad_wants)
            _feed(al, good[1:2], first + bad.n)
            _check(al, index, gw[:2] + bad_wants)
    finally:
        al.close()


@pytest.mark.gpu
def test_export_sizes_through_the_abi(case, hip_lib, monkeypatch):
    """groot_hip_shared_export with cap = 0 and 0 < cap < n_pairs writes the first cap pairs and reports n_pairs; groot_hip_ec_export
    with cap_ec or cap_ids one too small returns GROOT_E_NOSPACE and writes nothing"""
    index, batches = case
    b = batches[0].take(np.arange(2000), "2000")
    w = b.want(index)
    assert (w.graphs > 4).sum() > 32 and (w.graphs == 4).sum() > 20
    _stage(monkeypatch, "path_first")
    al = _open(index, [b], cov=False)
    try:
        _feed(al, [b])
        lib, h = device.lib(), al._h
        a, bb, cnt = al.shared()
        n_pairs = len(a)
        assert n_pairs == int((w.tri > 0).sum()) > 1000
        GUARD32, GUARD64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
        n = C.c_uint64(0)
        assert lib.groot_hip_shared_export(h, None, None, None, C.c_uint64(0), C.byref(n)) == 0 and n.value == n_pairs
        for cap in (1, n_pairs // 2, n_pairs - 1):
            pa, pb, pc = np.full(n_pairs, GUARD32, dtype=np.uint32), np.full(n_pairs, GUARD32, dtype=np.uint32), np.full(n_pairs, GUARD64, dtype=np.uint64)
            n = C.c_uint64(0)
            rc = lib.groot_hip_shared_export(h, _ffi.as_ptr(pa, C.c_uint32), _ffi.as_ptr(pb, C.c_uint32), _ffi.as_ptr(pc, C.c_uint64), C.c_uint64(cap), C.byref(n))
            assert rc == 0 and n.value == n_pairs
            assert np.array_equal(pa[:cap], a[:cap]) and np.array_equal(pb[:cap], bb[:cap]) and np.array_equal(pc[:cap], cnt[:cap])
            assert np.all(pa[cap:] == GUARD32) and np.all(pb[cap:] == GUARD32) and np.all(pc[cap:] == GUARD64)
        off, ids, ec_cnt = al.ecs()
        ne, ni = len(ec_cnt), len(ids)
        assert ne == len(w.ecs) > 10 and ni == sum(len(i) for i in w.ecs)
        for cap_ec, cap_ids in ((ne - 1, ni), (ne, ni - 1)):
            o = np.full(ne + 2, GUARD64, dtype=np.uint64)
            i = np.full(ni + 1, GUARD32, dtype=np.uint32)
            c = np.full(ne + 1, GUARD64, dtype=np.uint64)
            me, mi = C.c_uint64(0), C.c_uint64(0)
            rc = lib.groot_hip_ec_export(h, _ffi.as_ptr(o, C.c_uint64), _ffi.as_ptr(i, C.c_uint32), _ffi.as_ptr(c, C.c_uint64), C.c_uint64(cap_ec), C.c_uint64(cap_ids),
                                         C.byref(me), C.byref(mi))
            assert rc == -6 and (me.value, mi.value) == (ne, ni)
            assert np.all(o == GUARD64) and np.all(i == GUARD32) and np.all(c == GUARD64)
        # with exactly enough room: the arrays, and nothing behind them
        o = np.full(ne + 2, GUARD64, dtype=np.uint64)
        i = np.full(ni + 1, GUARD32, dtype=np.uint32)
        c = np.full(ne + 1, GUARD64, dtype=np.uint64)
        me, mi = C.c_uint64(0), C.c_uint64(0)
        rc = lib.groot_hip_ec_export(h, _ffi.as_ptr(o, C.c_uint64), _ffi.as_ptr(i, C.c_uint32), _ffi.as_ptr(c, C.c_uint64), C.c_uint64(ne), C.c_uint64(ni), C.byref(me), C.byref(mi))
        assert rc == 0 and np.array_equal(o[:ne + 1], off) and np.array_equal(i[:ni], ids) and np.array_equal(c[:ne], ec_cnt)
        assert o[ne + 1] == GUARD64 and i[ni] == GUARD32 and c[ne] == GUARD64
    finally:
        al.close()
