"""The default first pass of the align stage, align_path_kernel (kernels_path.hpp: walks compared against path text), against the CPU
oracle, against align_kernel alone (GROOT_NO_PATH_PASS=1) and against the node-by-node first pass (GROOT_LEAN=1): every record, path set,
call count and counter must be the same, and the pass must finish reads itself rather than leave them all to align_kernel."""
import os

import numpy as np
import pytest

import oracle_check
from conftest import DATA, read_fastq
from groot_amd import device, synth

pytestmark = pytest.mark.gpu

MODES = {"path": {}, "no_path": {"GROOT_NO_PATH_PASS": "1"}, "lean": {"GROOT_LEAN": "1"}}
DIAG = ("lean_reads",)          # which first pass finished a read: differs by design


@pytest.fixture(scope="module", autouse=True)
def need_gpu(hip_lib):
    assert device.device_count() > 0, "no MI355X visible: the HIP path has no CPU fallback"


def _pack(reads):
    seqs = [r[1] for r in reads]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), off


def _set_mode(monkeypatch, mode):
    for v in ("GROOT_NO_PATH_PASS", "GROOT_LEAN", "GROOT_NO_SIG"):
        monkeypatch.delenv(v, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def _run(monkeypatch, mode, index, seq, off, threshold=0.99, max_read_len=256):
    _set_mode(monkeypatch, mode)
    al = device.Aligner(index, threshold=threshold, max_batch_reads=max(1024, len(off) - 1), max_read_len=max_read_len, memo_budget_mb=device.MEMO_OFF)
    try:
        al.submit(seq, off)
        c = al.wait()
        t, m = al.travs()
        return c, t, m, al.attempts().copy(), al.path_pass_stats(), oracle_check.device_results(al, index)
    finally:
        al.close()


def _same(a, b):
    (ca, ta, ma, atta, *_), (cb, tb, mb, attb, *_) = a, b
    assert {k: v for k, v in ca.items() if k not in DIAG} == {k: v for k, v in cb.items() if k not in DIAG}
    assert np.array_equal(ta, tb) and np.array_equal(ma, mb) and np.array_equal(atta, attb)


def _three(monkeypatch, index, seq, off, threshold=0.99, max_read_len=256):
    """the shipped stage against the oracle, then the two other stages against the shipped one"""
    p = _run(monkeypatch, "path", index, seq, off, threshold, max_read_len)
    oracle_check.assert_same(p[0], p[5], oracle_check.oracle_run(index, seq, off, threshold), "path pass vs oracle")
    _same(p, _run(monkeypatch, "no_path", index, seq, off, threshold, max_read_len))
    _same(p, _run(monkeypatch, "lean", index, seq, off, threshold, max_read_len))
    assert p[0]["lean_reads"] == 0
    return p[:5]


def _with_errors(seq, rate, seed, n_rate=0.0):
    rng = np.random.default_rng(seed)
    out = seq.copy()
    hit = rng.random(len(out)) < rate
    out[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    if n_rate:
        out[rng.random(len(out)) < n_rate] = ord("N")
    return out


@pytest.mark.parametrize("fq", ["full-argannot-perfect-reads-small.fq.gz", "full-argannot-perfect-reads-small-variable-rl.fq.gz",
                                "test-reads-OXA90-OXA106-100bp-with-errors.fastq.gz", "argannot-150bp-10000-reads.fq.gz"])
def test_golden_reads_agree(argannot_index, monkeypatch, fq):
    seq, off = _pack(read_fastq(os.path.join(DATA, fq)))
    c, t, m, att, st = _three(monkeypatch, argannot_index, seq, off)
    assert st["ran"] and st["reads"] <= c["walked_reads"] and (st["reads"] > 0 or c["walked_reads"] == 0), (st, c)


# share of the walked reads the pass must finish (short reads bring more than four seed windows more often: those are left to align_kernel)
_SYN_FINISH = {"exact": 0.9, "sub1": 0.9, "sub3_n": 0.85, "len90": 0.5, "len60": 0.3}


@pytest.mark.parametrize("case", sorted(_SYN_FINISH))
def test_synthetic_reads_agree(argannot_index, monkeypatch, case):
    """both strands (synth draws them), substitutions (jumps between paths, mismatches at node starts), read bytes 'N' (left to
    align_kernel), shorter reads (more seed windows), short reads (levels 3 / 4 clip a base of the few windows they have)"""
    cat, o, lens = synth.reference_sequences(argannot_index)
    L = {"len90": 90, "len60": 60}.get(case, 100)
    seq, off, _ = synth.reads_np(cat, o, lens, 200_000, L, seed=1234)
    if case == "sub1":
        seq = _with_errors(seq, 0.01, 7)
    elif case == "sub3_n":
        seq = _with_errors(seq, 0.03, 8, n_rate=0.0005)
    c, t, m, att, st = _three(monkeypatch, argannot_index, seq, off)
    print("case %s: %s %s" % (case, st, {k: c[k] for k in ("walked_reads", "mapped", "travs")}))
    assert c["walked_reads"] > 0.1 * (len(off) - 1), c
    assert st["ran"] and _SYN_FINISH[case] * c["walked_reads"] <= st["reads"] <= c["walked_reads"], (st, c)


def test_variation_graph_agrees(testgfa_index, monkeypatch):
    """test.gfa: a small graph of bubbles -- boundaries where two neighbours share a first base, sinks, reads ending in overhangs"""
    cat, o, lens = synth.reference_sequences(testgfa_index)
    for L, rate in ((25, 0.0), (28, 0.0), (28, 0.02)):
        seq, off, _ = synth.reads_np(cat, o, lens, 20_000, L, seed=99 + L)
        if rate:
            seq = _with_errors(seq, rate, L)
        c, t, m, att, st = _three(monkeypatch, testgfa_index, seq, off, threshold=0.9)
        print("test.gfa %d %.2f: %s %s" % (L, rate, st, {k: c[k] for k in ("walked_reads", "mapped", "travs")}))
        assert c["walked_reads"] > 0.1 * 20_000, c
        assert st["ran"] and 0.5 * c["walked_reads"] <= st["reads"] <= c["walked_reads"], (st, c)


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("workload", ["c2", "sub1", "mixed90"])
def test_at_benchmark_size(argannot_index, resfinder_index, monkeypatch, workload):
    """the three align stages on the batches bench.py times: 10 M error-free 100 bp reads of arg-annot.90 (configs[2]), the same with 1 %
    substitutions, 8 M reads of 75..150 bases of resfinder.90 at t = 0.90"""
    import torch

    mixed = workload == "mixed90"
    threshold = 0.90 if mixed else 0.99
    index = resfinder_index if mixed else argannot_index
    dev = torch.device("cuda", 0)
    cat, o, lens = synth.reference_sequences(index)
    cat_t, off_t, lens_t = (torch.from_numpy(x).to(dev) for x in (cat, o, lens))
    if mixed:
        R = 8_000_000
        d_seq, d_off, _ = synth.reads_torch_mixed(cat_t, off_t, lens_t, R, 150, 75)
        max_len, total = 150, int(d_off[-1].item())
    else:
        R, L = 10_000_000, 100
        parts = []
        for c0 in range(0, R, 1_000_000):
            p, _, _ = synth.reads_torch(cat_t, off_t, lens_t, 1_000_000, L, first=c0)
            parts.append(p[: 1_000_000 * L])
        d_seq = torch.zeros(R * L + 64, dtype=torch.uint8, device=dev)
        d_seq[: R * L] = torch.cat(parts)
        del parts
        d_off = torch.arange(0, R + 1, dtype=torch.int64, device=dev) * L
        max_len, total = L, R * L
        if workload == "sub1":
            g = torch.Generator(device=dev)
            g.manual_seed(0x70617468)
            rows = d_seq[: R * L].view(R, L)
            acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
            for c0 in range(0, R, 1_000_000):
                blk = rows[c0:c0 + 1_000_000]
                hit = torch.rand(blk.shape, generator=g, device=dev) < 0.01
                rows[c0:c0 + 1_000_000] = torch.where(hit, acgt[torch.randint(0, 4, blk.shape, generator=g, device=dev)], blk)
    torch.cuda.synchronize()

    def run(mode):
        _set_mode(monkeypatch, mode)
        al = device.Aligner(index, threshold=threshold, max_batch_reads=R, max_read_len=256, max_batch_bases=total + 64, memo_budget_mb=device.MEMO_OFF)
        try:
            al.set_profiling(True)
            al.attempts_reset()
            al.submit_device(d_seq.data_ptr(), d_off.data_ptr(), R, first_read_id=0, max_len=max_len, mixed=mixed)
            c = al.wait()
            t, m = al.travs()
            return c, t, m, al.attempts().copy(), al.path_pass_stats()
        finally:
            al.close()

    p = run("path")
    _same(p, run("no_path"))
    _same(p, run("lean"))
    c, st = p[0], p[4]
    assert c["lean_reads"] == 0
    if workload == "c2":
        assert st["ran"] and st["reads"] > 0.9 * c["walked_reads"], (st, c)


# ---- small graphs built for one case each ------------------------------------------------------------------------------------
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _gfa(path, nodes, edges, paths):
    """nodes: {id: sequence}; edges: [(a, b)]; paths: [(name, [ids])] -- one GFA file, path ids in the order given"""
    lines = ["H\tVN:Z:1"] + ["S\t%d\t%s\tLN:i:%d" % (i, s, len(s)) for i, s in sorted(nodes.items())]
    lines += ["L\t%d\t+\t%d\t+\t0M" % e for e in edges]
    lines += ["P\t%s\t%s" % (n, ",".join("%d+" % i for i in ids)) for n, ids in paths]
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def _seq(rng, n, avoid_first=()):
    while True:
        s = "".join(rng.choice(list("ACGT"), n))
        if s[0] not in avoid_first:
            return s


def _reads(rng, nodes, paths, n, L, clip=False, overhang=0):
    """reads drawn from the paths' texts, both strands; a graph 'N' becomes a random base (the DFS counts it as a match); clip: a third of
    the reads get their first base changed, a third their last (levels 3 / 4); overhang: reads that run this many bases past a path's end"""
    return _reads_from(rng, ["".join(nodes[i] for i in ids) for _, ids in paths], n, L, clip, overhang)


def _reads_from(rng, texts, n, L, clip=False, overhang=0, starts=None):
    """_reads on the given texts; starts: per text, the start positions to draw from (default: all)"""
    out = []
    for j in range(n):
        t = texts[j % len(texts)]
        if overhang:
            r = t[len(t) - (L - overhang):] + "".join(rng.choice(list("ACGT"), overhang))
        else:
            s0 = int(rng.choice(starts[j % len(texts)])) if starts else int(rng.integers(0, len(t) - L + 1))
            r = t[s0:s0 + L]
        r = "".join(ch if ch != "N" else "ACGT"[int(rng.integers(0, 4))] for ch in r)
        if clip and j % 3:
            p = 0 if j % 3 == 1 else L - 1
            r = r[:p] + "ACGT"["ACGT".index(r[p]) ^ 1] + r[p + 1:]
        rb = r.encode()
        if j & 1:
            rb = rb.translate(_COMP)[::-1]
        out.append((b"r%d" % j, rb, b"I" * L))
    return _pack(out)


def _bubbles(rng, n_bub, alleles, seg=24):
    """a backbone of `n_bub + 1` segments with a bubble between two: alleles(i) -> list of allele sequences; paths take allele choices"""
    nodes, edges, nid = {}, [], 1
    back = []
    for i in range(n_bub + 1):
        nodes[nid] = _seq(rng, seg)
        back.append(nid)
        nid += 1
    bub = []
    for i in range(n_bub):
        ids = []
        for a in alleles(i):
            nodes[nid] = a
            edges += [(back[i], nid), (nid, back[i + 1])]
            ids.append(nid)
            nid += 1
        bub.append(ids)
    return nodes, edges, back, bub


def _index(tmp_path, files):
    from groot_amd import host

    return host.Index.from_gfa_files(files, host.index_params(k=7, s=10, w=30))


def _case_graph(tmp_path, case, rng):
    L = 28
    if case == "jumps":
        # SNP bubbles, first bases distinct (no flagged boundary); three paths with different alleles: reads of paths 1, 2 start on nodes whose
        # lowest path is 0 and jump at every allele where they differ; reads end on the sinks of the paths
        nodes, edges, back, bub = _bubbles(rng, 6, lambda i: ["A", "C", "G"])
        paths = [("p%d" % p, [x for i in range(6) for x in (back[i], bub[i][(p * (i + 1)) % 3])] + [back[6]]) for p in range(3)]
        files = [_gfa(tmp_path / "g.gfa", nodes, edges, paths)]
        return files, [_reads(rng, nodes, paths, 6000, L), _reads(rng, nodes, paths, 3000, L, clip=True)]
    if case == "ambiguous":
        # alleles with the same first base (flagged boundaries: the neighbour loop decides, often the path's own next node) and pairs of
        # identical alleles (two records per walk: the second neighbour goes on the read's stack)
        nodes, edges, back, bub = _bubbles(rng, 5, lambda i: ["AC", "AG"] if i % 2 else ["TTA", "TTA"])
        paths = [("p%d" % p, [x for i in range(5) for x in (back[i], bub[i][(p + i) % 2])] + [back[5]]) for p in range(2)]
        files = [_gfa(tmp_path / "g.gfa", nodes, edges, paths)]
        return files, [_reads(rng, nodes, paths, 6000, L)]
    if case == "bypass":
        # a deletion: B1 -> B3 beside B1 -> B2 -> B3 (path 1 skips B2), and an insertion bubble
        nodes = {1: _seq(rng, 30), 2: _seq(rng, 12, avoid_first="A"), 3: "A" + _seq(rng, 29), 4: _seq(rng, 30)}
        edges = [(1, 2), (2, 3), (1, 3), (3, 4)]
        paths = [("full", [1, 2, 3, 4]), ("del", [1, 3, 4])]
        files = [_gfa(tmp_path / "g.gfa", nodes, edges, paths)]
        return files, [_reads(rng, nodes, paths, 6000, L)]
    if case == "ends":
        # path 0 ends at node 3, which is not a sink (its text ends: the neighbour loop takes node 4 and its own path); path 1 ends at the sink
        # 4; reads that run past the sink (an overhang is reported there), reads that end exactly on it
        nodes = {1: _seq(rng, 30), 2: _seq(rng, 20), 3: _seq(rng, 20), 4: _seq(rng, 30)}
        edges = [(1, 2), (2, 3), (3, 4)]
        paths = [("short", [1, 2, 3]), ("long", [1, 2, 3, 4])]
        files = [_gfa(tmp_path / "g.gfa", nodes, edges, paths)]
        return files, [_reads(rng, nodes, paths[1:], 3000, L, overhang=3) + (0.75,), _reads(rng, nodes, paths, 6000, L)]
    if case == "graph_n":
        # an 'N' inside a node and an allele that starts with 'N' (a neighbour whose first base is 'N': that boundary is flagged)
        nodes, edges, back, bub = _bubbles(rng, 4, lambda i: ["C", "N"] if i == 2 else ["A", "G"])
        nodes[back[1]] = nodes[back[1]][:10] + "N" + nodes[back[1]][11:]
        paths = [("p%d" % p, [x for i in range(4) for x in (back[i], bub[i][(p + i) % 2])] + [back[4]]) for p in range(2)]
        files = [_gfa(tmp_path / "g.gfa", nodes, edges, paths)]
        return files, [_reads(rng, nodes, paths, 6000, L)]
    if case == "many_records":
        # two consecutive pairs of identical alleles = four records per walk, in two identical graphs: reads of up to five records finish in
        # the pass (four held until the end), more are left to align_kernel
        nodes, edges, back, bub = _bubbles(rng, 2, lambda i: ["GCA", "GCA"], seg=14)
        paths = [("p0", [back[0], bub[0][0], back[1], bub[1][0], back[2]]), ("p1", [back[0], bub[0][1], back[1], bub[1][1], back[2]])]
        files = [_gfa(tmp_path / "g1.gfa", nodes, edges, paths), _gfa(tmp_path / "g2.gfa", nodes, edges, paths)]
        return files, [_reads(rng, nodes, paths, 4000, L)]
    if case == "fanout":
        # b0 has five out-neighbours and b1 six (more than a node record holds: flagged, the walk is left to align_kernel there); b2 has four
        # whose first bases all differ (unflagged: the read's next base decides, the pass finishes those walks); six paths take every allele
        nodes, edges, back, bub = _bubbles(rng, 3, lambda i: ["ACGTAC"[a] + _seq(rng, 4) for a in range((5, 6, 4)[i])], seg=40)
        paths = [("p%d" % p, [back[0], bub[0][p % 5], back[1], bub[1][p % 6], back[2], bub[2][p % 4], back[3]]) for p in range(6)]
        files = [_gfa(tmp_path / "g.gfa", nodes, edges, paths)]
        deg4 = [("x", [back[2], a, back[3]]) for a in bub[2]]
        return files, [_reads(rng, nodes, paths, 6000, L) + (0.9, {"defer": True}), _reads(rng, nodes, deg4, 3000, L) + (0.9, {"finish": 0.75})]
    if case == "no_text":
        # path 0 goes 1 -> 3 with no L edge between them: it has no text.  Nodes 1, 3, 4 and 7 have it as their lowest path and take the
        # text of path 1; node 5 lies on path 0 alone (no path with a text: a walk that starts on it or jumps to it is left to align_kernel)
        nodes = {1: _seq(rng, 30), 2: _seq(rng, 12), 3: _seq(rng, 30), 4: _seq(rng, 30), 5: "A" + _seq(rng, 11), 6: "C" + _seq(rng, 11),
                 7: _seq(rng, 30)}
        edges = [(1, 2), (2, 3), (3, 4), (4, 5), (4, 6), (5, 7), (6, 7)]
        paths = [("gap", [1, 3, 4, 5, 7]), ("full", [1, 2, 3, 4, 6, 7])]
        files = [_gfa(tmp_path / "g.gfa", nodes, edges, paths)]
        via5 = [("x", [4, 5, 7])]
        return files, [_reads(rng, nodes, paths, 6000, L) + (0.9, {"defer": True, "finish": 0.4, "mapped": 0.2}),
                       _reads(rng, nodes, via5, 3000, L) + (0.9, {"defer": True, "finish": 0.0})]
    if case == "stack":
        # pairs of identical alleles ("GCA" twice), each on another path: bubbles 0-2 lie within 19 bases (a read over all three has two
        # neighbours pending at the third: left to align_kernel), bubbles 3-4 within 12 (two pending at most: finished in the pass, the
        # pending neighbour resumes in the other path's text)
        segs = [30, 5, 5, 40, 6, 30]
        nodes, edges, back, bub = {}, [], [], []
        nid = 1
        for n in segs:
            nodes[nid] = _seq(rng, n); back.append(nid); nid += 1
        for i in range(5):
            ids = []
            for a in range(2):
                nodes[nid] = "GCA"; edges += [(back[i], nid), (nid, back[i + 1])]; ids.append(nid); nid += 1
            bub.append(ids)
        paths = [("p%d" % p, [x for i in range(5) for x in (back[i], bub[i][(p + i) % 2])] + [back[5]]) for p in range(2)]
        files = [_gfa(tmp_path / "g.gfa", nodes, edges, paths)]
        three = nodes[back[0]][-8:] + "GCA" + nodes[back[1]] + "GCA" + nodes[back[2]] + "GCA" + nodes[back[3]][:8]
        two = nodes[back[3]][-14:] + "GCA" + nodes[back[4]] + "GCA" + nodes[back[5]][:14]
        return files, [_reads(rng, nodes, paths, 6000, L) + (0.9, {"defer": True, "finish": 0.5}),
                       _reads_from(rng, [three], 3000, L) + (0.9, {"defer": True, "finish": 0.0, "finish_max": 0.2}),
                       _reads_from(rng, [two], 3000, L) + (0.9, {"finish": 0.9, "travs": (2.0, 4.0)})]
    if case == "hold":
        # a chain x1..x8 of 6-base nodes behind a 40-base head: behind every xi a one-base sink "A" (segment id 100 + i: first in the
        # OutEdges order, so the walk takes it first and the stack never holds more than one) beside x(i+1), which starts with 'A' as well.
        # Every boundary a read crosses adds one record (the sink reports its overhang): 28-base reads cross four or five of them, five
        # records (four held) finish in the pass, six are left to align_kernel (kPathHold = 4)
        nodes = {1: _seq(rng, 40)}
        for i in range(2, 10):
            nodes[i] = "A" + _seq(rng, 5)
        nodes[10] = "A" + _seq(rng, 39)
        edges = [(i, i + 1) for i in range(1, 10)] + [(i, 100 + i) for i in range(2, 10)]
        paths = [("main", list(range(1, 11)))]
        for i in range(2, 10):
            nodes[100 + i] = "A"
            paths.append(("stub%d" % i, list(range(1, i + 1)) + [100 + i]))
        files = [_gfa(tmp_path / "g.gfa", nodes, edges, paths)]
        text = "".join(nodes[i] for i in range(1, 11))
        bounds = [40 + 6 * k for k in range(1, 9)]                    # starts of x3..x9 and of the tail: each has a sink beside it
        def crossing(m):
            return [q for q in range(34, len(text) - L + 1) if sum(q < b <= q + L - 1 for b in bounds) == m]
        return files, [_reads_from(rng, [text], 3000, L, starts=[crossing(4)]) + (0.9, {"finish": 0.7, "most_travs": 5}),
                       _reads_from(rng, [text], 3000, L, starts=[crossing(5)]) + (0.9, {"defer": True, "finish": 0.0, "most_travs": 6})]
    if case == "wide_paths":
        # graphs of 64, 65, 128, 129 and 192 paths (three path words): the paths from `cut` on take a region of their own (bubbles of three
        # alleles, chosen at random), the others one node; reads from that region have path sets in word 0's top bit, word 1 or word 2 alone
        files, texts = [], []
        for n_paths, cut in ((64, 63), (65, 64), (128, 64), (129, 128), (192, 128)):
            f, t = _wide(rng, tmp_path / ("w%d.gfa" % n_paths), n_paths, cut)
            files.append(f); texts += t
        return files, [_reads_from(rng, texts, 8000, L) + (0.9, {"finish": 0.5, "path_words": 3}),
                       _reads_from(rng, texts, 8000, L, clip=True) + (0.9, {"finish": 0.3, "path_words": 3})]
    if case == "n_first":
        # path 0's first node starts with 'N' (the text cannot mark a node's first base as 'N'; the seed windows holding it are left at
        # staging); path 1 starts on a node of its own
        nodes = {1: "N" + _seq(rng, 29), 2: _seq(rng, 30), 3: _seq(rng, 20), 4: _seq(rng, 30)}
        edges = [(1, 2), (3, 2), (2, 4)]
        paths = [("n", [1, 2, 4]), ("other", [3, 2, 4])]
        files = [_gfa(tmp_path / "g.gfa", nodes, edges, paths)]
        texts = ["".join(nodes[i] for i in ids) for _, ids in paths]
        return files, [_reads(rng, nodes, paths, 6000, L) + (0.9, {"finish": 0.5}),
                       _reads_from(rng, texts[:1], 3000, L, starts=[[0, 1, 2, 3]]) + (0.9, {"finish": 0.0, "walked": 0.0, "mapped": 0.0})]
    raise ValueError(case)


def _wide(rng, path, n_paths, cut, n_bub=5):
    """head -> (paths < cut) one node | (paths >= cut) a chain of bubbles of three alleles -> tail; the high region's texts, per path"""
    nodes = {1: _seq(rng, 30), 2: _seq(rng, 40), 3: _seq(rng, 30)}
    edges = [(1, 2), (2, 3)]
    back, bub, nid = [], [], 10
    for i in range(n_bub + 1):
        nodes[nid] = _seq(rng, 8); back.append(nid); nid += 1
    edges += [(1, back[0]), (back[-1], 3)]
    for i in range(n_bub):
        ids = []
        for a, ch in enumerate("ACG"):
            nodes[nid] = ch + (_seq(rng, a) if a else ""); edges += [(back[i], nid), (nid, back[i + 1])]; ids.append(nid); nid += 1
        bub.append(ids)
    paths, texts = [], []
    for p in range(n_paths):
        if p < cut:
            paths.append(("p%d" % p, [1, 2, 3]))
            continue
        pick = [bub[i][(p - cut) % 3 if p - cut < 3 else int(rng.integers(0, 3))] for i in range(n_bub)]
        hi = [x for i in range(n_bub) for x in (back[i], pick[i])] + [back[-1]]
        paths.append(("p%d" % p, [1] + hi + [3]))
        texts.append("".join(nodes[i] for i in hi))
    used = {x for _, ids in paths for x in ids}
    nodes = {k: v for k, v in nodes.items() if k in used}
    edges = [e for e in edges if e[0] in used and e[1] in used]
    return _gfa(path, nodes, edges, paths), texts


def _fuzz_graph(rng, path, n_paths):
    """a random DAG: backbone nodes of 1..40 bases; between two, a bubble (2-3 alleles), a deletion (an allele or the edge past it) or an
    insertion (an extra node or none); every path picks an option per site; a few graph 'N's"""
    nodes, edges, opts, nid = {}, [], [], 1
    n_sites = int(rng.integers(6, 12))
    back = []
    for i in range(n_sites + 1):
        nodes[nid] = _seq(rng, int(rng.integers(30 if i == n_sites else 1, 41))); back.append(nid); nid += 1   # (a path spans a window)
    for i in range(n_sites):
        kind = int(rng.integers(0, 3))
        o = []
        for a in range(3 if kind == 0 and rng.random() < 0.5 else 2):
            if kind and a == 1:
                edges.append((back[i], back[i + 1])); o.append(None)
                continue
            nodes[nid] = _seq(rng, int(rng.integers(1, 41))); edges += [(back[i], nid), (nid, back[i + 1])]; o.append(nid); nid += 1
        opts.append(o)
    for _ in range(int(rng.integers(0, 4))):                        # graph 'N's, now and then on a node's first base
        n = int(rng.integers(1, nid))
        j = 0 if rng.random() < 0.3 else int(rng.integers(0, len(nodes[n])))
        nodes[n] = nodes[n][:j] + "N" + nodes[n][j + 1:]
    paths = []
    for p in range(n_paths):
        ids = []
        for i in range(n_sites):
            ids.append(back[i])
            o = opts[i][p % len(opts[i]) if p < 3 else int(rng.integers(0, len(opts[i])))]
            if o is not None:
                ids.append(o)
        ids.append(back[-1])
        paths.append(("p%d" % p, ids))
    used = {x for _, ids in paths for x in ids}
    nodes = {k: v for k, v in nodes.items() if k in used}
    edges = [e for e in edges if e[0] in used and e[1] in used]
    return _gfa(path, nodes, edges, paths), nodes, paths


# share of the walked reads the pass must finish per case (what it leaves: more than four windows, a read that needs the graph 'N', ...)
# (graph_n: reads whose seed windows hold an 'N' are left at staging, as by the node walk; many_records: reads of more than five records)
_FINISH = {"jumps": 0.8, "ambiguous": 0.8, "bypass": 0.8, "ends": 0.8, "graph_n": 0.25, "many_records": 0.5,
           "fanout": 0.3, "no_text": 0.4, "stack": 0.5, "hold": 0.9, "wide_paths": 0.5, "n_first": 0.5}


@pytest.mark.parametrize("case", sorted(_FINISH))
def test_built_graph_cases(tmp_path, monkeypatch, case):
    """small graphs (k=7 s=10 w=30) built for one branch of the pass each, against the oracle and the other two stages; opts per batch:
    finish / finish_max: bounds on the share of walked reads the pass finishes, defer: some reads are left to align_kernel, travs: bounds
    on the records per mapped read, most_travs: the most records of one read, walked / mapped: least shares of the batch"""
    rng = np.random.default_rng(sum(map(ord, case)))
    files, batches = _case_graph(tmp_path, case, rng)
    index = _index(tmp_path, files)
    for seq, off, *more in batches:
        thr, opts = (more[0] if more else 0.9), (more[1] if len(more) > 1 else {})
        c, t, m, att, st = _three(monkeypatch, index, seq, off, threshold=thr)
        n = len(off) - 1
        print("case %s: %s %s finish share %.3f" % (case, st, {k: c[k] for k in ("walked_reads", "mapped", "travs", "alignments")},
                                                     st["reads"] / max(1, c["walked_reads"])))
        assert c["walked_reads"] > opts.get("walked", 0.3) * n and c["mapped"] > opts.get("mapped", 0.3) * n, (case, c)
        if case in ("ambiguous", "many_records"):
            assert c["travs"] > 1.2 * c["mapped"], (case, c)      # walks with more than one record
        lo, hi = opts.get("finish", _FINISH[case]), opts.get("finish_max", 1.0)
        assert st["ran"] and lo * c["walked_reads"] <= st["reads"] <= min(hi * c["walked_reads"], c["walked_reads"]), (case, st, c)
        if case == "many_records" or opts.get("defer"):
            assert st["reads"] < c["walked_reads"], (case, st, c)    # some reads are left to align_kernel
        if "travs" in opts:
            assert opts["travs"][0] * c["mapped"] <= c["travs"] <= opts["travs"][1] * c["mapped"], (case, c)
        if "most_travs" in opts:                                    # the most records a read of the batch has
            assert np.bincount(t["read_id"]).max() == opts["most_travs"], (case, np.bincount(np.bincount(t["read_id"])))
        if "path_words" in opts:
            assert index.view.path_words == opts["path_words"]


@pytest.mark.parametrize("seed", [3, 17, 101, 2024, 65537])
def test_fuzz_graphs(tmp_path, monkeypatch, seed):
    """random DAGs (bubbles, deletions, insertions; nodes of 1..40 bases, so texts start at every offset mod 16 and segments cross the
    32-base pieces of path_segment; 1..192 paths; a few graph 'N's): exact reads, reads with 1 % and 3 % substitutions, reads with their
    first or last base changed"""
    rng = np.random.default_rng(seed)
    files, texts = [], []
    for g, n_paths in enumerate((1 + seed % 5, int(rng.integers(6, 129)), int(rng.integers(129, 193)))):
        f, nodes, paths = _fuzz_graph(rng, tmp_path / ("f%d.gfa" % g), n_paths)
        files.append(f)
        texts += ["".join(nodes[i] for i in ids) for _, ids in paths]
    index = _index(tmp_path, files)
    assert index.view.path_words == 3
    for L, rate, clip in ((28, 0.0, False), (32, 0.0, False), (28, 0.01, False), (28, 0.03, False), (28, 0.0, True)):
        seq, off = _reads_from(rng, [t for t in texts if len(t) >= L], 6000, L, clip=clip)
        if rate:
            seq = _with_errors(seq, rate, seed + int(rate * 100))
        c, t, m, att, st = _three(monkeypatch, index, seq, off, threshold=0.9)
        print("fuzz %d L%d %.2f%s: %s %s finish share %.3f" % (seed, L, rate, " clip" if clip else "", st,
              {k: c[k] for k in ("walked_reads", "mapped", "travs", "alignments")}, st["reads"] / max(1, c["walked_reads"])))
        assert c["walked_reads"] > 0.2 * (len(off) - 1), c
        assert st["ran"] and 0.2 * c["walked_reads"] <= st["reads"] <= c["walked_reads"], (st, c)


def test_wide_path_limit(tmp_path, monkeypatch):
    """a graph of 193 paths (four path words): no first pass at all, the same results"""
    rng = np.random.default_rng(193)
    f, texts = _wide(rng, tmp_path / "w193.gfa", 193, 128)
    index = _index(tmp_path, [f])
    assert index.view.path_words == 4
    seq, off = _reads_from(rng, texts, 6000, 28)
    c, t, m, att, st = _three(monkeypatch, index, seq, off, threshold=0.9)
    assert c["mapped"] > 0.3 * (len(off) - 1), c
    assert not st["ran"] and st["reads"] == 0, st


# ---- reads of 129..256 bases: the NCH = 5 and NCH = 8 instantiations of both first passes --------------------------------------------
@pytest.fixture(scope="module")
def w256_index(msa_dir):
    """k31 s21 w256 over the first 60 clusters of arg-annot.90: reads longer than the default window of 100 seed here"""
    from groot_amd import host

    names = sorted((n for n in os.listdir(msa_dir) if n.startswith("cluster") and n.endswith(".msa")), key=lambda n: int(n[8:-4]))[:60]
    return host.Index.from_msa_files([os.path.join(msa_dir, n) for n in names], host.index_params(k=31, s=21, w=256))


@pytest.mark.parametrize("threshold", [0.99, 0.90])
@pytest.mark.parametrize("batch", ["128", "129", "160", "161", "200", "256", "mixed129_256", "sub1_200", "257"])
def test_long_read_variants(w256_index, monkeypatch, threshold, batch):
    cat, o, lens = synth.reference_sequences(w256_index)
    if batch == "mixed129_256":
        seq, off, _ = synth.reads_np(cat, o, lens, 20_000, 256, seed=129, min_len=129)
        L = int(np.max(np.diff(off)))
    else:
        L = int(batch.split("_")[-1])
        seq, off, _ = synth.reads_np(cat, o, lens, 20_000, L, seed=L)
        if batch.startswith("sub1"):
            seq = _with_errors(seq, 0.01, L)
    c, t, m, att, st = _three(monkeypatch, w256_index, seq, off, threshold=threshold, max_read_len=512)
    print("w256 %s t%.2f: %s %s finish share %.3f" % (batch, threshold, st, {k: c[k] for k in ("walked_reads", "mapped", "travs")},
                                                      st["reads"] / max(1, c["walked_reads"])))
    assert c["walked_reads"] > 0.05 * (len(off) - 1) and c["mapped"] > 0, c
    if L > 256:
        assert not st["ran"] and st["reads"] == 0, st                 # longer than kLeanMaxLen: align_kernel alone
    else:
        assert st["ran"] and 0 < st["reads"] <= c["walked_reads"], (st, c)
