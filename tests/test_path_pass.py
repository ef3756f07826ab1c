"""The default first pass of the align stage, align_path_kernel (kernels_path.hpp: walks compared against path text), against align_kernel
alone (GROOT_NO_PATH_PASS=1) and against the node-by-node first pass (GROOT_LEAN=1): every record, path set, call count and counter must
be the same, and the pass must finish reads itself rather than leave them all to align_kernel."""
import os

import numpy as np
import pytest

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


def _run(monkeypatch, mode, index, seq, off, threshold=0.99):
    _set_mode(monkeypatch, mode)
    al = device.Aligner(index, threshold=threshold, max_batch_reads=max(1024, len(off) - 1), memo_budget_mb=device.MEMO_OFF)
    try:
        al.submit(seq, off)
        c = al.wait()
        t, m = al.travs()
        return c, t, m, al.attempts().copy(), al.path_pass_stats()
    finally:
        al.close()


def _same(a, b):
    (ca, ta, ma, atta, _), (cb, tb, mb, attb, _) = a, b
    assert {k: v for k, v in ca.items() if k not in DIAG} == {k: v for k, v in cb.items() if k not in DIAG}
    assert np.array_equal(ta, tb) and np.array_equal(ma, mb) and np.array_equal(atta, attb)


def _three(monkeypatch, index, seq, off, threshold=0.99):
    p = _run(monkeypatch, "path", index, seq, off, threshold)
    _same(p, _run(monkeypatch, "no_path", index, seq, off, threshold))
    _same(p, _run(monkeypatch, "lean", index, seq, off, threshold))
    assert p[0]["lean_reads"] == 0
    return p


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
    texts = ["".join(nodes[i] for i in ids) for _, ids in paths]
    out = []
    for j in range(n):
        t = texts[j % len(texts)]
        if overhang:
            r = t[len(t) - (L - overhang):] + "".join(rng.choice(list("ACGT"), overhang))
        else:
            s0 = int(rng.integers(0, len(t) - L + 1))
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
    raise ValueError(case)


# share of the walked reads the pass must finish per case (what it leaves: more than four windows, a read that needs the graph 'N', ...)
# (graph_n: reads whose seed windows hold an 'N' are left at staging, as by the node walk; many_records: reads of more than five records)
_FINISH = {"jumps": 0.8, "ambiguous": 0.8, "bypass": 0.8, "ends": 0.8, "graph_n": 0.25, "many_records": 0.5}


@pytest.mark.parametrize("case", sorted(_FINISH))
def test_built_graph_cases(tmp_path, monkeypatch, case):
    rng = np.random.default_rng(sum(map(ord, case)))
    files, batches = _case_graph(tmp_path, case, rng)
    index = _index(tmp_path, files)
    for seq, off, *thr in batches:
        c, t, m, att, st = _three(monkeypatch, index, seq, off, threshold=thr[0] if thr else 0.9)
        n = len(off) - 1
        print("case %s: %s %s" % (case, st, {k: c[k] for k in ("walked_reads", "mapped", "travs", "alignments")}))
        assert c["walked_reads"] > 0.3 * n and c["mapped"] > 0.3 * n, (case, c)
        if case in ("ambiguous", "many_records"):
            assert c["travs"] > 1.2 * c["mapped"], (case, c)      # walks with more than one record
        assert st["ran"] and _FINISH[case] * c["walked_reads"] <= st["reads"] <= c["walked_reads"], (case, st, c)
        if case == "many_records":
            assert st["reads"] < c["walked_reads"], (case, st, c)    # some reads hold too many records and are left to align_kernel
