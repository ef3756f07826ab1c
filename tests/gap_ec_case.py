"""The index and the reads of the tests of the gap-placed reads in the equivalence classes (tests/test_gap_ec_def.py on the CPU,
tests/test_gap_ec.py and tests/test_abundance_gapped_cli.py on the device): small enough for the brute force of tests/gap_def.py, with every
input class the definition (include/groot_hip.h, "gap-placed reads in the equivalence classes") tells apart.

Eleven graphs, 88 paths:
    graphs 0-2   the three of tests/gap_case.py (gaps of both types, a tandem repeat, the "ungapped with two substitutions, gapped with
                 none" tail), seven paths, all sets in one graph
    graphs 3-8   two or three paths each around 120-base segments they share verbatim:  S6 in all six, S3 in graphs 3, 4, 5 (which hold it
                 behind S6), S2 in graph 6 -- and in graph 10
    graph 9      one path with a 100-base stretch twice (kept placements at two x of one path)
    graph 10     S2 . a fan of 66 alleles . a short tail: a set with bits in two mask words of one graph
The reads are gap_case's batch plus, per shared segment and for the repeat, 80- to 100-base stretches with one planted deletion or
insertion of 1 to 3 bases at least 24 bases from either end (both strands, every third with one substitution), and error-free and
one-substitution stretches of S6, S2 and the repeat: exact and rescued reads with the sets the gap reads have.  S3 has gap reads only."""
import numpy as np

import gap_case
import gap_def
from gap_sets_def import gap_sets
from groot_amd import host
from rescue_def import Tables, _rc, path_texts
from rescue_sets_def import rescued_sets
from test_counter_edges import _of_reads
from test_path_pass import _gfa, _seq
from test_rescue import _has_record, _mut, _reads_of

SEG, FAN = 120, 66
DEL, INS = 0, 1


def _fan_graph(rng, path, name, chain, n_alleles, tail):
    """chain . (allele 0 | allele 1 | ...) . tail, path p through allele p (test_counter_edges._graph's construction)"""
    alleles = []
    while len(alleles) < n_alleles:
        a = _seq(rng, int(rng.integers(3, 6)))
        if a not in alleles:
            alleles.append(a)
    nodes = {i + 1: s for i, s in enumerate(chain + alleles + [tail])}
    m, t = len(chain), len(chain) + len(alleles) + 1
    edges = [(i, i + 1) for i in range(1, m)]
    for a in range(m + 1, t):
        edges += [(m, a), (a, t)]
    return _gfa(path, nodes, edges, [("%sp%d" % (name, p), list(range(1, m + 1)) + [m + 1 + p, t]) for p in range(n_alleles)])


def build_graphs(rng, tmp):
    """-> (the eleven GFA files, {segment name: its text})"""
    files = gap_case.build_graphs(rng, tmp)
    seg = {n: _seq(rng, SEG) for n in ("S6", "S3", "S2")}
    seg["R"] = _seq(rng, 100)
    for g, (extra, n_paths) in enumerate([("S3", 3), ("S3", 2), ("S3", 2), ("S2", 2), (None, 2), (None, 3)]):
        chain = [_seq(rng, 10), seg["S6"]] + ([_seq(rng, 8), seg[extra]] if extra else [])
        files.append(_fan_graph(rng, tmp / ("s%d.gfa" % g), "s%d" % g, chain, n_paths, _seq(rng, 10)))
    nodes = {1: _seq(rng, 12), 2: seg["R"], 3: _seq(rng, 14), 4: seg["R"], 5: _seq(rng, 12)}
    files.append(_gfa(tmp / "twice.gfa", nodes, [(1, 2), (2, 3), (3, 4), (4, 5)], [("r0", [1, 2, 3, 4, 5])]))
    files.append(_fan_graph(rng, tmp / "fan.gfa", "f", [_seq(rng, 4), seg["S2"]], FAN, _seq(rng, 6)))
    return files, {k: v.encode() for k, v in seg.items()}


def make_reads(rng, seg):
    """-> [(class name, read)] of the stretches of the shared segments"""
    out = []

    def put(name, r):
        out.append((name, _rc(r) if len(out) & 1 else r))                  # both strands, in turn

    for name in ("S6", "S3", "S2", "R"):
        t = seg[name]
        for i in range(16):                                                # one planted gap, at least 24 bases from either end
            typ, g = i & 1, 1 + i % 3
            L = int(rng.integers(80, min(100, len(t) - g) + 1))
            x = int(rng.integers(0, len(t) - L - g + 1))
            while True:                                                    # (a deletion out of a run could move to the left: the read is the same)
                k = int(rng.integers(24, (L if typ == DEL else L - g) - 24 + 1))
                r = gap_case.gapped(rng, t, x, L, typ, g, k)
                if typ == DEL or r[k:k + g] != t[x + k:x + k + g]:         # (inserted bases that repeat the text behind them are no insertion)
                    break
            subs = [int(rng.choice([j for j in range(3, L - 3) if j < k - 4 or j > k + g + 4]))] if i % 3 == 2 else []
            put("gap" + name, _mut(rng, r, subs))
    for name in ("S6", "S2", "R"):
        t = seg[name]
        for i in range(12):                                                # error-free, about as long as the index's window: the aligner takes them
            x = int(rng.integers(0, len(t) - 100 + 1))
            put("exact" + name, t[x:x + 100])
        for i in range(12):                                                # one substitution: rescued ungapped
            L = int(rng.integers(80, 101))
            x = int(rng.integers(0, len(t) - L + 1))
            put("sub" + name, _mut(rng, t[x:x + L], [int(rng.integers(20, L - 20))]))
    return out


class Case:
    """the index, the batch, and per (M, G) the definition's S++(r) of every read of the batch"""

    def __init__(self, tmp):
        files, self.seg = build_graphs(np.random.default_rng(21), tmp)
        # (windows of 100 bases: the aligner takes the error-free reads of 96 and 100 bases, so that the batch holds reads with a record)
        self.index = host.Index.from_gfa_files(files, host.index_params(k=7, s=10, w=100))
        texts = path_texts(self.index)
        assert self.index.view.n_paths == 7 + 14 + 1 + FAN and all(t is not None and t[1] == 0 for t in texts)
        assert self.index.view.path_words == 2 and sum(len(t[0]) for t in texts) <= 16000
        named = gap_case.make_reads(np.random.default_rng(22), texts) + make_reads(np.random.default_rng(25), self.seg)
        order = np.random.default_rng(23).permutation(len(named))
        self.names = [named[i][0] for i in order]
        self.batch = _of_reads("gap ec classes", [named[i][1] for i in order])
        self.reads = _reads_of(self.batch)
        self.has = _has_record(self.batch, self.index)
        self.gpo = self.index.arrays["graph_path_off"].astype(np.int64)
        self._tables = Tables(self.index, 1)                               # (the windows of the texts, shared by every M)
        self._brute = {}
        self._res, self._gap = {}, {}

    def placements(self, M, G):
        """read -> every gapped placement with d <= M and g <= G at least.  A brute force with gaps up to 3 serves G <= 3; for a larger G
        a read with e* <= 3 under G = 3 keeps its placements (one with g >= 4 costs e >= 4), every other read is searched with gaps up to 8"""
        def brute(g_max):
            if g_max not in self._brute:
                self._brute[g_max] = gap_def.Brute(self.index, 2, g_max=g_max)
            return self._brute[g_max]

        def of(read):
            pl = brute(3).placements(read)
            if G <= 3:
                return pl
            e = gap_def.keep(pl, M, 3)[0]
            return pl if e is not None and e <= 3 else brute(gap_def.G_MAX).placements(read)

        return of

    def exact(self, batch=None):
        """{read: S(r)} of the reads with a record"""
        w = (batch or self.batch).want(self.index)
        r, p = w.read_ref >> 10, w.read_ref & 1023
        starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]]) if len(r) else np.zeros(0, dtype=np.int64)
        return {int(r[s]): tuple(int(v) for v in p[s:e]) for s, e in zip(starts, np.r_[starts[1:], len(r)])}

    def rescued(self, M):
        if M not in self._res:
            self._res[M] = rescued_sets(self.index, M, self.reads, self.has, self._tables)
        return self._res[M]

    def gapped(self, M, G):
        if (M, G) not in self._gap:
            self._gap[M, G] = gap_sets(self.index, M, G, self.reads, self.has, self.placements(M, G))
        return self._gap[M, G]

    def graphs_of(self, ids):
        return len(set((np.searchsorted(self.gpo, np.array(ids), side="right") - 1).tolist()))


_CASE = {}


def case(tmp_path_factory):
    """built once per session, for every test module"""
    if not _CASE:
        _CASE["case"] = Case(tmp_path_factory.mktemp("gap_ec"))
    return _CASE["case"]
