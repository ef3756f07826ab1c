"""The definition of mismatch rescue (include/groot_hip.h, "mismatch rescue") as a brute force, for the tests that check the device tables
(tests/test_rescue.py), the writer (tests/test_variants.py) and the command line (tests/test_variants_cli.py): path_texts gives the texts of
the definition from an index view, Tables the rescued depth, the alt counts and the stats over ALL (path, strand, x), with no anchor, no
table and no knowledge of the kernels.  numpy only."""
import numpy as np

A = 16
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rc(s):
    return s.translate(_COMP)[::-1]


# ---- the definition -------------------------------------------------------------------------------------------------------------

def path_texts(index):
    """per global path: (its text as bytes, Position of its first node), or None where build_path_tables gives none"""
    a = {k: v.astype(np.int64) for k, v in index.arrays.items() if k != "bases"}
    bases = index.arrays["bases"].tobytes()
    v = index.view
    on = [[] for _ in range(v.n_paths)]
    for g in range(v.n_graphs):
        for n in range(a["graph_node_off"][g], a["graph_node_off"][g + 1]):
            for i in range(a["node_np_off"][n], a["node_np_off"][n + 1]):
                on[a["graph_path_off"][g] + a["np_path"][i]].append((int(a["np_pos"][i]), int(n)))
    out = []
    for nodes in on:
        nodes.sort()
        seq = lambda n: bases[a["node_seq_off"][n]:a["node_seq_off"][n + 1]]
        kids = lambda n: set(a["edges"][a["node_edge_off"][n]:a["node_edge_off"][n + 1]].tolist())
        ok = bool(nodes) and all(len(seq(n)) for _, n in nodes)
        ok = ok and all(p + len(seq(n)) == p2 and n2 in kids(n) for (p, n), (p2, n2) in zip(nodes, nodes[1:]))
        out.append((b"".join(seq(n) for _, n in nodes), nodes[0][0]) if ok else None)
    return out


class Tables:
    """rdepth / alt / stats of the definition, summed over the batches given to add()"""

    def __init__(self, index, M):
        self.M, self.texts = M, path_texts(index)
        self.plen = index.arrays["path_len"].astype(np.int64)
        self.base = np.r_[0, np.cumsum(self.plen)]
        n = int(self.base[-1])
        self.diff = np.zeros(n + 1, dtype=np.int64)            # += 1 at a placement's first base, -= 1 behind its last (its path's slots only)
        self.alt = np.zeros((n, 4), dtype=np.int64)
        self.stats = dict.fromkeys(("candidates", "rescued", "exact", "placements", "too_short", "non_acgt"), 0)
        self.d_star = []                                        # per candidate of every batch added: (batch-relative read, d* or None, kept placements)
        self._win = {}

    def _windows(self, L):
        """every window of L bases of every text that lies inside path_len and holds A/C/G/T only -> (one-hot [n, 4L] f32, bytes [n, L], slot of the first base [n])"""
        if L not in self._win:
            rows, at = [], []
            for p, t in enumerate(self.texts):
                if t is None:
                    continue
                s, first = np.frombuffer(t[0], dtype=np.uint8), t[1]
                n = min(len(s), int(self.plen[p]) - first)
                if n < L:
                    continue
                w = np.lib.stride_tricks.sliding_window_view(s[:n], L)
                ok = np.isin(w, _ACGT).all(axis=1)
                rows.append(w[ok])
                at.append(self.base[p] + first + np.flatnonzero(ok))
            w = np.concatenate(rows) if rows else np.zeros((0, L), dtype=np.uint8)
            self._win[L] = ((w[:, :, None] == _ACGT).reshape(len(w), 4 * L).astype(np.float32), w, np.concatenate(at) if at else np.zeros(0, dtype=np.int64))
        return self._win[L]

    def add(self, reads, has_record):
        by_len = {}
        for i, r in enumerate(reads):
            if has_record[i]:
                continue
            if not all(c in b"ACGT" for c in r):
                self.stats["non_acgt"] += 1
            elif len(r) < A * (self.M + 1):
                self.stats["too_short"] += 1
            else:
                by_len.setdefault(len(r), []).append(i)
        for L, idx in sorted(by_len.items()):
            oh, w, at = self._windows(L)
            for c0 in range(0, len(idx), 256):
                chunk = idx[c0:c0 + 256]
                ori = np.array([np.frombuffer(o, dtype=np.uint8) for i in chunk for o in (reads[i], _rc(reads[i]))])      # [2n, L]: strand 0, strand 1
                d = L - np.rint(oh @ (ori[:, :, None] == _ACGT).reshape(len(ori), 4 * L).astype(np.float32).T).astype(np.int64) if len(w) else np.zeros((0, len(ori)), dtype=np.int64)
                for j, i in enumerate(chunk):
                    self.stats["candidates"] += 1
                    dj = d[:, 2 * j:2 * j + 2]
                    best = int(dj.min()) if dj.size else self.M + 1
                    if best > self.M:
                        self.d_star.append((i, None, 0))
                        continue
                    self.stats["rescued"] += 1
                    self.stats["exact"] += best == 0
                    kept = 0
                    for strand in (0, 1):
                        rows = np.flatnonzero(dj[:, strand] == best)
                        kept += len(rows)
                        np.add.at(self.diff, at[rows], 1)
                        np.add.at(self.diff, at[rows] + L, -1)
                        o = ori[2 * j + strand]
                        rr, cc = np.nonzero(w[rows] != o)
                        np.add.at(self.alt, (at[rows][rr] + cc, np.searchsorted(_ACGT, o[cc])), 1)
                    self.stats["placements"] += kept
                    self.d_star.append((i, best, kept))

    def depth(self):
        # a placement ends inside its own path, so its -1 falls at most on the next path's first slot: the running sum is per path all the same
        return np.cumsum(self.diff[:-1]).astype(np.uint64)
