"""The definition of gapped rescue (include/groot_hip.h, "gapped rescue") as a brute force, for the tests that check the device tables
(tests/test_gap_rescue.py): over ALL (path, strand, x, type, g, k), with no anchor, no table and no knowledge of the kernel.  "Candidate
and not rescued" comes from rescue_def.Tables, "has a record" from the caller (the CPU oracle's records).  numpy only.

Per (oriented read R, text T) one table E[y][i] = (R[i] != T[y + i]) and its prefix sums C[y][i] = |E[y][0, i)| are built once; then
    DEL:  d(x, k) = C[x][k] + C[x + g][len] - C[x + g][k]            (R[k, len) lies on T[x + k + g, ..): the diagonal of y = x + g)
    INS:  d(x, k) = C[x][k] + C[x - g][len] - C[x - g][k + g]        (R[k + g, len) lies on T[x + k, ..): the diagonal of y = x - g)
are two look-ups each.  y runs from -8, over a text padded with bytes that no read holds; a padded cell is never inside a window W."""
import numpy as np

from rescue_def import A, Tables, _rc, path_texts

G_MAX = 8
DEL, INS = 0, 1
STATS = ("candidates", "rescued", "placements", "del_placements", "ins_placements", "too_short")
_CODE = {c: i for i, c in enumerate(b"ACGT")}


class Brute:
    """every gapped placement (p, strand, x, type, g) with d <= m_max and g <= g_max of a read, with its d and k*: computed once per read"""

    def __init__(self, index, m_max, texts=None, g_max=G_MAX):
        """texts: [(text as bytes, first Position) or None] in place of the index's (hand-made cases); g_max: no gap longer than that is looked for"""
        self.m_max, self.g_max = m_max, g_max
        self.plen = index.arrays["path_len"].astype(np.int64) if texts is None else np.array([len(t[0]) + t[1] if t else 0 for t in texts], dtype=np.int64)
        self.texts = []
        for p, t in enumerate(path_texts(index) if texts is None else texts):
            if t is None:
                self.texts.append(None)
                continue
            s, first = np.frombuffer(t[0], dtype=np.uint8), t[1]
            n = max(min(len(s), int(self.plen[p]) - first), 0)        # the bases inside path_len
            self.texts.append((s[:n], first, np.r_[0, np.cumsum(~np.isin(s[:n], np.frombuffer(b"ACGT", dtype=np.uint8)))]))
        self._memo = {}

    def placements(self, read):
        """-> [(p, strand, x, type, g, d, k*)]"""
        if read not in self._memo:
            out = []
            L = len(read)
            for strand, ori in enumerate((read, _rc(read))):
                R = np.frombuffer(ori, dtype=np.uint8)
                for p, t in enumerate(self.texts):
                    if t is None or len(t[0]) < L - G_MAX:
                        continue
                    T, _, n_cum = t
                    n = len(T)
                    pad = np.r_[np.zeros(G_MAX, np.uint8), T, np.zeros(L + G_MAX, np.uint8)]
                    E = np.lib.stride_tricks.sliding_window_view(pad, L)[:n + G_MAX] != R                # row y + 8: the diagonal of y
                    C = np.zeros((n + G_MAX, L + 1), dtype=np.int32)
                    np.cumsum(E, axis=1, out=C[:, 1:])
                    for g in range(1, self.g_max + 1):
                        for typ in (DEL, INS):
                            wlen = L + g if typ == DEL else L - g
                            if wlen > n:
                                continue
                            xs = np.arange(0, n - wlen + 1)
                            xs = xs[n_cum[xs + wlen] == n_cum[xs]]                                  # no 'N' in W
                            if not len(xs):
                                continue
                            ks = np.arange(A, (L - A if typ == DEL else L - g - A) + 1)
                            if not len(ks):
                                continue
                            pre = C[xs + G_MAX][:, ks]
                            y = xs + G_MAX + (g if typ == DEL else -g)
                            suf = C[y, L][:, None] - C[y][:, ks + (0 if typ == DEL else g)]
                            d = pre + suf
                            kstar = d.argmin(axis=1)                                                   # the first minimum: the smallest k
                            dmin = d[np.arange(len(xs)), kstar]
                            for i in np.flatnonzero(dmin <= self.m_max):
                                out.append((p, strand, int(xs[i]), typ, g, int(dmin[i]), int(ks[kstar[i]])))
            self._memo[read] = out
        return self._memo[read]


def keep(placements, M, G):
    """-> (e*, the kept placements) under (M, G), or (None, []) when there is none"""
    pl = [x for x in placements if x[5] <= M and x[4] <= G]
    if not pl:
        return None, []
    e = min(x[5] + x[4] for x in pl)
    return e, [x for x in pl if x[5] + x[4] == e]


def event_of(placement, read, first=0):
    """(path, pos, type, g, seq) of a placement of `read`"""
    p, strand, x, typ, g, d, k = placement
    ori = read if strand == 0 else _rc(read)
    return (p, first + x + k - 1, typ, g, sum(_CODE[ori[k + j]] << (2 * j) for j in range(g)) if typ == INS else 0)


class GapTables:
    """gdepth / events / stats of the definition for (M, G), summed over the batches given to add()"""

    def __init__(self, index, M, G, brute):
        assert M <= brute.m_max and 1 <= G <= brute.g_max
        self.index, self.M, self.G, self.brute = index, M, G, brute
        self.base = np.r_[0, np.cumsum(brute.plen)]
        self.gdepth = np.zeros(int(self.base[-1]), dtype=np.int64)
        self.events = {}                                             # (path, pos, type, g, seq) -> reads
        self.stats = dict.fromkeys(STATS, 0)
        self.per_read = []                                           # per gap candidate of every batch added: (batch-relative read, e* or None, kept placements)

    def add(self, reads, has_record):
        t = Tables(self.index, self.M)
        t.add(reads, has_record)
        for i, d_star, _ in t.d_star:
            if d_star is not None:
                continue                                             # rescued ungapped: never looked at
            r = reads[i]
            if len(r) < A * (self.M + 3):
                self.stats["too_short"] += 1
                continue
            self.stats["candidates"] += 1
            e, kept = keep(self.brute.placements(r), self.M, self.G)
            self.per_read.append((i, e, kept))
            if e is None:
                continue
            self.stats["rescued"] += 1
            self.stats["placements"] += len(kept)
            for p, strand, x, typ, g, d, k in kept:
                first = self.brute.texts[p][1]
                X = int(self.base[p]) + first + x
                L = len(r)
                if typ == DEL:
                    self.stats["del_placements"] += 1
                    self.gdepth[X:X + k] += 1
                    self.gdepth[X + k + g:X + L + g] += 1
                else:
                    self.stats["ins_placements"] += 1
                    self.gdepth[X:X + L - g] += 1
                key = event_of((p, strand, x, typ, g, d, k), r, first)
                self.events[key] = self.events.get(key, 0) + 1

    def sorted_events(self):
        return [k + (v,) for k, v in sorted(self.events.items())]
