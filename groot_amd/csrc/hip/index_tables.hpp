// index_tables.hpp -- the device tables of a ctx as plain host functions: groot_index_view (+ a few scalars) -> std::vectors holding exactly
// the bytes open.hip uploads, padding and sentinel entries included.  No HIP runtime call and no ctx: tools/open_tables_check.cpp runs
// every builder on a CPU under the sanitizers (tests/test_open_tables.py).
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <numeric>
#include <thread>
#include <utility>
#include <vector>

#include "device_types.hpp"
#include "groot_index.h"

namespace groot {

// 2-bit code of a graph base (A=0 C=1 T=2 G=3, (b >> 1) & 3 for those four), -1 for any other byte
inline int code_of(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'T' ? 2 : b == 'G' ? 3 : -1; }
// base i of a text at 2 bits per base, 16 to a dword (the words start out zero)
inline void put2(uint32_t *words, size_t i, uint32_t code) { words[i >> 4] |= code << (2 * (i & 15)); }
// The first-pass kernels address their 2-bit texts (LeanArgs::bases2, LeanArgs::path_text) with 32-bit bit offsets and read up to 512 bases
// past a position: a text of this many bases can be addressed that way
inline bool bit_addressable32(uint64_t n_bases) { return n_bases + 512 < (1ull << 31); }
// graph of every node
inline std::vector<uint32_t> build_node_graph(const groot_index_view *v)
{
    std::vector<uint32_t> g_of(v->n_nodes, 0);
    for (uint32_t g = 0; g < v->n_graphs; g++)
        for (uint32_t n = v->graph_node_off[g]; n < v->graph_node_off[g + 1]; n++) g_of[n] = g;
    return g_of;
}

inline uint32_t round_pw(uint32_t pw)
{
    for (uint32_t c : {3u, 11u})   // NodeRec<3> = 64 B, NodeRec<11> = 128 B
        if (pw <= c) return c;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// LSH Ensemble parameters (github.com/ekzhu/lshensemble v1.1.0: OptimalKL, Containment), computed
// once per possible kmerCount at open -- the reference caches them per (x, q, t) at query time.
// ---------------------------------------------------------------------------------------------
struct KLProb {
    int x, q, l, k;
    double p(double t) const { return 1.0 - std::pow(1.0 - std::pow(t / (1.0 + double(x) / double(q) - t), double(k)), double(l)); }
};

template <class F> double integrate(F f, double a, double b, double precision)
{
    double area = 0.0;
    for (double x = a; x < b; x += precision) area += f(x + 0.5 * precision) * precision;
    return area;
}

inline void optimal_kl(int max_k, int max_l, int x, int q, double t, int &opt_k, int &opt_l)
{
    const double prec = 0.01;
    double min_err = 1.7976931348623157e308;
    opt_k = 0; opt_l = 0;
    const double xq = double(x) / double(q);
    for (int l = 1; l <= max_l; l++)
        for (int k = 1; k <= max_k; k++) {
            KLProb pr{x, q, l, k};
            double fp = 0.0, fn = 0.0;
            if (xq >= 1.0) {
                fp = integrate([&](double v) { return pr.p(v); }, 0.0, t, prec);
                fn = integrate([&](double v) { return 1.0 - pr.p(v); }, t, 1.0, prec);
            } else if (xq >= t) {
                fp = integrate([&](double v) { return pr.p(v); }, 0.0, t, prec);
                fn = integrate([&](double v) { return 1.0 - pr.p(v); }, t, xq, prec);
            }
            const double err = fn + fp;
            if (min_err > err) { min_err = err; opt_k = k; opt_l = l; }
        }
}

// smallest eq in [1, s] with Containment(eq) > t (monotone in eq); s+1 if none
inline uint32_t min_equal_slots(uint32_t s, int q_size, int x_size, double t)
{
    if (q_size == 0 || x_size == 0) return s + 1;
    for (uint32_t eq = 1; eq <= s; eq++) {
        const double jaccard = double(eq) / double(s);
        const double c = (double(x_size) / double(q_size) + 1.0) * jaccard / (1.0 + jaccard);
        if (c > t) return eq;
    }
    return s + 1;
}

// per kmerCount 0..max_q: (K, L) of the partitions (all have Upper = NumWindowKmers) and min #equal slots
struct QTables {
    std::vector<uint8_t> k, l;
    std::vector<uint16_t> min_eq;
};
inline QTables build_q_tables(const groot_index_view *v, uint32_t max_q, uint32_t l_max, double threshold)
{
    const uint32_t s = v->sketch_size;
    QTables t{std::vector<uint8_t>(max_q + 1, 0), std::vector<uint8_t>(max_q + 1, 0), std::vector<uint16_t>(max_q + 1, (uint16_t)(s + 1))};
    for (uint32_t q = 1; q <= max_q; q++) {
        int K, L;
        optimal_kl((int)v->max_k, (int)l_max, (int)v->num_window_kmers, (int)q, threshold, K, L);
        t.k[q] = (uint8_t)K; t.l[q] = (uint8_t)L;
        t.min_eq[q] = (uint16_t)min_equal_slots(s, (int)q, (int)v->num_window_kmers, threshold);
    }
    return t;
}

// ---- the first pass against path text (kernels_path.hpp): what it reads ----
struct PathTables {
    std::vector<uint4> node;           // LeanArgs::path_node, two per node
    std::vector<uint32_t> text, tag;   // LeanArgs::path_text / path_tag
    std::vector<uint32_t> nodes;       // LeanArgs::path_nodes
    std::vector<uint64_t> tab;         // LeanArgs::path_tab (three words per entry)
    uint32_t n_text_paths = 0;
    size_t n_bases = 0;
    // per global path (not uploaded; build_rescue_tables reads them): where its text starts (kEmpty: it has none), its bases, the Position of its first node
    std::vector<uint32_t> path_at, path_bases, path_first;
};
// false: the paths' texts are not bit_addressable32: no first pass against path text
inline bool build_path_tables(const groot_index_view *v, const std::vector<uint32_t> &gnode, PathTables &pt)
{
    auto nlen = [&](uint32_t n) { return v->node_seq_off[n + 1] - v->node_seq_off[n]; };
    // flag[n]: the DFS's step out of node n is not decided by the read's next base alone -- more than four OutEdges (the node records
    // hold four), two non-empty neighbours with the same first base, a neighbour that starts with an 'N'
    std::vector<uint8_t> flag(v->n_nodes, 0);
    for (uint32_t n = 0; n < v->n_nodes; n++) {
        const uint32_t e0 = v->node_edge_off[n], deg = v->node_edge_off[n + 1] - e0;
        uint32_t seen = 0;
        bool f = deg > 4;
        for (uint32_t e = 0; e < deg && !f; e++) {
            const uint32_t ch = v->edges[e0 + e];
            if (nlen(ch) == 0) continue;                   // never entered (dfsRecursive returns at once)
            const int cd = code_of(v->bases[v->node_seq_off[ch]]);
            if (cd < 0 || (seen >> cd) & 1u) f = true;
            else seen |= 1u << cd;
        }
        flag[n] = f;
    }
    auto has_edge = [&](uint32_t a, uint32_t b) {
        for (uint32_t e = v->node_edge_off[a]; e < v->node_edge_off[a + 1]; e++)
            if (v->edges[e] == b) return true;
        return false;
    };
    // every path's nodes by position; a path has a text when its nodes are non-empty, follow each other without gap or overlap, and are
    // joined by OutEdges -- then its text is exactly what the DFS spells along it
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> pl(v->n_paths);
    for (uint32_t n = 0; n < v->n_nodes; n++)
        for (uint32_t i = v->node_np_off[n]; i < v->node_np_off[n + 1]; i++) {
            const uint32_t gp = v->graph_path_off[gnode[n]] + v->np_path[i];
            if (gp < v->n_paths) pl[gp].push_back({v->np_pos[i], n});
        }
    std::vector<uint8_t> ok(v->n_paths, 0);
    size_t total = 0;
    for (uint32_t p = 0; p < v->n_paths; p++) {
        auto &L = pl[p];
        std::sort(L.begin(), L.end());
        bool good = !L.empty();
        for (size_t i = 0; good && i < L.size(); i++) {
            if (nlen(L[i].second) == 0) good = false;
            else if (i + 1 < L.size() && ((uint64_t)L[i].first + nlen(L[i].second) != L[i + 1].first || !has_edge(L[i].second, L[i + 1].second))) good = false;
        }
        if (!good) continue;
        ok[p] = 1;
        pt.n_text_paths++;
        total += (uint64_t)L.back().first + nlen(L.back().second) - L.front().first;
    }
    pt.n_bases = total;
    if (!bit_addressable32(total)) return false;
    pt.path_at.assign(v->n_paths, kEmpty); pt.path_bases.assign(v->n_paths, 0); pt.path_first.assign(v->n_paths, 0);
    pt.text.assign(total / 16 + 20, 0);
    pt.tag.assign(total / 16 + 20, 0);
    pt.node.assign((size_t)v->n_nodes * 2, make_uint4(kEmpty, 0, 0, 0));
    const uint32_t pw = std::min<uint32_t>(v->path_words, 3);
    size_t at = 0;
    for (uint32_t p = 0; p < v->n_paths; p++) {
        if (!ok[p]) continue;
        const auto &L = pl[p];
        const uint32_t n = (uint32_t)L.size(), nbase = (uint32_t)pt.nodes.size(), tbase = (uint32_t)(pt.tab.size() / 3);
        const uint32_t tend = (uint32_t)(at + (L.back().first + nlen(L.back().second) - L.front().first));
        pt.path_at[p] = (uint32_t)at; pt.path_bases[p] = tend - (uint32_t)at; pt.path_first[p] = L.front().first;
        uint32_t levels = 1;
        while ((2ull << (levels - 1)) <= n) levels++;
        pt.tab.resize(pt.tab.size() + (size_t)3 * levels * n, 0);
        uint64_t *T = pt.tab.data() + (size_t)3 * tbase;
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t w = 0; w < pw; w++) T[(size_t)3 * i + w] = v->node_mask[(size_t)L[i].second * v->path_words + w];
        for (uint32_t k = 1; k < levels; k++)
            for (uint32_t i = 0; i + (1u << k) <= n; i++)
                for (uint32_t w = 0; w < 3; w++)
                    T[(size_t)3 * ((size_t)k * n + i) + w] = T[(size_t)3 * ((size_t)(k - 1) * n + i) + w] & T[(size_t)3 * ((size_t)(k - 1) * n + i + (1u << (k - 1))) + w];
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t nd = L[i].second, s0 = v->node_seq_off[nd], len = nlen(nd);
            if (pt.node[2 * (size_t)nd].x == kEmpty) {          // the node's lowest path with a text
                pt.node[2 * (size_t)nd] = make_uint4((uint32_t)at, i, tend, nbase);
                pt.node[2 * (size_t)nd + 1] = make_uint4(tbase, n, 0, 0);
            }
            pt.nodes.push_back(nd);
            for (uint32_t j = 0; j < len; j++, at++) {
                const int cd = code_of(v->bases[s0 + j]);
                const uint32_t tg = j == 0 ? 1u | ((i > 0 && flag[L[i - 1].second]) ? 2u : 0u) : (cd < 0 ? 2u : 0u);
                put2(pt.text.data(), at, (uint32_t)(cd < 0 ? 0 : cd));
                put2(pt.tag.data(), at, tg);
            }
        }
    }
    if (pt.nodes.empty()) pt.nodes.push_back(0);
    if (pt.tab.empty()) pt.tab.assign(3, 0);
    return true;
}

// ---- mismatch rescue (kernels_rescue.hpp): the path texts once more, and an exact table of their 16-mers ----
// tab: open addressing over the distinct 16-mers of all texts that hold no 'N' (mask = tab.size() - 1, slot = rescue_hash(key) & mask, linear
// probing): {key = the 16 bases at 2 bits each, first occurrence in occ, occurrences, 0}; occurrences == 0: the slot is free.  The key is the
// whole 16-mer, so a hit is never a false positive.  occ: {global path, offset of the 16-mer in the text array}, a key's occurrences back to
// back, ascending by (path, offset).  path: per global path {start of its text in the text array (kEmpty: no text), its bases (those inside path_len),
// Position of its first node, 0}.
struct RescueTables {
    std::vector<uint32_t> text;            // PathTables::text
    std::vector<uint32_t> tag;             // laid out like it; bit 0 of a base's two: the graph has no A/C/G/T there ('N').  (PathTables::tag cannot
                                           // say so for a node's first base, where it holds the boundary flags.)
    std::vector<uint4> path, tab;
    std::vector<uint2> occ;
    uint32_t n_text_paths = 0;
    size_t n_bases = 0, n_kmers = 0;
};
// the 16 bases from base i of a 2-bit text as one dword
inline uint32_t get32(const uint32_t *words, size_t i)
{
    const uint64_t two = (uint64_t)words[i >> 4] | ((uint64_t)words[(i >> 4) + 1] << 32);
    return (uint32_t)(two >> (2 * (i & 15)));
}
// false: the paths' texts are not bit_addressable32 (no rescue on such an index)
inline bool build_rescue_tables(const groot_index_view *v, RescueTables &rt)
{
    PathTables pt;
    if (!build_path_tables(v, build_node_graph(v), pt)) return false;
    rt.text.swap(pt.text);
    rt.tag.assign(rt.text.size(), 0);
    {
        size_t at = 0, nd = 0;             // pt.nodes lists the nodes of the paths with a text, path after path
        for (uint32_t p = 0; p < v->n_paths; p++) {
            if (pt.path_at[p] == kEmpty) continue;
            for (const size_t end = at + pt.path_bases[p]; at < end; nd++) {
                const uint32_t n = pt.nodes[nd];
                for (uint32_t i = v->node_seq_off[n]; i < v->node_seq_off[n + 1]; i++, at++)
                    if (code_of(v->bases[i]) < 0) put2(rt.tag.data(), at, 1u);
            }
        }
    }
    rt.n_text_paths = pt.n_text_paths; rt.n_bases = pt.n_bases;
    rt.path.assign(v->n_paths, make_uint4(kEmpty, 0, 0, 0));
    // every 16-mer without an 'N' as key << 32 | its number in (path, offset) order; sorted, a key's occurrences are neighbours in that order
    std::vector<uint64_t> all;
    std::vector<uint2> where;
    for (uint32_t p = 0; p < v->n_paths; p++) {
        if (pt.path_at[p] == kEmpty) continue;
        const uint32_t at = pt.path_at[p], n = pt.path_bases[p];
        // (bases past path_len, were a view to claim fewer than its nodes spell, take no placement: the dense tables end at path_len)
        const uint32_t first = pt.path_first[p], inside = v->path_len[p] > first ? std::min(n, v->path_len[p] - first) : 0u;
        rt.path[p] = make_uint4(at, inside, first, 0);
        uint32_t clean = 0;                 // bases since the last 'N'
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t tg = (rt.tag[(at + i) >> 4] >> (2 * ((at + i) & 15))) & 3u;
            clean = tg ? 0 : clean + 1;
            if (clean < kRescueAnchor) continue;
            const uint32_t s = at + i + 1 - kRescueAnchor;
            all.push_back((uint64_t)get32(rt.text.data(), s) << 32 | where.size());
            where.push_back(make_uint2(p, s));
        }
    }
    std::sort(all.begin(), all.end());
    for (size_t i = 0; i < all.size(); i++)
        if (i == 0 || (all[i] >> 32) != (all[i - 1] >> 32)) rt.n_kmers++;
    uint32_t cap = 16;
    while (cap < 2 * (uint64_t)rt.n_kmers) cap <<= 1;
    rt.tab.assign(cap, make_uint4(0, 0, 0, 0));
    rt.occ.resize(std::max<size_t>(all.size(), 1), make_uint2(0, 0));
    for (size_t i = 0; i < all.size();) {
        size_t j = i;
        while (j < all.size() && (all[j] >> 32) == (all[i] >> 32)) { rt.occ[j] = where[(uint32_t)all[j]]; j++; }
        const uint32_t key = (uint32_t)(all[i] >> 32);
        uint32_t slot = rescue_hash(key) & (cap - 1);
        while (rt.tab[slot].z) slot = (slot + 1) & (cap - 1);
        rt.tab[slot] = make_uint4(key, (uint32_t)i, (uint32_t)(j - i), 0);
        i = j;
    }
    return true;
}

// AlignArgs::node_rec: NodeRec<pw> of every node, pw = 3 or 11 (round_pw)
template <int PW> void build_node_records(const groot_index_view *v, std::vector<unsigned char> &out)
{
    std::vector<NodeRec<PW>> recs(v->n_nodes);
    for (uint32_t n = 0; n < v->n_nodes; n++) {
        NodeRec<PW> &r = recs[n];
        memset(&r, 0, sizeof r);
        r.seq_off = v->node_seq_off[n];
        r.seq_len = v->node_seq_off[n + 1] - v->node_seq_off[n];
        const uint32_t e0 = v->node_edge_off[n], deg = v->node_edge_off[n + 1] - e0;
        bool wild = false;
        for (uint32_t i = 0; i < r.seq_len; i++) wild |= v->bases[r.seq_off + i] == 'N';
        r.deg = deg | (wild ? 0x80000000u : 0u);        // bit 31: the node holds an 'N' (the wildcard of alignment.go:212-222)
        if (deg <= 4) {
            for (uint32_t e = 0; e < deg; e++) {
                const uint32_t c = v->edges[e0 + e];
                r.edges[e] = c;
                r.child_first[e] = v->node_seq_off[c] < v->node_seq_off[c + 1] ? v->bases[v->node_seq_off[c]] : (uint8_t)0;   // (an empty node spells nothing)
            }
        } else {
            r.edges[0] = e0;
        }
        for (uint32_t i = 0; i < 8 && i < r.seq_len; i++) r.first8 |= (uint64_t)v->bases[r.seq_off + i] << (8 * i);
        for (uint32_t w = 0; w < v->path_words; w++) r.mask[w] = v->node_mask[(size_t)n * v->path_words + w];
    }
    out.resize(recs.size() * sizeof(NodeRec<PW>));
    if (!recs.empty()) memcpy(out.data(), recs.data(), out.size());
}
inline std::vector<unsigned char> build_node_records(const groot_index_view *v, uint32_t pw)
{
    std::vector<unsigned char> recs;
    if (pw == 3) build_node_records<3>(v, recs);
    else build_node_records<11>(v, recs);
    return recs;
}

// ---- first pass of the align stage (kernels_lean.hpp): everything at 2 bits per base; needs bit_addressable32(v->n_bases) ----
struct LeanTables {
    std::vector<uint32_t> bases2;      // LeanArgs::bases2
    std::vector<LeanNode> nodes;
    std::vector<LeanExt> ext;
    std::vector<uint32_t> cn_pre2;     // LeanArgs::cn_pre2, four dwords per entry
    std::vector<uint8_t> win_ok;
};
inline LeanTables build_lean_tables(const groot_index_view *v)
{
    LeanTables t;
    t.bases2.assign((size_t)(v->n_bases + 15) / 16 + 20, 0);
    for (uint64_t i = 0; i < v->n_bases; i++) {
        const int cd = code_of(v->bases[i]);
        if (cd > 0) put2(t.bases2.data(), i, (uint32_t)cd);
    }
    t.nodes.resize(v->n_nodes);
    t.ext.resize(v->n_nodes);
    std::vector<uint8_t> node_bad(v->n_nodes, 0);
    for (uint32_t n = 0; n < v->n_nodes; n++) {
        LeanNode &r = t.nodes[n];
        memset(&r, 0, sizeof r);
        memset(&t.ext[n], 0, sizeof(LeanExt));
        r.seq_off = v->node_seq_off[n];
        r.seq_len = v->node_seq_off[n + 1] - v->node_seq_off[n];
        const uint32_t e0 = v->node_edge_off[n], deg = v->node_edge_off[n + 1] - e0;
        bool no = deg > 4;
        for (uint32_t i = 0; i < r.seq_len; i++) {
            const int cd = code_of(v->bases[r.seq_off + i]);
            if (cd < 0) no = true;                             // the graph's 'N' (alignment.go:212-222): align_kernel's business
            else if (i < 32) r.first32 |= (uint64_t)cd << (2 * i);
            else if (i < 256) t.ext[n].b[(i >> 5) - 1] |= (uint64_t)cd << (2 * (i & 31));
        }
        node_bad[n] = no;
        r.deg_kids = std::min(deg, 7u) | (no ? kLeanNo : 0u);
        for (uint32_t e = 0; e < std::min(deg, 4u); e++) {
            const uint32_t ch = v->edges[e0 + e];
            r.edges[e] = ch;
            uint32_t kid = 8;                                   // an empty neighbour spells nothing: never entered
            if (v->node_seq_off[ch] < v->node_seq_off[ch + 1]) {
                const int cd = code_of(v->bases[v->node_seq_off[ch]]);
                kid = cd < 0 ? 4u : (uint32_t)cd;
            }
            r.deg_kids |= kid << (8 + 4 * e);
            if (v->node_seq_off[ch + 1] - v->node_seq_off[ch] > 32u) r.deg_kids |= 1u << (24 + e);
        }
        for (uint32_t w = 0; w < v->path_words && w < 3; w++) r.mask[w] = v->node_mask[(size_t)n * v->path_words + w];
    }
    t.cn_pre2.assign((size_t)v->n_cn * 4 + 4, 0);
    for (uint64_t i = 0; i < v->n_cn; i++) {
        const uint32_t nd = v->cn_node[i];
        const uint32_t s0 = v->node_seq_off[nd], nlen = v->node_seq_off[nd + 1] - s0;
        uint64_t bits = 0;
        for (uint32_t j = 0; j < std::min(nlen, 24u); j++) {
            const int cd = code_of(v->bases[s0 + j]);
            if (cd > 0) bits |= (uint64_t)cd << (2 * j);
        }
        uint32_t *e = &t.cn_pre2[(size_t)i * 4];
        e[0] = (uint32_t)bits; e[1] = (uint32_t)(bits >> 32) | (std::min(nlen, 65535u) << 16); e[2] = nd; e[3] = s0;
    }
    t.win_ok.assign(v->n_windows, 1);
    for (uint32_t w = 0; w < v->n_windows; w++) {
        if (node_bad[v->win_node[w]]) t.win_ok[w] = 0;
        for (uint32_t i = v->win_cn_off[w]; i < v->win_cn_off[w + 1]; i++) {
            const uint32_t nd = v->cn_node[i];
            if (node_bad[nd] || v->node_seq_off[nd + 1] - v->node_seq_off[nd] > 65535u) t.win_ok[w] = 0;
        }
    }
    return t;
}

// level 2 of AlignRead: the first 24 bases, index and length of every ContainedNodes entry, in list order (DeviceIndex::cn_pre, eight dwords per entry)
inline std::vector<uint32_t> build_cn_pre(const groot_index_view *v)
{
    std::vector<uint32_t> pre((size_t)v->n_cn * 8 + 8, 0);
    for (uint64_t i = 0; i < v->n_cn; i++) {
        const uint32_t nd = v->cn_node[i];
        const uint32_t s0 = v->node_seq_off[nd], nlen = v->node_seq_off[nd + 1] - s0;
        uint32_t *e = &pre[(size_t)i * 8];
        memcpy(e, v->bases + s0, std::min(nlen, 24u));
        e[6] = nd; e[7] = nlen;
    }
    return pre;
}

// the 8-mers a DFS from one (node, offset) can spell, as a set of l2_bloom_bits
struct L2Walk {
    const groot_index_view *v;
    uint64_t set = 0;
    uint32_t budget = 0;
    // the strings of length 8 that start with `code` (d bases so far) and go on at (node, off)
    void go(uint32_t node, uint32_t off, uint32_t d, uint32_t code)
    {
        if (set == ~0ull) return;
        if (++budget > 4096) { set = ~0ull; return; }               // (a thicket of N and branches: anything goes)
        const uint32_t s0 = v->node_seq_off[node], len = v->node_seq_off[node + 1] - s0;
        if (off >= len) return;                                      // alignment.go:199-201 (also: an empty node ends the path)
        for (uint32_t i = off; i < len; i++) {
            if (d == 8) { set |= l2_bloom_bits(code); return; }
            const uint8_t b = v->bases[s0 + i];
            if (b == 'N') {                                          // :212-216 the graph's wildcard
                for (uint32_t x = 0; x < 4; x++) rest(node, i + 1, d + 1, code | (x << (2 * d)));
                return;
            }
            if (code_of(b) < 0) return;                              // never equals a base of the read
            code |= (uint32_t)code_of(b) << (2 * d);
            d++;
        }
        rest_at_end(node, d, code);
    }
    // ... continuing inside the node at i (after a wildcard)
    void rest(uint32_t node, uint32_t i, uint32_t d, uint32_t code)
    {
        const uint32_t s0 = v->node_seq_off[node], len = v->node_seq_off[node + 1] - s0;
        if (i < len) { go(node, i, d, code); return; }
        rest_at_end(node, d, code);
    }
    void rest_at_end(uint32_t node, uint32_t d, uint32_t code)
    {
        if (d == 8) { set |= l2_bloom_bits(code); return; }
        const uint32_t e0 = v->node_edge_off[node], deg = v->node_edge_off[node + 1] - e0;
        if (!deg) { set = ~0ull; return; }                           // :229-236 a sink reports the traversal whatever the read goes on with
        for (uint32_t e = 0; e < deg; e++) go(v->edges[e0 + e], 0, d, code);
    }
};
// DeviceIndex::node_l2b: which 8-mers a DFS from (node, offset 0..10) can spell; on nt threads
inline std::vector<uint64_t> build_node_l2b(const groot_index_view *v, unsigned nt)
{
    std::vector<uint64_t> sets((size_t)v->n_nodes * 11, 0);
    nt = std::max(1u, nt);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&, t]() {
            for (uint32_t nd = t; nd < v->n_nodes; nd += nt) {
                const uint32_t len = v->node_seq_off[nd + 1] - v->node_seq_off[nd];
                for (uint32_t o = 0; o < std::min(len, 11u); o++) {
                    L2Walk w{v};
                    w.go(nd, o, 0, 0);
                    sets[(size_t)nd * 11 + o] = w.set;
                }
            }
        });
    for (auto &x : th) x.join();
    return sets;
}

// DeviceIndex::graph_win_end: one past the last window of every graph; empty when the windows are not numbered graph by graph (canonical seed order)
inline std::vector<uint32_t> build_graph_win_end(const groot_index_view *v)
{
    std::vector<uint32_t> end(v->n_graphs, 0);
    for (uint32_t w = 0; w < v->n_windows; w++) {
        if (w && v->win_graph[w] < v->win_graph[w - 1]) return {};
        end[v->win_graph[w]] = w + 1;
    }
    return end;
}
// ceil(paths / 8) per graph: BYTES of a traversal's compact path set (<= 88: path sets of up to 704 bits)
inline std::vector<uint8_t> build_graph_words(const groot_index_view *v)
{
    std::vector<uint8_t> gw(v->n_graphs, 1);
    for (uint32_t g = 0; g < v->n_graphs; g++) gw[g] = (uint8_t)std::max<uint32_t>(1, (v->graph_path_off[g + 1] - v->graph_path_off[g] + 7) / 8);
    return gw;
}

inline std::vector<WinRec> build_win_rec(const groot_index_view *v)
{
    std::vector<WinRec> wr(v->n_windows);
    for (uint32_t w = 0; w < v->n_windows; w++) {
        const uint32_t node = v->win_node[w];
        const uint32_t nlen = v->node_seq_off[node + 1] - v->node_seq_off[node];
        const uint64_t last = (uint64_t)v->win_offset[w] + v->win_merge_span[w] + v->window_size;
        wr[w] = WinRec{v->win_graph[w], node, v->win_offset[w], (uint32_t)std::min<uint64_t>(nlen, last + 1), v->win_cn_off[w],
                       v->win_cn_off[w + 1], v->node_seq_off[node], nlen};
    }
    return wr;
}

// exact-match table over the windows' whole sketches (DeviceIndex::exact, mask = tab.size() - 1), and per window the smallest window id with the same 64-bit sketch
struct ExactTable {
    std::vector<ExactEntry> tab;
    std::vector<uint32_t> sketch_class;
};
inline ExactTable build_exact_table(const groot_index_view *v)
{
    const uint32_t n = v->n_windows, s = v->sketch_size;
    uint32_t cap = 16;
    while (cap < 2 * (uint64_t)n) cap <<= 1;
    ExactTable t{std::vector<ExactEntry>(cap, ExactEntry{0, kEmpty}), std::vector<uint32_t>(n)};
    auto &tab = t.tab; auto &sketch_class = t.sketch_class;
    for (uint32_t w = 0; w < n; w++) {
        uint64_t h = GROOT_SKETCH_HASH_INIT;
        for (uint32_t i = 0; i < s; i++) h = sketch_hash_step(h, v->win_sketch[(size_t)w * s + i]);
        uint32_t slot = (uint32_t)h & (cap - 1);
        sketch_class[w] = w;
        for (; tab[slot].id != kEmpty; slot = (slot + 1) & (cap - 1))
            if (sketch_class[w] == w && tab[slot].tag == (uint32_t)(h >> 32) &&
                !memcmp(v->win_sketch + (size_t)tab[slot].id * s, v->win_sketch + (size_t)w * s, (size_t)s * 8))
                sketch_class[w] = sketch_class[tab[slot].id];
        tab[slot] = ExactEntry{(uint32_t)(h >> 32), w};
    }
    return t;
}

// LSH forest band tables: per band the low-32 hash values of its max_k slots, sorted; hash tables over the distinct K-prefixes of every
// band (the query finds the first matching row with one or two probes instead of a binary search of ~log2(n) dependent loads); the rows'
// 5-bit signatures; the runs of equal K-prefixes.  Host work only (sorts): start_lsh_tables sizes the tables and leaves `job` filling
// them, the bands dealt out over `workers` threads; join it before reading.
struct LshTables {
    std::vector<uint32_t> keys, ids, run;
    std::vector<ExactEntry> tab;
    std::vector<uint8_t> sig;
    uint32_t hash_bits = 0;            // DeviceIndex::band_hash_bits
    std::thread job;
    ~LshTables() { if (job.joinable()) job.join(); }
};
inline void start_lsh_tables(LshTables &lsh, const groot_index_view *v, uint32_t lmax, uint32_t workers)
{
    const uint32_t n = v->n_windows, s = v->sketch_size, mk = v->max_k;
    lsh.keys.assign((size_t)lmax * n * mk, 0); lsh.ids.assign((size_t)lmax * n, 0);
    uint32_t bits = 4;
    while ((1ull << bits) < 2 * (uint64_t)n) bits++;
    lsh.hash_bits = bits;
    const uint32_t cap = 1u << bits;
    lsh.tab.assign((size_t)lmax * mk * cap, ExactEntry{0, kEmpty});
    lsh.sig.assign((size_t)lmax * n * kRowBytes, 0);
    lsh.run.assign((size_t)lmax * mk * n, 0);
    const uint32_t sl = std::min<uint32_t>(s, kRowSlots);
    lsh.job = std::thread([&lsh, v, n, s, mk, lmax, bits, cap, sl, workers]() {
        auto &keys = lsh.keys; auto &ids = lsh.ids; auto &tab = lsh.tab; auto &sig = lsh.sig; auto &run = lsh.run;
        auto band = [&](uint32_t b) {                            // the bands are independent: one thread each
            std::vector<uint32_t> order(n);
            std::iota(order.begin(), order.end(), 0u);
            const uint64_t *sk = v->win_sketch;
            std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
                for (uint32_t j = 0; j < mk; j++) {
                    const uint32_t a = (uint32_t)sk[(size_t)x * s + b * mk + j], bb = (uint32_t)sk[(size_t)y * s + b * mk + j];
                    if (a != bb) return a < bb;
                }
                return x < y;
            });
            for (uint32_t e = 0; e < n; e++) {
                ids[(size_t)b * n + e] = order[e];
                for (uint32_t j = 0; j < mk; j++)
                    keys[((size_t)b * n + e) * mk + j] = (uint32_t)sk[(size_t)order[e] * s + b * mk + j];
            }
            for (uint32_t K = 1; K <= mk; K++) {
                ExactEntry *t = tab.data() + (((size_t)b * mk + (K - 1)) << bits);
                for (uint32_t e = 0; e < n; e++) {
                    const uint32_t *ke = &keys[((size_t)b * n + e) * mk];
                    if (e && std::equal(ke, ke + K, ke - mk)) continue;      // same prefix as the previous row
                    uint64_t h = GROOT_SKETCH_HASH_INIT;
                    for (uint32_t j = 0; j < K; j++) h = sketch_hash_step(h, ke[j]);
                    uint32_t slot = (uint32_t)h & (cap - 1);
                    while (t[slot].id != kEmpty) slot = (slot + 1) & (cap - 1);
                    t[slot] = ExactEntry{(uint32_t)(h >> 32), e};
                }
            }
            for (uint32_t e = 0; e < n; e++) {
                const uint64_t *ws = v->win_sketch + (size_t)ids[(size_t)b * n + e] * s;
                uint32_t row[4] = {0, 0, 0, 0};                 // 5 bits per slot, six slots to a dword (kernels_common.hpp row_same6)
                for (uint32_t i = 0; i < sl; i++) row[i / 6] |= sig5(ws[i]) << (5 * (i % 6));
                memcpy(&sig[((size_t)b * n + e) * kRowBytes], row, kRowBytes);
            }
            for (uint32_t K = 1; K <= mk; K++) {
                uint32_t *rn = run.data() + ((size_t)b * mk + (K - 1)) * n;
                for (uint32_t e = n; e-- > 0;) {             // backwards: length of the run of equal K-prefixes starting at e
                    const uint32_t *ke = &keys[((size_t)b * n + e) * mk];
                    rn[e] = (e + 1 < n && std::equal(ke, ke + K, ke + mk)) ? rn[e + 1] + 1 : 1;
                }
            }
        };
        std::atomic<uint32_t> next{0};
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < std::min(lmax, workers); t++)
            th.emplace_back([&]() { for (uint32_t b; (b = next.fetch_add(1)) < lmax;) band(b); });
        for (auto &x : th) x.join();
    });
}

// ---- sketch_sig_kernel's side of the index ----
// The bases every window was sketched from (step 1 of the signature index): WindowSize + MergeSpan of them along its first Ref path,
// starting at (Key.Node, Key.OffSet) -- WindowGraph walks a path through the graph's nodes in order (graph.go:243-262) and merges
// consecutive windows of equal sketch into the first one (:293-333).  Texts stop at a base other than ACGT.  text: per window a
// forward and a reverse-complement row of kTextMax bytes; tlen: bases of them (0: no text of at least WindowSize bases).  On nt threads.
struct WindowTexts {
    std::vector<uint8_t> text;
    std::vector<uint32_t> tlen;
};
inline WindowTexts build_window_texts(const groot_index_view *v, unsigned nt)
{
    const uint32_t n = v->n_windows, w = v->window_size;
    WindowTexts wt{std::vector<uint8_t>((size_t)n * 2 * kTextMax + 64, 0), std::vector<uint32_t>(n, 0)};
    auto &text = wt.text; auto &tlen = wt.tlen;
    nt = std::max(1u, nt);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&, t]() {
            for (uint32_t i = t; i < n; i += nt) {
                if (v->win_ref_off[i] == v->win_ref_off[i + 1]) continue;
                const uint32_t g = v->win_graph[i], p = v->win_ref[v->win_ref_off[i]];
                const uint32_t n1 = v->graph_node_off[g + 1];
                const uint32_t want = (uint32_t)std::min<uint64_t>(kTextMax, (uint64_t)w + v->win_merge_span[i]);
                uint8_t *fw = &text[(size_t)i * 2 * kTextMax], *rc = fw + kTextMax;
                uint32_t node = v->win_node[i], off = v->win_offset[i], got = 0;
                bool stop = false;
                for (; !stop && got < want && node < n1; node++, off = 0) {
                    if (!((v->node_mask[(size_t)node * v->path_words + (p >> 6)] >> (p & 63)) & 1ULL)) {
                        if (node == v->win_node[i]) stop = true;      // the window's own node is not on its path?
                        continue;
                    }
                    const uint32_t s0 = v->node_seq_off[node], nlen = v->node_seq_off[node + 1] - s0;
                    for (; off < nlen && got < want; off++) {
                        const uint8_t b = v->bases[s0 + off];
                        if (code_of(b) < 0) { stop = true; break; }
                        fw[got++] = b;
                    }
                }
                if (got < w) { memset(fw, 0, kTextMax); continue; }
                tlen[i] = got;
                for (uint32_t j = 0; j < got; j++) {
                    const uint8_t b = fw[got - 1 - j];
                    rc[j] = b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : 'A';
                }
            }
        });
    for (auto &x : th) x.join();
    return wt;
}

// DeviceIndex::win_nodes: min(255, contained nodes of the window)
inline std::vector<uint8_t> build_win_nodes(const groot_index_view *v)
{
    std::vector<uint8_t> nodes(v->n_windows);
    for (uint32_t i = 0; i < v->n_windows; i++) nodes[i] = (uint8_t)std::min<uint32_t>(255, v->win_cn_off[i + 1] - v->win_cn_off[i]);
    return nodes;
}

// Signature index (step 4): the windows grouped by the hash of their signature (kSigG slots of the sketch: sig_step -- the slots the
// kernel computes), a group's windows sorted by (sketch class, id); a directory over the distinct signatures (buckets of two, load <= 1/4:
// four dwords per bucket, mask = dir.size() / 4 - 1) says where each group starts.  verdict: DeviceIndex::sig_info, vstride words per text row.
struct SigTables {
    std::vector<SigEntry> ent;
    std::vector<uint32_t> dir;
};
inline SigTables build_sig_tables(const groot_index_view *v, const std::vector<uint32_t> &sketch_class, const std::vector<uint32_t> &tlen,
                                  const std::vector<uint8_t> &argmin, const std::vector<uint32_t> &verdict, const std::vector<uint8_t> &nodes, uint32_t vstride)
{
    const uint32_t n = v->n_windows, s = v->sketch_size, k = v->kmer_size;
    const uint32_t m5 = (uint32_t)(((uint64_t)k * GROOT_MULTI_SEED) & 31u);
    std::vector<uint64_t> key(n);
    for (uint32_t i = 0; i < n; i++) {
        uint64_t x = GROOT_SIG_HASH_INIT;
        x = sig_hash_step(x, sig_part(0, v->win_sketch[(size_t)i * s]));
        for (int j = 1; j < kSigG; j++) x = sig_hash_step(x, sig_part(j, v->win_sketch[(size_t)i * s + (uint32_t)(sig_step(j, (int)s, (int)m5) ^ (int)m5)]));
        key[i] = sig_hash_fin(x);
    }
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (key[a] != key[b]) return key[a] < key[b];
        if (sketch_class[a] != sketch_class[b]) return sketch_class[a] < sketch_class[b];
        return a < b;
    });
    SigTables t;
    auto &ent = t.ent; auto &dir = t.dir;
    ent.assign((size_t)n + 8, SigEntry{kEmpty, kEmpty, 0, 0, {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}}});
    uint32_t n_keys = 0;
    for (uint32_t i = 0; i < n;) {
        uint32_t j = i;
        while (j < n && key[order[j]] == key[order[i]]) j++;
        for (uint32_t x = i; x < j; x++) {
            const uint32_t w_ = order[x];
            SigEntry e{w_, sketch_class[w_], sig_text_pack(tlen[w_], argmin[2 * w_], argmin[2 * w_ + 1]) | kSigInline, (j - x) | ((uint32_t)nodes[w_] << 24), {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}}};
            for (uint32_t row = 0; row < 2; row++)
                for (uint32_t o = 0; o < 8 && o < vstride; o++) e.verdict[row][o] = (uint8_t)verdict[((size_t)w_ * 2 + row) * vstride + o];
            ent[x] = e;
        }
        n_keys++;
        i = j;
    }
    uint32_t cap = 16;
    while ((uint64_t)cap * 2 < 4 * (uint64_t)n_keys) cap <<= 1;
    dir.resize((size_t)cap * 4);
    for (size_t i = 0; i < (size_t)cap; i++) { dir[4 * i] = 0; dir[4 * i + 1] = kEmpty; dir[4 * i + 2] = 0; dir[4 * i + 3] = kEmpty; }
    for (uint32_t i = 0; i < n; i += ent[i].group & 0xFFFFFFu) {
        const uint64_t x = key[order[i]];
        for (uint32_t b = (uint32_t)x & (cap - 1);; b = (b + 1) & (cap - 1)) {
            uint32_t *q = &dir[(size_t)b * 4];
            if (q[1] == kEmpty) { q[0] = (uint32_t)(x >> 32); q[1] = i; break; }
            if (q[3] == kEmpty) { q[2] = (uint32_t)(x >> 32); q[3] = i; break; }
        }
    }
    return t;
}

// ---- strings at 2 bits per base (the memo of open.hip: outcome table, text table) ----
struct StringSet {                          // distinct strings at 2 bits per base, tw dwords each; open addressing over their hashes
    uint32_t tw = 0;
    std::vector<uint32_t> words;            // [n * tw]
    std::vector<uint32_t> slots;            // index + 1, 0 = free
    size_t n = 0;
    uint32_t mask = 0;
    void init(uint32_t tw_, size_t expect)
    {
        tw = tw_;
        uint32_t cap = 1024;
        while (cap < 2 * expect) cap <<= 1;
        slots.assign(cap, 0);
        mask = cap - 1;
        words.reserve(expect * tw);
    }
    static uint64_t hash(const uint32_t *w, uint32_t tw)
    {
        uint64_t h = GROOT_TEXT_HASH_INIT;
        for (uint32_t j = 0; j < tw; j++) h = text_hash_step(h, w[j]);
        return h;
    }
    // index of the string, inserting it if `insert`; -1 if absent
    long find(const uint32_t *w, bool insert)
    {
        const uint64_t h = hash(w, tw);
        for (uint32_t s = (uint32_t)(h ^ (h >> 32)) & mask;; s = (s + 1) & mask) {
            if (!slots[s]) {
                if (!insert) return -1;
                words.insert(words.end(), w, w + tw);
                slots[s] = (uint32_t)++n;
                return (long)n - 1;
            }
            if (!memcmp(&words[(size_t)(slots[s] - 1) * tw], w, (size_t)tw * 4)) return (long)slots[s] - 1;
        }
    }
};
// bases [i, i + len) of a sequence packed at 2 bits per base (16 per dword, trailing dwords zero-padded)
inline void pack_at(const std::vector<uint32_t> &packed, size_t i, uint32_t len, uint32_t tw, uint32_t *out)
{
    const size_t d = i >> 4;
    const uint32_t sh = 2 * (uint32_t)(i & 15);
    for (uint32_t j = 0; j < tw; j++) {
        const uint64_t two = (uint64_t)packed[d + j] | ((uint64_t)packed[d + j + 1] << 32);
        out[j] = (uint32_t)(two >> sh);
    }
    const uint32_t full = len >> 4, tail = len & 15;
    if (full < tw) out[full] &= tail ? (1u << (2 * tail)) - 1u : 0u;
    for (uint32_t j = full + 1; j < tw; j++) out[j] = 0;
}

} // namespace groot
