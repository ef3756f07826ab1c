// open_tables_check.cpp -- every builder of groot_amd/csrc/hip/index_tables.hpp (the device tables groot_hip_open uploads) as a stand-alone
// program on a CPU: built with the host library's sources under -fsanitize=address,undefined (tests/test_open_tables.py) it builds an
// index from each fixture given on the command line and two hand-made views (what the fixtures may lack: a node with an 'N', a node with
// five out-edges, an empty node, two neighbours with the same first base, a path that skips a node; the same graphs without windows),
// runs every builder on each, checks what can be checked without a device and prints one line per table:
//     <index>/<table>  <bytes>  <fnv1a-64 of the bytes>
// usage: open_tables_check test.gfa test2.gfa test-genes.msa cluster1.msa cluster2.msa ...      (exit 0: every check held)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../groot_amd/csrc/common/view_check.hpp"
#include "groot_host.h"
#include "index_tables.hpp"

using namespace groot;

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); failures++; } \
    } while (0)

template <class T> static void line(const std::string &index, const char *table, const std::vector<T> &t)
{
    unsigned long long h = 0xcbf29ce484222325ull;
    const unsigned char *b = reinterpret_cast<const unsigned char *>(t.data());
    const size_t bytes = t.size() * sizeof(T);
    for (size_t i = 0; i < bytes; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    printf("%s/%s  %zu  %016llx\n", index.c_str(), table, bytes, h);
}

static uint32_t get2(const std::vector<uint32_t> &words, size_t i) { return (words[i >> 4] >> (2 * (i & 15))) & 3u; }

// a path's text equals the concatenation of its nodes; every node with an entry points into such a text
static void check_path_tables(const groot_index_view *v, const PathTables &pt)
{
    for (uint32_t nd = 0; nd < v->n_nodes; nd++) {
        const uint4 a = pt.node[2 * (size_t)nd], b = pt.node[2 * (size_t)nd + 1];
        if (a.x == kEmpty) continue;
        CHECK(a.y < b.y && (size_t)a.w + b.y <= pt.nodes.size() && pt.nodes[a.w + a.y] == nd, "path_node[%u] does not point at the node", nd);
        size_t at = a.x;
        for (uint32_t i = a.y; i-- > 0;) at -= v->node_seq_off[pt.nodes[a.w + i] + 1] - v->node_seq_off[pt.nodes[a.w + i]];
        for (uint32_t i = 0; i < b.y; i++) {
            const uint32_t n = pt.nodes[a.w + i];
            for (uint32_t j = v->node_seq_off[n]; j < v->node_seq_off[n + 1]; j++, at++) {
                const int cd = code_of(v->bases[j]);
                CHECK(get2(pt.text, at) == (uint32_t)(cd < 0 ? 0 : cd), "path text of node %u differs from node %u at base %u", nd, n, j);
                CHECK((get2(pt.tag, at) & 1u) == (j == v->node_seq_off[n] ? 1u : 0u), "path tag of node %u: node start at base %u", nd, j);
            }
        }
        CHECK(at == a.z, "path text of node %u ends at %zu, not %u", nd, at, a.z);
    }
}

static void run(const std::string &name, const groot_index_view *v)
{
    const std::string why = check_index_view(v);
    CHECK(why.empty(), "%s: %s", name.c_str(), why.c_str());
    if (!why.empty()) return;
    const uint32_t n = v->n_windows, s = v->sketch_size, l_max = s / v->max_k, pw = round_pw(v->path_words);
    const unsigned nt = 3;
    CHECK(pw != 0, "%s: path_words %u", name.c_str(), v->path_words);
    line(name, "node_rec", build_node_records(v, pw));
    const std::vector<uint32_t> node_graph = build_node_graph(v);
    line(name, "node_graph", node_graph);
    for (uint32_t g = 0; g < v->n_graphs; g++)
        for (uint32_t nd = v->graph_node_off[g]; nd < v->graph_node_off[g + 1]; nd++) CHECK(node_graph[nd] == g, "node_graph[%u]", nd);
    {
        PathTables pt;
        const bool ok = build_path_tables(v, node_graph, pt);
        CHECK(ok, "%s: path tables refused", name.c_str());
        line(name, "path_node", pt.node); line(name, "path_text", pt.text); line(name, "path_tag", pt.tag);
        line(name, "path_nodes", pt.nodes); line(name, "path_tab", pt.tab);
        printf("%s/path_texts  %u of %u paths, %zu bases\n", name.c_str(), pt.n_text_paths, v->n_paths, pt.n_bases);
        if (ok) check_path_tables(v, pt);
    }
    {
        const LeanTables lt = build_lean_tables(v);
        line(name, "bases2", lt.bases2); line(name, "lean_nodes", lt.nodes); line(name, "lean_ext", lt.ext);
        line(name, "cn_pre2", lt.cn_pre2); line(name, "win_ok", lt.win_ok);
        for (uint64_t i = 0; i < v->n_bases; i++) {
            const int cd = code_of(v->bases[i]);
            CHECK(get2(lt.bases2, i) == (uint32_t)(cd < 0 ? 0 : cd), "%s: bases2 at base %llu", name.c_str(), (unsigned long long)i);
        }
    }
    line(name, "cn_pre", build_cn_pre(v));
    line(name, "node_l2b", build_node_l2b(v, nt));
    line(name, "graph_win_end", build_graph_win_end(v));
    line(name, "graph_words", build_graph_words(v));
    line(name, "win_rec", build_win_rec(v));
    const ExactTable ex = build_exact_table(v);
    line(name, "exact", ex.tab); line(name, "sketch_class", ex.sketch_class);
    for (uint32_t w = 0; w < n; w++) {                      // every window is found in the exact table
        uint64_t h = GROOT_SKETCH_HASH_INIT;
        for (uint32_t i = 0; i < s; i++) h = sketch_hash_step(h, v->win_sketch[(size_t)w * s + i]);
        const uint32_t mask = (uint32_t)ex.tab.size() - 1;
        bool found = false;
        for (uint32_t slot = (uint32_t)h & mask; ex.tab[slot].id != kEmpty && !found; slot = (slot + 1) & mask)
            found = ex.tab[slot].id == w && ex.tab[slot].tag == (uint32_t)(h >> 32);
        CHECK(found, "%s: window %u is not in the exact table", name.c_str(), w);
        CHECK(ex.sketch_class[w] <= w && !memcmp(v->win_sketch + (size_t)ex.sketch_class[w] * s, v->win_sketch + (size_t)w * s, (size_t)s * 8), "%s: sketch_class[%u]", name.c_str(), w);
    }
    {
        LshTables lsh;
        start_lsh_tables(lsh, v, l_max, 2);
        lsh.job.join();
        line(name, "band_keys", lsh.keys); line(name, "band_ids", lsh.ids); line(name, "band_hash", lsh.tab);
        line(name, "band_sig", lsh.sig); line(name, "band_run", lsh.run);
        printf("%s/band_hash_bits  %u\n", name.c_str(), lsh.hash_bits);
        const uint32_t mk = v->max_k;
        for (uint32_t b = 0; b < l_max; b++) {              // every band's ids: a permutation sorted by its keys
            std::vector<uint8_t> seen(n, 0);
            for (uint32_t e = 0; e < n; e++) {
                const uint32_t id = lsh.ids[(size_t)b * n + e];
                CHECK(id < n && !seen[id], "%s: band %u row %u: id %u", name.c_str(), b, e, id);
                if (id >= n) continue;
                seen[id] = 1;
                const uint32_t *ke = &lsh.keys[((size_t)b * n + e) * mk];
                for (uint32_t j = 0; j < mk; j++) CHECK(ke[j] == (uint32_t)v->win_sketch[(size_t)id * s + b * mk + j], "%s: band %u row %u key %u", name.c_str(), b, e, j);
                if (e) CHECK(!std::lexicographical_compare(ke, ke + mk, ke - mk, ke), "%s: band %u row %u sorts before row %u", name.c_str(), b, e, e - 1);
            }
        }
    }
    {
        const uint32_t max_q = 256 - v->kmer_size + 1;      // groot_params_default: max_read_len 256, containment threshold 0.99
        const QTables qt = build_q_tables(v, max_q, l_max, 0.99);
        line(name, "q_k", qt.k); line(name, "q_l", qt.l); line(name, "q_min_eq", qt.min_eq);
    }
    if (n && v->window_size <= kTextMax && v->window_size >= v->kmer_size) {
        const WindowTexts wt = build_window_texts(v, nt);
        line(name, "text", wt.text); line(name, "tlen", wt.tlen);
        const std::vector<uint8_t> nodes = build_win_nodes(v);
        line(name, "win_nodes", nodes);
        const uint32_t m5 = (uint32_t)(((uint64_t)v->kmer_size * GROOT_MULTI_SEED) & 31u);
        if (sig_step(kSigG - 1, (int)s, (int)m5) >= 0) {    // the sketch has the slots the signature wants
            // (argmin and the verdicts come from the device at open: none here, so `sig` is not what a ctx uploads; `sig_dir` is)
            const uint32_t vstride = kTextMax - v->window_size + 1;
            const std::vector<uint8_t> argmin((size_t)n * 2, 0);
            const std::vector<uint32_t> verdict((size_t)n * 2 * vstride + 16, 0);
            const SigTables sg = build_sig_tables(v, ex.sketch_class, wt.tlen, argmin, verdict, nodes, vstride);
            line(name, "sig", sg.ent); line(name, "sig_dir", sg.dir);
            uint32_t groups = 0;
            for (uint32_t i = 0; i < n; i += sg.ent[i].group & 0xFFFFFFu) groups++;
            uint32_t in_dir = 0;
            for (size_t b = 0; b < sg.dir.size() / 4; b++) in_dir += (sg.dir[4 * b + 1] != kEmpty) + (sg.dir[4 * b + 3] != kEmpty);
            CHECK(groups == in_dir, "%s: %u signature groups, %u directory entries", name.c_str(), groups, in_dir);
        }
    }
}

// ---- the hand-made views ----
struct Hand {
    std::vector<uint32_t> graph_node_off, graph_path_off, node_seg_id, node_seq_off, node_edge_off, node_np_off, edges, np_path, np_pos, path_len, path_name_off;
    std::vector<uint8_t> graph_masked, bases;
    std::vector<uint64_t> node_mask, win_sketch;
    std::string path_names;
    std::vector<uint32_t> win_graph, win_node, win_offset, win_merge_span, win_cn_off, cn_node, cn_count, win_ref_off, win_ref;
    groot_index_view view(bool windows) const
    {
        groot_index_view v{};
        v.kmer_size = 3; v.sketch_size = 16; v.window_size = 6; v.num_part = 1; v.max_k = 4; v.num_window_kmers = 4; v.path_words = 1;
        v.n_graphs = (uint32_t)graph_masked.size(); v.n_nodes = (uint32_t)node_seg_id.size(); v.n_edges = (uint32_t)edges.size();
        v.n_paths = (uint32_t)path_len.size(); v.n_bases = bases.size(); v.n_np = np_path.size(); v.n_name_bytes = path_names.size();
        v.graph_node_off = graph_node_off.data(); v.graph_path_off = graph_path_off.data(); v.graph_masked = graph_masked.data();
        v.node_seg_id = node_seg_id.data(); v.node_seq_off = node_seq_off.data(); v.node_edge_off = node_edge_off.data(); v.node_np_off = node_np_off.data();
        v.node_mask = node_mask.data(); v.bases = bases.data(); v.edges = edges.data(); v.np_path = np_path.data(); v.np_pos = np_pos.data();
        v.path_len = path_len.data(); v.path_name_off = path_name_off.data(); v.path_names = path_names.data();
        if (windows) {
            v.n_windows = (uint32_t)win_graph.size(); v.n_cn = cn_node.size(); v.n_wref = win_ref.size();
            v.win_graph = win_graph.data(); v.win_node = win_node.data(); v.win_offset = win_offset.data(); v.win_merge_span = win_merge_span.data();
            v.win_cn_off = win_cn_off.data(); v.cn_node = cn_node.data(); v.cn_count = cn_count.data(); v.win_ref_off = win_ref_off.data();
            v.win_ref = win_ref.data(); v.win_sketch = win_sketch.data();
        }
        return v;
    }
};

static Hand hand_made()
{
    // graph 0, nodes 0..6: node 0 has five out-edges, to 1 ("GANT": an 'N') and 2 ("GGCA": the same first base as 1), 3 (empty), 4, 5; all lead
    // to the sink 6.  Its paths: 0 = 0,2,6   1 = 0,4,6   2 = 0,1,6 (through the 'N')   3 = 0,6 (skips a node: positions 0 and 10, no edge).
    // graph 1, nodes 7, 8: one path.
    const char *seq[] = {"ACGTAC", "GANT", "GGCA", "", "TTACG", "CCATG", "ACGTTGCA", "ACGTACGTAC", "GGTTAACC"};
    const std::vector<std::vector<uint32_t>> out = {{1, 2, 3, 4, 5}, {6}, {6}, {6}, {6}, {6}, {}, {8}, {}};
    const std::vector<std::vector<std::pair<uint32_t, uint32_t>>> on = {      // per node: (local path, position)
        {{0, 0}, {1, 0}, {2, 0}, {3, 0}}, {{2, 6}}, {{0, 6}}, {}, {{1, 6}}, {}, {{0, 10}, {1, 11}, {2, 10}, {3, 10}}, {{0, 0}}, {{0, 10}}};
    Hand h;
    h.graph_node_off = {0, 7, 9}; h.graph_path_off = {0, 4, 5}; h.graph_masked = {0, 0};
    h.path_len = {18, 19, 18, 14, 18};
    h.path_names = "p0p1p2p3q0"; h.path_name_off = {0, 2, 4, 6, 8, 10};
    h.node_seq_off = {0}; h.node_edge_off = {0}; h.node_np_off = {0};
    for (uint32_t n = 0; n < 9; n++) {
        h.node_seg_id.push_back(n + 1);
        for (const char *p = seq[n]; *p; p++) h.bases.push_back((uint8_t)*p);
        h.node_seq_off.push_back((uint32_t)h.bases.size());
        for (uint32_t e : out[n]) h.edges.push_back(e);
        h.node_edge_off.push_back((uint32_t)h.edges.size());
        uint64_t mask = 0;
        for (auto &pp : on[n]) { h.np_path.push_back(pp.first); h.np_pos.push_back(pp.second); mask |= 1ull << pp.first; }
        h.node_np_off.push_back((uint32_t)h.np_path.size());
        h.node_mask.push_back(mask);
    }
    // windows in canonical order (graph, node, offset): {graph, node, offset, merge span, contained nodes, Ref}
    struct W { uint32_t g, node, off, span; std::vector<uint32_t> cn, ref; };
    const std::vector<W> ws = {{0, 0, 0, 0, {0}, {0, 1, 2, 3}}, {0, 0, 2, 2, {0, 2}, {0}}, {0, 1, 0, 0, {1, 6}, {2}}, {0, 4, 1, 0, {4, 6}, {1}},
                               {1, 7, 0, 3, {7}, {0}},          {1, 7, 4, 0, {7, 8}, {0}}};
    h.win_cn_off = {0}; h.win_ref_off = {0};
    uint64_t x = 0x243F6A8885A308D3ull;
    for (size_t i = 0; i < ws.size(); i++) {
        const W &w = ws[i];
        h.win_graph.push_back(w.g); h.win_node.push_back(w.node); h.win_offset.push_back(w.off); h.win_merge_span.push_back(w.span);
        for (uint32_t c : w.cn) { h.cn_node.push_back(c); h.cn_count.push_back(1); }
        h.win_cn_off.push_back((uint32_t)h.cn_node.size());
        for (uint32_t r : w.ref) h.win_ref.push_back(r);
        h.win_ref_off.push_back((uint32_t)h.win_ref.size());
        for (uint32_t j = 0; j < 16; j++) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            h.win_sketch.push_back(x ^ (x >> 29));
        }
    }
    // window 5: the sketch of window 4 (one sketch class); window 1: the first band of window 0 (a run of two equal prefixes)
    for (uint32_t j = 0; j < 16; j++) h.win_sketch[5 * 16 + j] = h.win_sketch[4 * 16 + j];
    for (uint32_t j = 0; j < 4; j++) h.win_sketch[1 * 16 + j] = h.win_sketch[0 * 16 + j];
    return h;
}

int main(int argc, char **argv)
{
    // the 32-bit guard on the 2-bit texts: the last size that fits, the first that does not, 2^32
    const uint64_t sizes[3] = {(1ull << 31) - 513, (1ull << 31) - 512, 1ull << 32};
    for (uint64_t n : sizes) printf("bit_addressable32  %llu  %d\n", (unsigned long long)n, (int)bit_addressable32(n));
    CHECK(bit_addressable32(sizes[0]) && !bit_addressable32(sizes[1]) && !bit_addressable32(sizes[2]), "bit_addressable32");

    struct Fixture { const char *name; bool gfa; uint32_t k, s, w; int first, count; };
    const Fixture fx[] = {{"test.gfa", true, 7, 10, 30, 1, 1}, {"test2.gfa", true, 7, 10, 30, 2, 1}, {"test-genes.msa", false, 51, 30, 100, 3, 1},
                          {"arg-annot.90[:24]", false, 31, 21, 100, 4, argc - 4}};
    if (argc < 5) { printf("usage: %s test.gfa test2.gfa test-genes.msa cluster*.msa...\n", argv[0]); return 2; }
    for (const Fixture &f : fx) {
        groot_index_params p;
        groot_index_params_default(&p);
        p.kmer_size = f.k; p.sketch_size = f.s; p.window_size = f.w; p.n_threads = 2;
        groot_index *idx = nullptr;
        const int rc = (f.gfa ? groot_index_build_gfa_files : groot_index_build_msa_files)(argv + f.first, (uint32_t)f.count, &p, &idx);
        if (rc) { printf("%s: error %d: %s\n", f.name, rc, groot_host_last_error()); return 1; }
        groot_index_view v;
        groot_index_get_view(idx, &v);
        run(f.name, &v);
        groot_index_free(idx);
    }
    const Hand h = hand_made();
    const groot_index_view hv = h.view(true), hv0 = h.view(false);
    run("hand-made", &hv);
    run("hand-made, no windows", &hv0);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
