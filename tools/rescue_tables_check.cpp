// rescue_tables_check.cpp -- build_rescue_tables of groot_amd/csrc/hip/index_tables.hpp (the tables groot_hip_rescue_enable uploads) as a
// stand-alone program on a CPU: built with the host library's sources under -fsanitize=address,undefined (tests/test_rescue_tables.py) it
// builds an index from each fixture given on the command line and one hand-made view (a path without a text, an 'N', a 16-mer in three
// paths, a path shorter than 16 bases), runs the builder on each and checks it against a restatement from the view alone: every path's
// text and 'N' tag, and for every 16-mer of every text that its probe finds exactly its occurrences, ascending by (path, offset) -- and
// that a 16-mer with an 'N', or one that occurs nowhere, finds none.  One line per index:
//     <index>/rescue  <text paths> of <paths> paths, <bases> bases, <occurrences> occurrences of <distinct> 16-mers, <slots> slots
// usage: rescue_tables_check test.gfa test2.gfa test-genes.msa cluster1.msa cluster2.msa ...      (exit 0: every check held)
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../groot_amd/csrc/common/view_check.hpp"
#include "groot_host.h"
#include "index_tables.hpp"

using namespace groot;

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond)) { if (failures < 20) { printf("FAILED %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } failures++; } \
    } while (0)

static uint32_t get2(const std::vector<uint32_t> &words, size_t i) { return (words[i >> 4] >> (2 * (i & 15))) & 3u; }

// the occurrences the table holds for key
static std::vector<uint2> probe(const RescueTables &rt, uint32_t key)
{
    const uint32_t mask = (uint32_t)rt.tab.size() - 1;
    for (uint32_t slot = rescue_hash(key) & mask; rt.tab[slot].z; slot = (slot + 1) & mask)
        if (rt.tab[slot].x == key) return std::vector<uint2>(rt.occ.begin() + rt.tab[slot].y, rt.occ.begin() + rt.tab[slot].y + rt.tab[slot].z);
    return {};
}

static void run(const std::string &name, const groot_index_view *v)
{
    const std::string why = check_index_view(v);
    CHECK(why.empty(), "%s: %s", name.c_str(), why.c_str());
    if (!why.empty()) return;
    RescueTables rt;
    CHECK(build_rescue_tables(v, rt), "%s: refused", name.c_str());
    CHECK(rt.path.size() == v->n_paths && rt.tab.size() >= 16 && !(rt.tab.size() & (rt.tab.size() - 1)) && rt.tab.size() >= 2 * rt.n_kmers, "%s: sizes", name.c_str());
    // the paths from the view alone: nodes by Position, spelled base by base
    const std::vector<uint32_t> g_of = build_node_graph(v);
    std::vector<std::map<uint32_t, uint32_t>> nodes(v->n_paths);
    for (uint32_t n = 0; n < v->n_nodes; n++)
        for (uint32_t i = v->node_np_off[n]; i < v->node_np_off[n + 1]; i++) {
            const uint32_t gp = v->graph_path_off[g_of[n]] + v->np_path[i];
            if (gp < v->n_paths) nodes[gp][v->np_pos[i]] = n;
        }
    std::map<uint32_t, std::vector<uint2>> want;      // 16-mer -> occurrences, in (path, offset) order
    size_t text_paths = 0, bases = 0, n_occ = 0, next = 0;
    for (uint32_t p = 0; p < v->n_paths; p++) {
        const uint4 pi = rt.path[p];
        if (pi.x == kEmpty) { CHECK(pi.y == 0, "%s: path %u", name.c_str(), p); continue; }
        text_paths++;
        CHECK(pi.x == next, "%s: the text of path %u starts at %u, the one before ended at %zu", name.c_str(), p, pi.x, next);
        std::string s;
        for (auto &kv : nodes[p]) s.append((const char *)v->bases + v->node_seq_off[kv.second], v->node_seq_off[kv.second + 1] - v->node_seq_off[kv.second]);
        CHECK(!nodes[p].empty() && pi.z == nodes[p].begin()->first, "%s: first Position of path %u", name.c_str(), p);
        CHECK(s.size() == v->path_len[p] && pi.y == s.size(), "%s: path %u spells %zu bases, path_len %u, table %u", name.c_str(), p, s.size(), v->path_len[p], pi.y);
        next = pi.x + s.size();
        bases += s.size();
        if ((size_t)pi.x + s.size() + 64 > rt.text.size() * 16) { CHECK(false, "%s: text of path %u runs past the array", name.c_str(), p); continue; }
        uint32_t clean = 0;
        for (size_t i = 0; i < s.size(); i++) {
            const int cd = code_of((uint8_t)s[i]);
            CHECK(get2(rt.text, pi.x + i) == (uint32_t)(cd < 0 ? 0 : cd) && get2(rt.tag, pi.x + i) == (cd < 0 ? 1u : 0u), "%s: path %u base %zu", name.c_str(), p, i);
            clean = cd < 0 ? 0 : clean + 1;
            if (i + 1 < kRescueAnchor) continue;
            uint32_t key = 0;
            for (uint32_t j = 0; j < kRescueAnchor; j++) key |= (uint32_t)std::max(code_of((uint8_t)s[i + 1 - kRescueAnchor + j]), 0) << (2 * j);
            if (clean >= kRescueAnchor) { want[key].push_back(make_uint2(p, (uint32_t)(pi.x + i + 1 - kRescueAnchor))); n_occ++; }
            else want[key];                               // (with an 'N': unless it occurs clean elsewhere, the table has nothing under its key)
        }
    }
    size_t distinct = 0;
    for (auto &kv : want) {
        const std::vector<uint2> got = probe(rt, kv.first);
        bool same = got.size() == kv.second.size();
        for (size_t i = 0; same && i < got.size(); i++) same = got[i].x == kv.second[i].x && got[i].y == kv.second[i].y;
        CHECK(same, "%s: 16-mer %08x: %zu occurrences in the table, %zu in the texts", name.c_str(), kv.first, got.size(), kv.second.size());
        distinct += !kv.second.empty();
    }
    uint64_t x = 0x243F6A8885A308D3ull;
    for (int i = 0; i < 1000; i++) {                      // keys that occur nowhere
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t key = (uint32_t)(x >> 32);
        if (!want.count(key)) CHECK(probe(rt, key).empty(), "%s: 16-mer %08x is in the table and in no text", name.c_str(), key);
    }
    size_t used = 0;
    for (const uint4 &e : rt.tab) used += e.z != 0;
    CHECK(text_paths == rt.n_text_paths && bases == rt.n_bases && distinct == rt.n_kmers && used == distinct && (n_occ == rt.occ.size() || (!n_occ && rt.occ.size() == 1)),
          "%s: totals", name.c_str());
    printf("%s/rescue  %zu of %u paths, %zu bases, %zu occurrences of %zu 16-mers, %zu slots\n", name.c_str(), text_paths, v->n_paths, bases, n_occ, distinct, rt.tab.size());
}

// ---- the hand-made view ----
struct Hand {
    std::vector<uint32_t> graph_node_off, graph_path_off, node_seg_id, node_seq_off, node_edge_off, node_np_off, edges, np_path, np_pos, path_len, path_name_off;
    std::vector<uint8_t> graph_masked, bases;
    std::vector<uint64_t> node_mask;
    std::string path_names;
    groot_index_view view() const
    {
        groot_index_view v{};
        v.kmer_size = 3; v.sketch_size = 16; v.window_size = 6; v.num_part = 1; v.max_k = 4; v.num_window_kmers = 4; v.path_words = 1;
        v.n_graphs = (uint32_t)graph_masked.size(); v.n_nodes = (uint32_t)node_seg_id.size(); v.n_edges = (uint32_t)edges.size();
        v.n_paths = (uint32_t)path_len.size(); v.n_bases = bases.size(); v.n_np = np_path.size(); v.n_name_bytes = path_names.size();
        v.graph_node_off = graph_node_off.data(); v.graph_path_off = graph_path_off.data(); v.graph_masked = graph_masked.data();
        v.node_seg_id = node_seg_id.data(); v.node_seq_off = node_seq_off.data(); v.node_edge_off = node_edge_off.data(); v.node_np_off = node_np_off.data();
        v.node_mask = node_mask.data(); v.bases = bases.data(); v.edges = edges.data(); v.np_path = np_path.data(); v.np_pos = np_pos.data();
        v.path_len = path_len.data(); v.path_name_off = path_name_off.data(); v.path_names = path_names.data();
        return v;
    }
};

static Hand hand_made()
{
    // graph 0: node 0 (28 bases) leads to 1 (28 bases, an 'N' at its base 22), 2 (20 bases) and 3 (empty), 3 leads to 2.  Paths: 0 = 0,1 (the 'N')
    // 1 = 0,2   2 = 0 alone   3 = 0,3,2 (an empty node: no text).  Node 0's thirteen 16-mers lie in three texts.
    // graph 1: node 4 alone, six bases: a text shorter than an anchor.
    const char *seq[] = {"ACGTACGTTGCAAGGCTTAACCGGATCA", "GATTACAGATTACAGGCCTTAANCCGTA", "TTGACCAGTCAGGCATCGAT", "ACGTAC", ""};
    // node order inside the view: graph 0 = nodes 0, 1, 2, 3 (the empty one), graph 1 = node 4
    const char *order[] = {seq[0], seq[1], seq[2], seq[4], seq[3]};
    const std::vector<std::vector<uint32_t>> out = {{1, 2, 3}, {}, {}, {2}, {}};
    const std::vector<std::vector<std::pair<uint32_t, uint32_t>>> on = {      // per node: (local path, position)
        {{0, 0}, {1, 0}, {2, 0}, {3, 0}}, {{0, 28}}, {{1, 28}, {3, 28}}, {{3, 28}}, {{0, 0}}};
    Hand h;
    h.graph_node_off = {0, 4, 5}; h.graph_path_off = {0, 4, 5}; h.graph_masked = {0, 0};
    h.path_len = {56, 48, 28, 48, 6};
    h.path_names = "p0p1p2p3q0"; h.path_name_off = {0, 2, 4, 6, 8, 10};
    h.node_seq_off = {0}; h.node_edge_off = {0}; h.node_np_off = {0};
    for (uint32_t n = 0; n < 5; n++) {
        h.node_seg_id.push_back(n + 1);
        for (const char *p = order[n]; *p; p++) h.bases.push_back((uint8_t)*p);
        h.node_seq_off.push_back((uint32_t)h.bases.size());
        for (uint32_t e : out[n]) h.edges.push_back(e);
        h.node_edge_off.push_back((uint32_t)h.edges.size());
        uint64_t mask = 0;
        for (auto &pp : on[n]) { h.np_path.push_back(pp.first); h.np_pos.push_back(pp.second); mask |= 1ull << pp.first; }
        h.node_np_off.push_back((uint32_t)h.np_path.size());
        h.node_mask.push_back(mask);
    }
    return h;
}

int main(int argc, char **argv)
{
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
    const groot_index_view hv = h.view();
    run("hand-made", &hv);
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
