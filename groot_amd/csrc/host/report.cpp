// report.cpp -- `groot report`: per-reference breadth of coverage from the BAM written by `groot align`
//
// Restates src/reporting/reporting.go:33-173 (BAMreader.Run) and :178-213 (cigarClean); cmd/report.go:104-129 for the
// cutoff handling.  It sits after the hot path (the BAM is the hot path's output) and is here so that the reference's
// own end-to-end assertion -- testing/run_travis_tests.sh:36-56, "(Bla)B-7 is the only ARG reported" -- can be run
// against this build.  Free choices of the reference fixed here: annotations are printed in BAM header order (the
// reference ranges over a Go map), and the read count is the number of records on that reference (the reference reads
// a loop variable shared between goroutines, reporting.go:149).
#include <zlib.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <atomic>
#include <map>
#include <string>
#include <thread>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "host_common.hpp"
#include "../common/rare_perm.hpp"

using namespace groot;

namespace {

// sequential reader of a BGZF stream (concatenated gzip members), file or stdin
struct BgzfIn {
    FILE *f = nullptr;
    bool own = false;
    std::vector<uint8_t> in, out;
    size_t out_pos = 0;
    bool eof = false;
    std::string err;

    bool open(const char *path)
    {
        if (!path) { f = stdin; return true; }
        f = fopen(path, "rb");
        own = true;
        return f != nullptr;
    }
    ~BgzfIn() { if (f && own) fclose(f); }

    bool next_block()
    {
        uint8_t hdr[18];
        const size_t got = fread(hdr, 1, 18, f);
        if (got == 0) { eof = true; return false; }
        if (got != 18 || hdr[0] != 0x1f || hdr[1] != 0x8b || hdr[2] != 8 || !(hdr[3] & 4)) { err = "not a BGZF block"; return false; }
        const unsigned xlen = hdr[10] | (hdr[11] << 8);
        // the BC subfield is the first (and in practice only) extra field of a BGZF writer
        if (xlen < 6 || hdr[12] != 'B' || hdr[13] != 'C') { err = "BGZF block without a BC field"; return false; }
        const unsigned bsize = (hdr[16] | (hdr[17] << 8)) + 1u;
        if (bsize < 18 + (xlen - 6) + 8) { err = "bad BGZF block size"; return false; }
        in.resize(bsize - 18);
        if (fread(in.data(), 1, in.size(), f) != in.size()) { err = "truncated BGZF block"; return false; }
        const size_t skip = xlen - 6;
        const size_t clen = in.size() - skip - 8;
        const uint8_t *tail = in.data() + in.size() - 8;
        const uint32_t isize = tail[4] | (tail[5] << 8) | (tail[6] << 16) | ((uint32_t)tail[7] << 24);
        out.resize(isize);
        out_pos = 0;
        if (isize == 0) return true;
        z_stream zs{};
        if (inflateInit2(&zs, -15) != Z_OK) { err = "zlib init failed"; return false; }
        zs.next_in = in.data() + skip; zs.avail_in = (uInt)clen;
        zs.next_out = out.data(); zs.avail_out = (uInt)isize;
        const int rc = inflate(&zs, Z_FINISH);
        inflateEnd(&zs);
        if (rc != Z_STREAM_END || zs.total_out != isize) { err = "corrupt BGZF block"; return false; }
        return true;
    }
    // false at a clean end of file before the first byte, or on error (err set)
    bool read(void *dst, size_t n, bool *clean_eof = nullptr)
    {
        uint8_t *d = (uint8_t *)dst;
        size_t done = 0;
        while (done < n) {
            if (out_pos == out.size()) {
                if (!next_block()) {
                    if (clean_eof) *clean_eof = eof && done == 0 && err.empty();
                    if (err.empty() && !(eof && done == 0)) err = "unexpected end of BAM";
                    return false;
                }
                continue;
            }
            const size_t take = std::min(n - done, out.size() - out_pos);
            memcpy(d + done, out.data() + out_pos, take);
            out_pos += take; done += take;
        }
        return true;
    }
};

uint32_t le32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }

// reporting.go:178-213.  Returns the run-length string and whether it holds "internal" uncovered stretches.
std::string cigar_clean(const std::vector<uint8_t> &covered, bool &internal_d)
{
    std::string cigar;
    internal_d = false;
    if (covered.empty()) return cigar;
    size_t counter = 1;
    uint8_t pre = covered[0];
    size_t runs[2] = {0, 0};   // [0] = "D", [1] = "M"
    const char sym[2] = {'D', 'M'};
    for (size_t i = 1; i < covered.size(); i++) {
        const uint8_t val = covered[i];
        if (i == covered.size() - 1) {
            if (val == pre) {
                counter++;
                cigar += std::to_string(counter) + sym[val];
                runs[val]++;
            } else {
                cigar += std::to_string(counter) + sym[pre] + "1" + sym[val];
                runs[val]++;                 // (the run before it is not counted: reporting.go:194-197)
            }
            break;
        }
        if (val == pre) counter++;
        else {
            runs[pre]++;
            cigar += std::to_string(counter) + sym[pre];
            pre = val;
            counter = 1;
        }
    }
    internal_d = !((runs[0] + runs[1] <= 2) || (runs[0] == 2 && runs[1] == 1));
    return cigar;
}

// cmd/report.go:95-97 and :119-122
int check_cutoff(double &cov_cutoff, int low_cov)
{
    if (cov_cutoff > 1.0) return set_error(GROOT_E_INVALID, "supplied coverage cutoff exceeds 1.0 (100%%): %g", cov_cutoff);
    if (low_cov) cov_cutoff = 0.97;
    return GROOT_OK;
}

// reporting.go:128-160: the lines of the report from per-reference record counts and pileups, in reference order.  covered(r, i) =
// base i of reference r has a non-zero pileup; has_pileup(r) = reference r got a pileup (of its length).  name_len NULL = C strings.
// reported: NULL, or set to 1 for every reference written.
template <class Covered, class HasPileup>
int write_report(uint32_t n_ref, const char *const *names, const uint32_t *name_len, const uint32_t *lens, const uint64_t *count,
                 Covered covered_at, HasPileup has_pileup, double cov_cutoff, int low_cov, const char *out_path, uint64_t *n_reported,
                 std::vector<uint8_t> *reported_refs = nullptr, bool emit = true)
{
    if (reported_refs) reported_refs->assign(n_ref, 0);
    FILE *out = !emit ? nullptr : out_path ? fopen(out_path, "w") : stdout;
    if (emit && !out) return set_error(GROOT_E_IO, "cannot create %s", out_path);
    uint64_t reported = 0;
    std::vector<uint8_t> cov;
    for (uint32_t r = 0; r < n_ref; r++) {
        if (!count[r] || !has_pileup(r)) continue;
        const size_t len = lens[r];
        size_t covered = 0;
        cov.resize(len);
        for (size_t i = 0; i < len; i++) { cov[i] = covered_at(r, i) ? 1 : 0; covered += cov[i]; }
        if ((double)covered / (double)len < cov_cutoff) continue;         // reporting.go:130-131
        bool internal_d = false;
        const std::string cigar = cigar_clean(cov, internal_d);
        if (internal_d && low_cov) continue;                               // reporting.go:151-153
        const char *name = names[r];
        size_t nl = name_len ? name_len[r] : strlen(name);
        if (nl && name[0] == '*') { name++; nl--; }                         // cluster representative marker (:135-137)
        if (out) fprintf(out, "%.*s\t%llu\t%u\t%s\n", (int)nl, name, (unsigned long long)count[r], lens[r], cigar.c_str());
        reported++;
        if (reported_refs) (*reported_refs)[r] = 1;
    }
    if (out && out_path) fclose(out); else if (out) fflush(out);
    if (n_reported) *n_reported = reported;
    return GROOT_OK;
}

// The shared-reads file: "nameA \t nameB \t n" for every pair (a, b), a <= b, of reported references with n != 0, ascending by (a, b),
// names as the report prints them.  pairs = (a, b, n) sorted by (a, b), a pair at most once.
struct SharedPair {
    uint32_t a, b;
    uint64_t n;
};

int write_shared(const char *const *names, const uint32_t *name_len, const std::vector<uint8_t> &reported, const std::vector<SharedPair> &pairs,
                 const char *out_path, uint64_t *n_lines)
{
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) return set_error(GROOT_E_IO, "cannot create %s", out_path);
    auto name = [&](uint32_t r, size_t &nl) {
        const char *nm = names[r];
        nl = name_len ? name_len[r] : strlen(nm);
        if (nl && nm[0] == '*') { nm++; nl--; }                             // as the report prints it
        return nm;
    };
    uint64_t lines = 0;
    for (const SharedPair &p : pairs) {
        if (!p.n || !reported[p.a] || !reported[p.b]) continue;
        size_t la, lb;
        const char *na = name(p.a, la), *nb = name(p.b, lb);
        fprintf(out, "%.*s\t%.*s\t%llu\n", (int)la, na, (int)lb, nb, (unsigned long long)p.n);
        lines++;
    }
    if (out_path) fclose(out); else fflush(out);
    if (n_lines) *n_lines = lines;
    return GROOT_OK;
}

} // namespace

// `groot report` on a BAM; with shared_out, also the shared-reads file: S(read) = the references with a counted record of that QNAME
// read_sets: instead of any output, the (read << 32 | reference) pairs of the counted records, sorted and unique, and the header's names
// recs (with read_sets): every counted record as (read, reference, Pos, last = min(Pos + reference bases of its CIGAR, length - 1)), in
// file order; lens_out: the header's lengths
static int report_bam(const char *bam_path, double cov_cutoff, int low_cov, const char *out_path, uint64_t *n_reported, const char *shared_out,
                      uint64_t *n_lines, std::vector<uint64_t> *read_sets = nullptr, std::vector<std::string> *names_out = nullptr,
                      std::vector<std::array<uint32_t, 4>> *recs = nullptr, std::vector<uint32_t> *lens_out = nullptr)
{
    if (int rc = check_cutoff(cov_cutoff, low_cov)) return rc;
    BgzfIn in;
    if (!in.open(bam_path)) return set_error(GROOT_E_IO, "could not open BAM file %s", bam_path);
    uint8_t b4[4];
    if (!in.read(b4, 4) || memcmp(b4, "BAM\1", 4) != 0) return set_error(GROOT_E_FORMAT, "could not read BAM file: %s", in.err.empty() ? "bad magic" : in.err.c_str());
    if (!in.read(b4, 4)) return set_error(GROOT_E_FORMAT, "could not read BAM file: %s", in.err.c_str());
    std::vector<uint8_t> skip(le32(b4));
    if (!skip.empty() && !in.read(skip.data(), skip.size())) return set_error(GROOT_E_FORMAT, "could not read BAM file: %s", in.err.c_str());
    if (!in.read(b4, 4)) return set_error(GROOT_E_FORMAT, "could not read BAM file: %s", in.err.c_str());
    const uint32_t n_ref = le32(b4);
    std::vector<std::string> names(n_ref);
    std::vector<uint32_t> lens(n_ref);
    for (uint32_t r = 0; r < n_ref; r++) {
        if (!in.read(b4, 4)) return set_error(GROOT_E_FORMAT, "could not read BAM file: %s", in.err.c_str());
        const uint32_t l_name = le32(b4);
        std::vector<char> nm(l_name);
        if (l_name == 0 || !in.read(nm.data(), l_name) || !in.read(b4, 4)) return set_error(GROOT_E_FORMAT, "could not read BAM file: %s", in.err.c_str());
        names[r].assign(nm.data(), l_name - 1);
        lens[r] = le32(b4);
    }
    // pileup per reference (reporting.go:100-127): every record covers [Start, Start+Len] INCLUSIVE, clipped to the last base
    std::vector<std::vector<uint32_t>> pileup(n_ref);
    std::vector<uint64_t> count(n_ref, 0);
    std::vector<uint8_t> rec;
    // shared reads: reads are numbered by QNAME in order of first appearance (the reference interleaves the records of several
    // reads, so adjacency does not delimit a read); every counted record adds (read, reference)
    const bool shared = shared_out != nullptr || read_sets != nullptr;
    std::unordered_map<std::string, uint32_t> read_of;
    std::vector<uint64_t> read_ref;
    std::string qname;
    for (;;) {
        bool clean = false;
        if (!in.read(b4, 4, &clean)) {
            if (clean) break;
            return set_error(GROOT_E_FORMAT, "error reading bam: %s", in.err.c_str());
        }
        const uint32_t bs = le32(b4);
        if (bs < 32) return set_error(GROOT_E_FORMAT, "error reading bam: record too short");
        rec.resize(bs);
        if (!in.read(rec.data(), bs)) return set_error(GROOT_E_FORMAT, "error reading bam: %s", in.err.c_str());
        const int32_t ref_id = (int32_t)le32(rec.data()), pos = (int32_t)le32(rec.data() + 4);
        const uint32_t l_read_name = rec[8];
        const uint32_t n_cigar = rec[12] | (rec[13] << 8), flag = rec[14] | (rec[15] << 8);
        if (flag == 4) continue;                                            // reporting.go:81-83
        if (ref_id < 0 || (uint32_t)ref_id >= n_ref || pos < 0) continue;   // no reference to add the record to
        if (32 + (uint64_t)l_read_name + 4ull * n_cigar > bs) return set_error(GROOT_E_FORMAT, "error reading bam: cigar past the record");
        uint64_t ref_len = 0;                                               // sam.Record.Len(): reference bases the CIGAR consumes
        for (uint32_t c = 0; c < n_cigar; c++) {
            const uint32_t op = le32(rec.data() + 32 + l_read_name + 4 * c);
            const uint32_t t = op & 15;
            if (t == 0 || t == 2 || t == 3 || t == 7 || t == 8) ref_len += op >> 4;   // M D N = X
        }
        auto &pl = pileup[ref_id];
        if (pl.empty()) pl.assign(lens[ref_id], 0);
        count[ref_id]++;
        if (shared) {
            qname.assign((const char *)rec.data() + 32, l_read_name ? l_read_name - 1 : 0);   // (NUL-terminated)
            const uint32_t rd = read_of.emplace(qname, (uint32_t)read_of.size()).first->second;
            read_ref.push_back((uint64_t)rd << 32 | (uint32_t)ref_id);
            if (recs && lens[ref_id]) {
                const uint64_t last = std::min<uint64_t>((uint64_t)pos + ref_len, (uint64_t)lens[ref_id] - 1);
                recs->push_back({rd, (uint32_t)ref_id, (uint32_t)pos, (uint32_t)last});
            }
        }
        if (pl.empty()) continue;
        uint64_t end = (uint64_t)pos + ref_len;
        if (end > pl.size() - 1) end = pl.size() - 1;
        for (uint64_t i = (uint64_t)pos; i <= end; i++) pl[i]++;
    }
    if (read_sets) {
        std::sort(read_ref.begin(), read_ref.end());
        read_ref.erase(std::unique(read_ref.begin(), read_ref.end()), read_ref.end());
        *read_sets = std::move(read_ref);
        *names_out = std::move(names);
        if (lens_out) *lens_out = std::move(lens);
        return GROOT_OK;
    }
    std::vector<const char *> name_ptr(n_ref);
    for (uint32_t r = 0; r < n_ref; r++) name_ptr[r] = names[r].c_str();
    std::vector<uint8_t> reported;
    if (int rc = write_report(n_ref, name_ptr.data(), nullptr, lens.data(), count.data(),
                              [&](uint32_t r, size_t i) { return pileup[r][i] != 0; }, [&](uint32_t r) { return !pileup[r].empty(); },
                              cov_cutoff, low_cov, out_path, n_reported, &reported))
        return rc;
    if (!shared) return GROOT_OK;
    // S(read) restricted to the reported references, then every pair of it counted once per read
    pileup.clear();
    read_ref.erase(std::remove_if(read_ref.begin(), read_ref.end(), [&](uint64_t x) { return !reported[(uint32_t)x]; }), read_ref.end());
    std::sort(read_ref.begin(), read_ref.end());
    read_ref.erase(std::unique(read_ref.begin(), read_ref.end()), read_ref.end());
    // counters: a dense triangle over the reported references (rank order = header order) up to 1 GiB of them, else a map
    std::vector<uint32_t> rank(n_ref, 0), ref_of;
    for (uint32_t r = 0; r < n_ref; r++)
        if (reported[r]) { rank[r] = (uint32_t)ref_of.size(); ref_of.push_back(r); }
    const uint64_t R = ref_of.size(), tri = R * (R + 1) / 2;
    const bool dense = tri <= (1ull << 27);
    std::vector<uint64_t> dcnt(dense ? tri : 0);
    std::map<std::pair<uint32_t, uint32_t>, uint64_t> mcnt;
    for (size_t i = 0; i < read_ref.size();) {
        size_t j = i;
        while (j < read_ref.size() && read_ref[j] >> 32 == read_ref[i] >> 32) j++;
        for (size_t x = i; x < j; x++)
            for (size_t y = x; y < j; y++) {
                const uint64_t a = rank[(uint32_t)read_ref[x]], b = rank[(uint32_t)read_ref[y]];
                if (dense) dcnt[a * R - a * (a - 1) / 2 + (b - a)]++;
                else mcnt[{(uint32_t)a, (uint32_t)b}]++;
            }
        i = j;
    }
    std::vector<SharedPair> pairs;
    if (dense) {
        uint64_t k = 0;
        for (uint64_t a = 0; a < R; a++)
            for (uint64_t b = a; b < R; b++, k++)
                if (dcnt[k]) pairs.push_back({ref_of[a], ref_of[b], dcnt[k]});
    } else
        for (const auto &kv : mcnt) pairs.push_back({ref_of[kv.first.first], ref_of[kv.first.second], kv.second});
    return write_shared(name_ptr.data(), nullptr, reported, pairs, shared_out, n_lines);
}

extern "C" int groot_host_report(const char *bam_path, double cov_cutoff, int low_cov, const char *out_path, uint64_t *n_reported)
{
    return report_bam(bam_path, cov_cutoff, low_cov, out_path, n_reported, nullptr, nullptr);
}

extern "C" int groot_host_report_shared(const char *bam_path, double cov_cutoff, int low_cov, const char *report_out, const char *shared_out,
                                        uint64_t *n_reported, uint64_t *n_lines)
{
    if (!shared_out) return set_error(GROOT_E_INVALID, "null argument");
    return report_bam(bam_path, cov_cutoff, low_cov, report_out, n_reported, shared_out, n_lines);
}

static int report_counts(const groot_index_view *ix, const uint64_t *records, const uint64_t *depth, double cov_cutoff, int low_cov,
                         const char *out_path, uint64_t *n_reported, std::vector<uint8_t> *reported, bool emit = true)
{
    if (!ix || (ix->n_paths && (!records || !depth))) return set_error(GROOT_E_INVALID, "null argument");
    if (int rc = check_cutoff(cov_cutoff, low_cov)) return rc;
    const uint32_t n = ix->n_paths;
    std::vector<uint64_t> base(n + 1, 0);
    for (uint32_t p = 0; p < n; p++) base[p + 1] = base[p] + ix->path_len[p];
    std::vector<const char *> name_ptr(n);
    std::vector<uint32_t> name_len(n);
    for (uint32_t p = 0; p < n; p++) {
        name_ptr[p] = ix->path_names + ix->path_name_off[p];
        name_len[p] = ix->path_name_off[p + 1] - ix->path_name_off[p];
    }
    // a reference with records has a pileup of its length (reporting.go:100-103); one of length 0 is not reported
    return write_report(n, name_ptr.data(), name_len.data(), ix->path_len, records,
                        [&](uint32_t p, size_t i) { return depth[base[p] + i] != 0; }, [&](uint32_t p) { return ix->path_len[p] != 0; },
                        cov_cutoff, low_cov, out_path, n_reported, reported, emit);
}

extern "C" int groot_host_report_coverage(const groot_index_view *ix, const uint64_t *records, const uint64_t *depth, double cov_cutoff,
                                          int low_cov, const char *out_path, uint64_t *n_reported)
{
    return report_counts(ix, records, depth, cov_cutoff, low_cov, out_path, n_reported, nullptr);
}

extern "C" int groot_host_shared_from_counts(const groot_index_view *ix, const uint64_t *records, const uint64_t *depth, double cov_cutoff,
                                             int low_cov, uint64_t n_pairs, const uint32_t *pa, const uint32_t *pb, const uint64_t *count,
                                             const char *out_path, uint64_t *n_lines)
{
    if (!ix || (n_pairs && (!pa || !pb || !count))) return set_error(GROOT_E_INVALID, "null argument");
    const uint32_t n = ix->n_paths;
    std::vector<SharedPair> pairs(n_pairs);
    for (uint64_t i = 0; i < n_pairs; i++) {
        if (pa[i] > pb[i] || pb[i] >= n) return set_error(GROOT_E_INVALID, "pair %llu = (%u, %u) is not a <= b < %u", (unsigned long long)i, pa[i], pb[i], n);
        pairs[i] = {pa[i], pb[i], count[i]};
    }
    // the reported set: the report's own tail, written nowhere
    std::vector<uint8_t> reported;
    if (int rc = report_counts(ix, records, depth, cov_cutoff, low_cov, nullptr, nullptr, &reported, false)) return rc;
    // in any order, a pair given more than once (the lists of several contexts) is summed
    std::sort(pairs.begin(), pairs.end(), [](const SharedPair &x, const SharedPair &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    size_t m = 0;
    for (size_t i = 0; i < pairs.size(); i++) {
        if (m && pairs[m - 1].a == pairs[i].a && pairs[m - 1].b == pairs[i].b) pairs[m - 1].n += pairs[i].n;
        else pairs[m++] = pairs[i];
    }
    pairs.resize(m);
    std::vector<const char *> name_ptr(n);
    std::vector<uint32_t> name_len(n);
    for (uint32_t p = 0; p < n; p++) {
        name_ptr[p] = ix->path_names + ix->path_name_off[p];
        name_len[p] = ix->path_name_off[p + 1] - ix->path_name_off[p];
    }
    return write_shared(name_ptr.data(), name_len.data(), reported, pairs, out_path, n_lines);
}

// ---- variants: what the rescued reads say differs from the index (groot_hip_rescue_export) ----------------------------------
extern "C" int groot_host_variants_write(const groot_index_view *ix, const uint64_t *rescued_depth, const uint64_t *alt, const uint64_t *exact_depth,
                                         uint64_t min_reads, double min_share, const char *out_path, uint64_t *n_lines)
{
    if (!ix || (ix->n_paths && (!rescued_depth || !alt || !exact_depth))) return set_error(GROOT_E_INVALID, "null argument");
    if (!(min_share >= 0.0 && min_share <= 1.0)) return set_error(GROOT_E_INVALID, "minimum share %g is not in [0, 1]", min_share);
    // the nodes of every path with a count, by global path
    std::vector<uint64_t> base(ix->n_paths + 1, 0);
    for (uint32_t p = 0; p < ix->n_paths; p++) base[p + 1] = base[p] + ix->path_len[p];
    std::vector<uint8_t> wanted(ix->n_paths, 0);
    for (uint32_t p = 0; p < ix->n_paths; p++)
        for (uint64_t i = 4 * base[p]; i < 4 * base[p + 1] && !wanted[p]; i++) wanted[p] = alt[i] != 0;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> on(ix->n_paths);      // (Position, node)
    for (uint32_t g = 0; g < ix->n_graphs; g++)
        for (uint32_t n = ix->graph_node_off[g]; n < ix->graph_node_off[g + 1]; n++)
            for (uint32_t i = ix->node_np_off[n]; i < ix->node_np_off[n + 1]; i++) {
                const uint64_t gp = (uint64_t)ix->graph_path_off[g] + ix->np_path[i];
                if (gp < ix->n_paths && wanted[gp]) on[gp].push_back({ix->np_pos[i], n});
            }
    // (a kept placement adds to the depth of every base it adds an alt to: tables that say otherwise are refused before anything is written)
    for (uint64_t i = 0; i < base[ix->n_paths]; i++)
        for (uint32_t b = 0; b < 4; b++)
            if (alt[4 * i + b] > rescued_depth[i] || rescued_depth[i] + exact_depth[i] < rescued_depth[i])
                return set_error(GROOT_E_INVALID, "base %llu of the tables: %llu alt read(s) at a rescued depth of %llu", (unsigned long long)i,
                                 (unsigned long long)alt[4 * i + b], (unsigned long long)rescued_depth[i]);
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) return set_error(GROOT_E_IO, "cannot create %s", out_path);
    uint64_t lines = 0;
    std::string ref;
    for (uint32_t p = 0; p < ix->n_paths; p++) {
        if (!wanted[p]) continue;
        const uint32_t len = ix->path_len[p];
        ref.assign(len, 'N');                                                      // the path's bases by path coordinate
        for (const auto &pn : on[p])
            for (uint32_t j = ix->node_seq_off[pn.second]; j < ix->node_seq_off[pn.second + 1]; j++) {
                const uint64_t y = (uint64_t)pn.first + (j - ix->node_seq_off[pn.second]);
                if (y < len) ref[y] = (char)ix->bases[j];
            }
        const char *nm = ix->path_names + ix->path_name_off[p];
        size_t nl = ix->path_name_off[p + 1] - ix->path_name_off[p];
        if (nl && nm[0] == '*') { nm++; nl--; }                                    // as the report prints it
        for (uint32_t y = 0; y < len; y++)
            for (uint32_t b = 0; b < 4; b++) {
                const uint64_t n = alt[4 * (base[p] + y) + b], rd = rescued_depth[base[p] + y], ed = exact_depth[base[p] + y];
                if (!n || n < min_reads) continue;
                const double share = (double)n / (double)(rd + ed);
                if (!(share >= min_share)) continue;
                fprintf(out, "%.*s\t%u\t%c\t%c\t%llu\t%llu\t%llu\t%.4f\n", (int)nl, nm, y + 1, ref[y], "ACGT"[b], (unsigned long long)n, (unsigned long long)rd,
                        (unsigned long long)ed, share);
                lines++;
            }
    }
    if (out_path) fclose(out); else fflush(out);
    if (n_lines) *n_lines = lines;
    return GROOT_OK;
}

// ---- indels: the gaps the gap-rescued reads show against the index (groot_hip_gap_export) -----------------------------------
extern "C" int groot_host_indels_write(const groot_index_view *ix, const groot_gap_event *events, uint64_t n_events, const uint64_t *gdepth,
                                       const uint64_t *rescued_depth, const uint64_t *exact_depth, uint64_t min_reads, double min_share,
                                       const char *out_path, uint64_t *n_lines)
{
    if (!ix || (n_events && !events) || (ix->n_paths && (!gdepth || !rescued_depth || !exact_depth))) return set_error(GROOT_E_INVALID, "null argument");
    if (!(min_share >= 0.0 && min_share <= 1.0)) return set_error(GROOT_E_INVALID, "minimum share %g is not in [0, 1]", min_share);
    std::vector<uint64_t> base(ix->n_paths + 1, 0);
    for (uint32_t p = 0; p < ix->n_paths; p++) base[p + 1] = base[p] + ix->path_len[p];
    std::vector<uint8_t> wanted(ix->n_paths, 0);
    for (uint64_t i = 0; i < n_events; i++) {
        const groot_gap_event &e = events[i];
        if (e.path >= ix->n_paths || e.type > GROOT_GAP_INS || e.len < 1 || e.len > 8 || (uint64_t)e.pos + (e.type == GROOT_GAP_DEL ? e.len : 0) >= ix->path_len[e.path] ||
            (e.type == GROOT_GAP_DEL ? e.seq != 0 : (e.seq >> (2 * e.len)) != 0))
            return set_error(GROOT_E_INVALID, "event %llu: path %u, pos %u, type %u, len %u, seq %u is none of the index", (unsigned long long)i, e.path, e.pos, e.type, e.len, e.seq);
        const uint64_t at = base[e.path] + e.pos;
        if (e.reads > gdepth[at] || gdepth[at] + rescued_depth[at] < gdepth[at] || gdepth[at] + rescued_depth[at] + exact_depth[at] < exact_depth[at])
            return set_error(GROOT_E_INVALID, "event %llu: %llu read(s) at a gap depth of %llu", (unsigned long long)i, (unsigned long long)e.reads, (unsigned long long)gdepth[at]);
        wanted[e.path] = 1;
    }
    std::vector<std::string> ref(ix->n_paths);                                         // the bases of every path with an event, by path coordinate
    for (uint32_t p = 0; p < ix->n_paths; p++)
        if (wanted[p]) ref[p].assign(ix->path_len[p], 'N');
    for (uint32_t g = 0; g < ix->n_graphs; g++)
        for (uint32_t n = ix->graph_node_off[g]; n < ix->graph_node_off[g + 1]; n++)
            for (uint32_t i = ix->node_np_off[n]; i < ix->node_np_off[n + 1]; i++) {
                const uint64_t gp = (uint64_t)ix->graph_path_off[g] + ix->np_path[i];
                if (gp >= ix->n_paths || !wanted[gp]) continue;
                for (uint32_t j = ix->node_seq_off[n]; j < ix->node_seq_off[n + 1]; j++) {
                    const uint64_t y = (uint64_t)ix->np_pos[i] + (j - ix->node_seq_off[n]);
                    if (y < ix->path_len[gp]) ref[gp][y] = (char)ix->bases[j];
                }
            }
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) return set_error(GROOT_E_IO, "cannot create %s", out_path);
    uint64_t lines = 0;
    for (uint64_t i = 0; i < n_events; i++) {
        const groot_gap_event &e = events[i];
        const uint64_t at = base[e.path] + e.pos, gd = gdepth[at], rd = rescued_depth[at], ed = exact_depth[at];
        if (!e.reads || e.reads < min_reads) continue;
        const double share = (double)e.reads / (double)(gd + rd + ed);
        if (!(share >= min_share)) continue;
        char seq[9] = {0};
        for (uint32_t j = 0; j < e.len; j++) seq[j] = e.type == GROOT_GAP_DEL ? ref[e.path][e.pos + 1 + j] : "ACGT"[(e.seq >> (2 * j)) & 3];
        const char *nm = ix->path_names + ix->path_name_off[e.path];
        size_t nl = ix->path_name_off[e.path + 1] - ix->path_name_off[e.path];
        if (nl && nm[0] == '*') { nm++; nl--; }                                        // as the report prints it
        fprintf(out, "%.*s\t%u\t%s\t%u\t%s\t%llu\t%llu\t%llu\t%llu\t%.4f\n", (int)nl, nm, e.pos + 1, e.type == GROOT_GAP_DEL ? "DEL" : "INS", (unsigned)e.len, seq,
                (unsigned long long)e.reads, (unsigned long long)gd, (unsigned long long)rd, (unsigned long long)ed, share);
        lines++;
    }
    if (out_path) fclose(out); else fflush(out);
    if (n_lines) *n_lines = lines;
    return GROOT_OK;
}

// ---- abundance: EM over equivalence classes ---------------------------------------------------------------------------------
// src/em/em.go NewEM / Run / Return (lines 29-158), restated in double precision without FMA contraction (the library is built
// without -march), over ECs in canonical order: the reference iterates a Go map, so its sums are not reproducible.
extern "C" int groot_host_em(uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint32_t min_iter,
                             uint32_t max_iter, double *alpha_out, uint32_t *iterations)
{
    if ((n_ec && (!off || !count)) || (n_paths && !alpha_out)) return set_error(GROOT_E_INVALID, "null argument");
    if (max_iter < min_iter)                                                                     // em.go:31-33
        return set_error(GROOT_E_INVALID, "number of EM iterations (%u) must be greater than minimum iterations (%u)", max_iter, min_iter);
    if (max_iter < 1) return set_error(GROOT_E_INVALID, "no EM iterations were ran");           // em.go:153-155
    for (uint64_t e = 0; e < n_ec; e++) {
        if (off[e + 1] < off[e] || (off[e + 1] > off[e] && !ids)) return set_error(GROOT_E_INVALID, "EC %llu: bad offsets", (unsigned long long)e);
        for (uint64_t i = off[e]; i < off[e + 1]; i++)
            if (ids[i] >= n_paths) return set_error(GROOT_E_INVALID, "EC %llu holds path %u of %u", (unsigned long long)e, ids[i], n_paths);
    }
    const double tolerance = std::nextafter(1.0, 2.0) - 1.0;
    const double alpha_limit = 1e-7, alpha_change = 1e-2, alpha_change_limit = 1e-2;
    std::vector<double> alpha(n_paths, 1.0 / (double)n_paths), next(n_paths, 0.0);
    bool final_round = false;
    uint32_t it = 0;
    for (it = 0; it < max_iter; it++) {
        for (uint64_t e = 0; e < n_ec; e++) {
            const double c = (double)count[e];
            if (c == 0) continue;
            double denom = 0.0;
            for (uint64_t i = off[e]; i < off[e + 1]; i++) denom += alpha[ids[i]];
            if (denom < tolerance) continue;
            const double norm = c / denom;
            for (uint64_t i = off[e]; i < off[e + 1]; i++) next[ids[i]] += alpha[ids[i]] * norm;
        }
        uint32_t changed = 0;
        for (uint32_t p = 0; p < n_paths; p++) {
            if (next[p] > alpha_change_limit && std::fabs(next[p] - alpha[p]) / next[p] > alpha_change) changed++;
            alpha[p] = next[p];
            next[p] = 0.0;
        }
        const bool stop = changed == 0 && it > min_iter;
        if (final_round) break;
        if (stop) {                        // one more round after this one, from alpha with its tiny values zeroed
            final_round = true;
            for (uint32_t p = 0; p < n_paths; p++)
                if (alpha[p] < alpha_limit / 10.0) alpha[p] = 0.0;
        }
    }
    std::copy(alpha.begin(), alpha.end(), alpha_out);
    if (iterations) *iterations = it;
    return GROOT_OK;
}

// ---- bootstrap over the ECs (groot_host.h: resampling by splitmix64, the EM above per replicate) ---------------------------
extern "C" int groot_host_em_bootstrap(uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint32_t n_boot,
                                       uint64_t seed, uint64_t n_draws, uint32_t min_iter, uint32_t max_iter, uint32_t threads, uint64_t *boot_count,
                                       double *alpha, uint32_t *iterations)
{
    if ((n_ec && (!off || !count)) || (n_paths && !alpha)) return set_error(GROOT_E_INVALID, "null argument");
    if (n_boot == 0) return set_error(GROOT_E_INVALID, "no bootstrap replicates");
    if (max_iter < min_iter)
        return set_error(GROOT_E_INVALID, "number of EM iterations (%u) must be greater than minimum iterations (%u)", max_iter, min_iter);
    if (max_iter < 1) return set_error(GROOT_E_INVALID, "no EM iterations were ran");
    std::vector<uint64_t> cum(n_ec + 1, 0);
    for (uint64_t e = 0; e < n_ec; e++) {
        if (off[e + 1] < off[e] || (off[e + 1] > off[e] && !ids)) return set_error(GROOT_E_INVALID, "EC %llu: bad offsets", (unsigned long long)e);
        for (uint64_t i = off[e]; i < off[e + 1]; i++)
            if (ids[i] >= n_paths) return set_error(GROOT_E_INVALID, "EC %llu holds path %u of %u", (unsigned long long)e, ids[i], n_paths);
        cum[e + 1] = cum[e] + count[e];
        if (cum[e + 1] < cum[e]) return set_error(GROOT_E_INVALID, "the EC counts sum to 2^64 or more");
    }
    const uint64_t total = cum[n_ec];
    if (n_ec && total == 0) return set_error(GROOT_E_INVALID, "bootstrap over ECs without reads");
    if (n_draws == 0) n_draws = total;
    std::atomic<uint32_t> next_b{0};
    std::atomic<int> failed{0};
    auto work = [&]() {
        std::vector<uint64_t> own(boot_count ? 0 : n_ec);
        for (uint32_t b; (b = next_b.fetch_add(1)) < n_boot;) {
            uint64_t *bc = boot_count ? boot_count + (size_t)b * n_ec : own.data();
            std::fill(bc, bc + n_ec, 0);
            const uint64_t base = (uint64_t)b * n_draws;
            for (uint64_t j = 0; n_ec && j < n_draws; j++) {
                uint64_t z = seed + (base + j + 1) * 0x9E3779B97F4A7C15ull;
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                z = z ^ (z >> 31);
                const uint64_t t = (uint64_t)(((unsigned __int128)z * total) >> 64);
                bc[(std::upper_bound(cum.begin(), cum.end(), t) - cum.begin()) - 1]++;     // cum[e] <= t < cum[e + 1]
            }
            if (groot_host_em(n_paths, n_ec, off, ids, bc, min_iter, max_iter, alpha + (size_t)b * n_paths, iterations ? iterations + b : nullptr))
                failed = 1;
        }
    };
    const uint32_t nt = std::max(1u, std::min(threads, n_boot));
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    if (failed) return set_error(GROOT_E_INVALID, "the EM of a bootstrap replicate failed");
    return GROOT_OK;
}

namespace {

using EcMap = std::map<std::vector<uint32_t>, uint64_t>;   // canonical order

// the bootstrap columns of the abundance file: n replicates, from ready-made alpha[n][n_paths] or computed here over `threads`
struct Boot {
    uint32_t n = 0;
    uint64_t seed = 1;
    const double *alpha = nullptr;
    uint32_t threads = 1;
};

// ECs in any order, IDs in any order, repeats summed -> the canonical map (IDs ascending and unique, empty and count-0 ECs dropped)
int canonical_ecs(uint32_t n, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, EcMap &m)
{
    std::vector<uint32_t> v;
    for (uint64_t e = 0; e < n_ec; e++) {
        if (off[e + 1] < off[e] || (off[e + 1] > off[e] && !ids)) return set_error(GROOT_E_INVALID, "EC %llu: bad offsets", (unsigned long long)e);
        v.assign(ids + off[e], ids + off[e + 1]);
        for (uint32_t p : v)
            if (p >= n) return set_error(GROOT_E_INVALID, "EC %llu holds path %u of %u", (unsigned long long)e, p, n);
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        if (!v.empty() && count[e]) m[v] += count[e];          // (the lists of several contexts: repeats summed)
    }
    return GROOT_OK;
}

// the abundance file of the ECs in m (paths [0, n_paths), names as the report prints them); with boot, its four columns more
int write_abundance(uint32_t n_paths, const char *const *names, const uint32_t *name_len, const EcMap &m, double min_reads, const char *out_path,
                    uint64_t *n_lines, uint32_t *iterations, const Boot *boot = nullptr)
{
    std::vector<uint64_t> off{0}, count;
    std::vector<uint32_t> ids;
    std::vector<uint64_t> reads(n_paths, 0);
    for (const auto &kv : m) {
        for (uint32_t p : kv.first) { ids.push_back(p); reads[p] += kv.second; }
        off.push_back(ids.size());
        count.push_back(kv.second);
    }
    std::vector<double> alpha(n_paths);
    uint32_t it = 0;
    if (int rc = groot_host_em(n_paths, m.size(), off.data(), ids.data(), count.data(), GROOT_EM_MIN_ITER, GROOT_EM_MAX_ITER, alpha.data(), &it)) return rc;
    if (iterations) *iterations = it;
    const uint32_t B = boot ? boot->n : 0;
    std::vector<double> own;
    const double *ba = B ? boot->alpha : nullptr;
    if (B && !ba && !m.empty()) {
        own.resize((size_t)B * n_paths);
        if (int rc = groot_host_em_bootstrap(n_paths, m.size(), off.data(), ids.data(), count.data(), B, boot->seed, 0, GROOT_EM_MIN_ITER, GROOT_EM_MAX_ITER,
                                             boot->threads, nullptr, own.data(), nullptr))
            return rc;
        ba = own.data();
    }
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) return set_error(GROOT_E_IO, "cannot create %s", out_path);
    double sum = 0.0;
    for (uint32_t p = 0; p < n_paths; p++) sum += alpha[p];
    uint64_t lines = 0;
    std::vector<double> x(B);
    for (uint32_t p = 0; p < n_paths && !m.empty(); p++) {
        if (!(alpha[p] >= min_reads)) continue;
        const char *nm = names[p];
        size_t nl = name_len ? name_len[p] : strlen(nm);
        if (nl && nm[0] == '*') { nm++; nl--; }
        fprintf(out, "%.*s\t%llu\t%.2f\t%.6f", (int)nl, nm, (unsigned long long)reads[p], alpha[p], sum > 0 ? alpha[p] / sum : 0.0);
        if (B) {
            // groot_host.h: mean and sd with the sums in replicate order, the interval from the sorted replicates
            double s = 0.0, s2 = 0.0;
            for (uint32_t b = 0; b < B; b++) { x[b] = ba[(size_t)b * n_paths + p]; s += x[b]; }
            const double mean = s / (double)B;
            for (uint32_t b = 0; b < B; b++) { const double d = x[b] - mean; s2 += d * d; }
            const double sd = B > 1 ? std::sqrt(s2 / (double)(B - 1)) : 0.0;
            std::sort(x.begin(), x.end());
            const uint32_t q = (uint32_t)((25ull * (B - 1)) / 1000);
            fprintf(out, "\t%.2f\t%.2f\t%.2f\t%.2f", mean, sd, x[q], x[B - 1 - q]);
        }
        fputc('\n', out);
        lines++;
    }
    if (out_path) fclose(out); else fflush(out);
    if (n_lines) *n_lines = lines;
    return GROOT_OK;
}

int abundance_from_ecs(const groot_index_view *ix, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, double min_reads,
                       const char *out_path, uint64_t *n_lines, uint32_t *iterations, const Boot *boot)
{
    if (!ix || (n_ec && (!off || !count))) return set_error(GROOT_E_INVALID, "null argument");
    const uint32_t n = ix->n_paths;
    EcMap m;
    if (int rc = canonical_ecs(n, n_ec, off, ids, count, m)) return rc;
    std::vector<const char *> name_ptr(n);
    std::vector<uint32_t> name_len(n);
    for (uint32_t p = 0; p < n; p++) {
        name_ptr[p] = ix->path_names + ix->path_name_off[p];
        name_len[p] = ix->path_name_off[p + 1] - ix->path_name_off[p];
    }
    return write_abundance(n, name_ptr.data(), name_len.data(), m, min_reads, out_path, n_lines, iterations, boot);
}

int report_abundance(const char *bam_path, double min_reads, const char *out_path, uint64_t *n_lines, const Boot *boot)
{
    std::vector<uint64_t> read_ref;
    std::vector<std::string> names;
    if (int rc = report_bam(bam_path, 0.97, 0, nullptr, nullptr, nullptr, nullptr, &read_ref, &names)) return rc;
    // S(read): the references of one QNAME's records (read_ref is sorted by read, then reference)
    EcMap m;
    std::vector<uint32_t> v;
    for (size_t i = 0; i < read_ref.size();) {
        size_t j = i;
        v.clear();
        while (j < read_ref.size() && read_ref[j] >> 32 == read_ref[i] >> 32) v.push_back((uint32_t)read_ref[j++]);
        m[v]++;
        i = j;
    }
    std::vector<const char *> name_ptr(names.size());
    for (size_t r = 0; r < names.size(); r++) name_ptr[r] = names[r].c_str();
    return write_abundance((uint32_t)names.size(), name_ptr.data(), nullptr, m, min_reads, out_path, n_lines, nullptr, boot);
}

} // namespace

extern "C" int groot_host_ecs_canonical(uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint64_t *out_off,
                                        uint32_t *out_ids, uint64_t *out_count, uint64_t *n_out)
{
    if ((n_ec && (!off || !count || !out_count)) || !out_off || !n_out) return set_error(GROOT_E_INVALID, "null argument");
    EcMap m;
    if (int rc = canonical_ecs(n_paths, n_ec, off, ids, count, m)) return rc;
    uint64_t e = 0, at = 0;
    out_off[0] = 0;
    for (const auto &kv : m) {
        for (uint32_t p : kv.first) out_ids[at++] = p;
        out_count[e] = kv.second;
        out_off[++e] = at;
    }
    *n_out = e;
    return GROOT_OK;
}

extern "C" int groot_host_abundance_from_ecs(const groot_index_view *ix, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                                             double min_reads, const char *out_path, uint64_t *n_lines, uint32_t *iterations)
{
    return abundance_from_ecs(ix, n_ec, off, ids, count, min_reads, out_path, n_lines, iterations, nullptr);
}

extern "C" int groot_host_abundance_boot_from_ecs(const groot_index_view *ix, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                                                  double min_reads, uint32_t n_boot, uint64_t seed, const double *boot_alpha, uint32_t threads,
                                                  const char *out_path, uint64_t *n_lines, uint32_t *iterations)
{
    if (n_boot == 0) return set_error(GROOT_E_INVALID, "no bootstrap replicates");
    const Boot boot{n_boot, seed, boot_alpha, threads};
    return abundance_from_ecs(ix, n_ec, off, ids, count, min_reads, out_path, n_lines, iterations, &boot);
}

extern "C" int groot_host_report_abundance(const char *bam_path, double min_reads, const char *out_path, uint64_t *n_lines)
{
    return report_abundance(bam_path, min_reads, out_path, n_lines, nullptr);
}

extern "C" int groot_host_report_abundance_boot(const char *bam_path, double min_reads, uint32_t n_boot, uint64_t seed, uint32_t threads,
                                                const char *out_path, uint64_t *n_lines)
{
    if (n_boot == 0) return set_error(GROOT_E_INVALID, "no bootstrap replicates");
    const Boot boot{n_boot, seed, nullptr, threads};
    return report_abundance(bam_path, min_reads, out_path, n_lines, &boot);
}

// ---- calls: the EM-weighted pileup per path (groot_host.h "assigned coverage") ------------------------------------------------
namespace {

struct Tuple {
    uint32_t ec, path, pos, last;
    uint64_t n;
};
bool tuple_less(const Tuple &a, const Tuple &b) { return std::tie(a.ec, a.path, a.pos, a.last) < std::tie(b.ec, b.path, b.pos, b.last); }

// equal keys summed, ascending
void tuples_canonical(std::vector<Tuple> &t)
{
    std::sort(t.begin(), t.end(), tuple_less);
    size_t w = 0;
    for (size_t i = 0; i < t.size(); i++) {
        if (!t[i].n) continue;
        if (w && !tuple_less(t[w - 1], t[i])) t[w - 1].n += t[i].n;
        else t[w++] = t[i];
    }
    t.resize(w);
}

// the table checked and ordered by (path, EC, Pos, last): EC indices inside the list, the path an ID of its EC and inside the index
int tuples_by_path(uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn,
                   std::vector<Tuple> &out)
{
    out.clear();
    out.reserve(n_tuples);
    for (uint64_t i = 0; i < n_tuples; i++) {
        const Tuple t{tuples[4 * i], tuples[4 * i + 1], tuples[4 * i + 2], tuples[4 * i + 3], tn[i]};
        if (t.ec >= n_ec) return set_error(GROOT_E_INVALID, "tuple %llu names EC %u of %llu", (unsigned long long)i, t.ec, (unsigned long long)n_ec);
        if (t.path >= n_paths || !std::binary_search(ids + off[t.ec], ids + off[t.ec + 1], t.path))
            return set_error(GROOT_E_INVALID, "tuple %llu: path %u is not in EC %u", (unsigned long long)i, t.path, t.ec);
        out.push_back(t);
    }
    std::sort(out.begin(), out.end(), [](const Tuple &a, const Tuple &b) { return std::tie(a.path, a.ec, a.pos, a.last) < std::tie(b.path, b.ec, b.pos, b.last); });
    return GROOT_OK;
}

// w(e, p): alpha[p] over the sum of alpha over e in ID order, 0.0 where the EM skips e
double weight_of(const uint64_t *off, const uint32_t *ids, const double *alpha, uint32_t e, uint32_t p)
{
    const double tolerance = std::nextafter(1.0, 2.0) - 1.0;
    double denom = 0.0;
    for (uint64_t i = off[e]; i < off[e + 1]; i++) denom += alpha[ids[i]];
    if (denom < tolerance) return 0.0;
    return alpha[p] / denom;
}

// D_p of the tuples [lo, hi) of one path of length len (ordered by EC): per EC an integer difference array, then the weighted sum in
// EC order, the weight of the group that starts at tuple i being weight(i)
template <class W> void depth_weighted(const std::vector<Tuple> &t, size_t lo, size_t hi, uint32_t len, std::vector<double> &D, std::vector<int64_t> &diff, W weight)
{
    D.assign(len, 0.0);
    for (size_t i = lo; i < hi;) {
        size_t j = i;
        diff.assign((size_t)len + 1, 0);
        for (; j < hi && t[j].ec == t[i].ec; j++) {
            if (t[j].pos >= len || t[j].last < t[j].pos) continue;           // (a record past its path covers nothing)
            diff[t[j].pos] += (int64_t)t[j].n;
            diff[std::min<uint64_t>((uint64_t)t[j].last, (uint64_t)len - 1) + 1] -= (int64_t)t[j].n;
        }
        const double w = weight(i);
        int64_t d = 0;
        for (uint32_t x = 0; x < len; x++) {
            d += diff[x];
            const double term = (double)d * w;
            D[x] = D[x] + term;
        }
        i = j;
    }
}

// D_p with the point estimate's weights w(e, p)
void depth_of(const std::vector<Tuple> &t, size_t lo, size_t hi, const uint64_t *off, const uint32_t *ids, const double *alpha, uint32_t p, uint32_t len,
              std::vector<double> &D, std::vector<int64_t> &diff)
{
    depth_weighted(t, lo, hi, len, D, diff, [&](size_t i) { return weight_of(off, ids, alpha, t[i].ec, p); });
}

// groot_host_call_support (groot_host.h "bootstrap support for the calls"): covered_b[p] of every replicate and selected path
int call_support(uint32_t n_paths, const uint32_t *lens, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint64_t n_tuples,
                 const uint32_t *tuples, const uint64_t *tn, uint32_t n_boot, const uint64_t *boot_count, const double *boot_alpha, double call_depth,
                 uint32_t n_sel, const uint32_t *sel, uint32_t threads, uint32_t *covered)
{
    if ((n_paths && !lens) || (n_ec && (!off || !count || !boot_count)) || (n_paths && !boot_alpha) || (n_tuples && (!tuples || !tn)) ||
        (n_sel && (!sel || !covered)))
        return set_error(GROOT_E_INVALID, "null argument");
    if (n_boot == 0) return set_error(GROOT_E_INVALID, "no bootstrap replicates");
    for (uint64_t e = 0; e < n_ec; e++) {
        if (off[e + 1] < off[e] || (off[e + 1] > off[e] && !ids)) return set_error(GROOT_E_INVALID, "EC %llu: bad offsets", (unsigned long long)e);
        if (count[e] == 0) return set_error(GROOT_E_INVALID, "EC %llu has no reads", (unsigned long long)e);
        for (uint64_t i = off[e]; i < off[e + 1]; i++)
            if (ids[i] >= n_paths || (i > off[e] && ids[i] <= ids[i - 1])) return set_error(GROOT_E_INVALID, "EC %llu: its IDs do not ascend inside the index", (unsigned long long)e);
    }
    for (uint32_t s = 0; s < n_sel; s++)
        if (sel[s] >= n_paths) return set_error(GROOT_E_INVALID, "selected path %u of %u", sel[s], n_paths);
    std::vector<Tuple> t;
    if (int rc = tuples_by_path(n_paths, n_ec, off, ids, n_tuples, tuples, tn, t)) return rc;
    // per tuple the listed-ID index of its (EC, path); per path its range of tuples
    std::vector<uint64_t> listed(t.size());
    std::vector<size_t> first((size_t)n_paths + 1, 0);
    for (size_t i = 0; i < t.size(); i++) {
        if (t[i].last >= lens[t[i].path])
            return set_error(GROOT_E_INVALID, "a tuple of path %u ends at %u, the path has %u bases", t[i].path, t[i].last, lens[t[i].path]);
        listed[i] = (uint64_t)(std::lower_bound(ids + off[t[i].ec], ids + off[t[i].ec + 1], t[i].path) - ids);
        first[(size_t)t[i].path + 1]++;
    }
    for (uint32_t p = 0; p < n_paths; p++) first[p + 1] += first[p];
    const uint64_t n_listed = n_ec ? off[n_ec] : 0;
    const double tolerance = std::nextafter(1.0, 2.0) - 1.0;
    std::atomic<uint32_t> next_b{0};
    auto work = [&]() {
        std::vector<double> f(n_listed), D;
        std::vector<int64_t> diff;
        for (uint32_t b; (b = next_b.fetch_add(1)) < n_boot;) {
            const uint64_t *bc = boot_count + (size_t)b * n_ec;
            const double *alpha = boot_alpha + (size_t)b * n_paths;
            for (uint64_t e = 0; e < n_ec; e++) {
                double denom = 0.0;
                for (uint64_t i = off[e]; i < off[e + 1]; i++) denom = denom + alpha[ids[i]];
                const bool skip = bc[e] == 0 || denom < tolerance;
                const double s = (double)bc[e] / (double)count[e];
                for (uint64_t i = off[e]; i < off[e + 1]; i++) {
                    const double w = skip ? 0.0 : alpha[ids[i]] / denom;
                    f[i] = s * w;
                }
            }
            for (uint32_t k = 0; k < n_sel; k++) {
                const uint32_t p = sel[k], len = lens[p];
                depth_weighted(t, first[p], first[(size_t)p + 1], len, D, diff, [&](size_t i) { return f[listed[i]]; });
                uint32_t c = 0;
                for (uint32_t x = 0; x < len; x++) c += D[x] >= call_depth ? 1u : 0u;
                covered[(size_t)b * n_sel + k] = c;
            }
        }
    };
    const uint32_t nt = std::max(1u, std::min(threads, n_boot));
    std::vector<std::thread> pool;
    for (uint32_t i = 1; i < nt; i++) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    return GROOT_OK;
}

// the three support columns of the calls file: n replicates; boot_count[n][n_ec] and boot_alpha[n][n_paths] (used when both are given),
// covered[n][lines]; whatever is NULL is computed here on `threads` host threads
struct Support {
    uint32_t n = 0;
    uint64_t seed = 1;
    uint32_t threads = 1;
    const uint64_t *boot_count = nullptr;
    const double *boot_alpha = nullptr;
    const uint32_t *covered = nullptr;
};

// the calls file: a line per line of the abundance file (alpha >= min_reads, header order)
int write_calls(uint32_t n_paths, const char *const *names, const uint32_t *name_len, const uint32_t *lens, uint64_t n_ec, const uint64_t *off, const uint32_t *ids,
                const uint64_t *count, const double *alpha_in, uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn, double min_reads, double call_depth,
                double cov_cutoff, const char *out_path, uint64_t *n_lines, uint64_t *n_called, const Support *sup = nullptr)
{
    if ((n_ec && (!off || !count)) || (n_tuples && (!tuples || !tn))) return set_error(GROOT_E_INVALID, "null argument");
    if (sup && sup->n == 0) return set_error(GROOT_E_INVALID, "no bootstrap replicates");
    if (cov_cutoff > 1.0) return set_error(GROOT_E_INVALID, "supplied coverage cutoff exceeds 1.0 (100%%): %g", cov_cutoff);
    for (uint64_t e = 0; e < n_ec; e++) {
        if (off[e + 1] < off[e] || (off[e + 1] > off[e] && !ids)) return set_error(GROOT_E_INVALID, "EC %llu: bad offsets", (unsigned long long)e);
        for (uint64_t i = off[e]; i < off[e + 1]; i++)
            if (ids[i] >= n_paths || (i > off[e] && ids[i] <= ids[i - 1])) return set_error(GROOT_E_INVALID, "EC %llu: its IDs do not ascend inside the index", (unsigned long long)e);
    }
    std::vector<double> own;
    const double *alpha = alpha_in;
    if (!alpha) {
        own.resize(n_paths);
        if (int rc = groot_host_em(n_paths, n_ec, off, ids, count, GROOT_EM_MIN_ITER, GROOT_EM_MAX_ITER, own.data(), nullptr)) return rc;
        alpha = own.data();
    }
    std::vector<Tuple> t;
    if (int rc = tuples_by_path(n_paths, n_ec, off, ids, n_tuples, tuples, tn, t)) return rc;
    // with sup: covered[B][lines] of the replicates, over the paths that get a line
    const uint32_t B = sup && n_ec ? sup->n : 0;
    std::vector<uint32_t> sel, own_cov, v(B);
    const uint32_t *cov_b = B ? sup->covered : nullptr;
    if (B) {
        for (uint32_t p = 0; p < n_paths; p++)
            if (alpha[p] >= min_reads) sel.push_back(p);
        if (!cov_b) {
            std::vector<uint64_t> own_bc;
            std::vector<double> own_ba;
            const uint64_t *bc = sup->boot_count;
            const double *ba = sup->boot_alpha;
            if (!bc || !ba) {
                own_bc.resize((size_t)B * n_ec);
                own_ba.resize((size_t)B * n_paths);
                if (int rc = groot_host_em_bootstrap(n_paths, n_ec, off, ids, count, B, sup->seed, 0, GROOT_EM_MIN_ITER, GROOT_EM_MAX_ITER, sup->threads,
                                                     own_bc.data(), own_ba.data(), nullptr))
                    return rc;
                bc = own_bc.data(); ba = own_ba.data();
            }
            own_cov.resize((size_t)B * sel.size());
            if (int rc = call_support(n_paths, lens, n_ec, off, ids, count, n_tuples, tuples, tn, B, bc, ba, call_depth, (uint32_t)sel.size(), sel.data(),
                                      sup->threads, own_cov.data()))
                return rc;
            cov_b = own_cov.data();
        }
    }
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) return set_error(GROOT_E_IO, "cannot create %s", out_path);
    uint64_t lines = 0, called = 0;
    std::vector<double> D;
    std::vector<int64_t> diff;
    std::vector<uint8_t> cov;
    size_t at = 0;
    for (uint32_t p = 0; p < n_paths && n_ec; p++) {
        while (at < t.size() && t[at].path < p) at++;
        size_t hi = at;
        while (hi < t.size() && t[hi].path == p) hi++;
        if (!(alpha[p] >= min_reads)) { at = hi; continue; }
        const uint32_t len = lens[p];
        depth_of(t, at, hi, off, ids, alpha, p, len, D, diff);
        at = hi;
        cov.resize(len);
        size_t covered = 0;
        double sum = 0.0;
        for (uint32_t x = 0; x < len; x++) {
            cov[x] = D[x] >= call_depth ? 1 : 0;
            covered += cov[x];
            sum += D[x];
        }
        const double breadth = len ? (double)covered / (double)len : 0.0, depth = len ? sum / (double)len : 0.0;
        bool internal_d = false;
        const std::string cigar = cigar_clean(cov, internal_d);
        const int is_called = breadth >= cov_cutoff ? 1 : 0;
        const char *nm = names[p];
        size_t nl = name_len ? name_len[p] : strlen(nm);
        if (nl && nm[0] == '*') { nm++; nl--; }
        fprintf(out, "%.*s\t%.2f\t%u\t%.2f\t%.4f\t%s\t%d", (int)nl, nm, alpha[p], len, depth, breadth, cigar.c_str(), is_called);
        if (B) {
            // groot_host.h: support = the share of replicates that call p, the interval from the sorted covered counts
            uint32_t yes = 0;
            for (uint32_t b = 0; b < B; b++) {
                v[b] = cov_b[(size_t)b * sel.size() + lines];
                const double breadth_b = len ? (double)v[b] / (double)len : 0.0;
                yes += breadth_b >= cov_cutoff ? 1u : 0u;
            }
            std::sort(v.begin(), v.end());
            const uint32_t q = (uint32_t)((25ull * (B - 1)) / 1000);
            fprintf(out, "\t%.3f\t%.4f\t%.4f", (double)yes / (double)B, len ? (double)v[q] / (double)len : 0.0, len ? (double)v[B - 1 - q] / (double)len : 0.0);
        }
        fputc('\n', out);
        lines++;
        called += is_called;
    }
    if (out_path) fclose(out); else fflush(out);
    if (n_lines) *n_lines = lines;
    if (n_called) *n_called = called;
    return GROOT_OK;
}

} // namespace

extern "C" int groot_host_acov_merge(uint32_t n_paths, uint32_t n_ctx, const uint64_t *const *ec_off, const uint32_t *const *ec_ids, const uint64_t *const *ec_count,
                                     const uint64_t *n_ec, const uint32_t *const *tuples, const uint64_t *const *tn, const uint64_t *n_tuples, uint64_t *out_off,
                                     uint32_t *out_ids, uint64_t *out_count, uint32_t *out_tuples, uint64_t *out_tn, uint64_t *n_ec_out, uint64_t *n_tuples_out)
{
    if ((n_ctx && (!ec_off || !ec_ids || !ec_count || !n_ec || !tuples || !tn || !n_tuples)) || !out_off || !n_ec_out || !n_tuples_out)
        return set_error(GROOT_E_INVALID, "null argument");
    EcMap m;
    for (uint32_t c = 0; c < n_ctx; c++)
        if (int rc = canonical_ecs(n_paths, n_ec[c], ec_off[c], ec_ids[c], ec_count[c], m)) return rc;
    std::map<std::vector<uint32_t>, uint32_t> index;
    for (const auto &kv : m) { const uint32_t i = (uint32_t)index.size(); index[kv.first] = i; }
    std::vector<Tuple> all;
    std::vector<uint32_t> v, local;
    for (uint32_t c = 0; c < n_ctx; c++) {
        local.assign(n_ec[c], ~0u);
        for (uint64_t e = 0; e < n_ec[c]; e++) {
            v.assign(ec_ids[c] + ec_off[c][e], ec_ids[c] + ec_off[c][e + 1]);
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
            auto it = index.find(v);
            if (it != index.end()) local[e] = it->second;
        }
        for (uint64_t i = 0; i < n_tuples[c]; i++) {
            const uint32_t e = tuples[c][4 * i];
            if (e >= n_ec[c] || local[e] == ~0u) return set_error(GROOT_E_INVALID, "export %u, tuple %llu: EC %u is not in its list", c, (unsigned long long)i, e);
            all.push_back(Tuple{local[e], tuples[c][4 * i + 1], tuples[c][4 * i + 2], tuples[c][4 * i + 3], tn[c][i]});
        }
    }
    tuples_canonical(all);
    uint64_t e = 0, at = 0;
    out_off[0] = 0;
    for (const auto &kv : m) {
        for (uint32_t p : kv.first) out_ids[at++] = p;
        out_count[e] = kv.second;
        out_off[++e] = at;
    }
    for (size_t i = 0; i < all.size(); i++) {
        out_tuples[4 * i] = all[i].ec; out_tuples[4 * i + 1] = all[i].path; out_tuples[4 * i + 2] = all[i].pos; out_tuples[4 * i + 3] = all[i].last;
        out_tn[i] = all[i].n;
    }
    *n_ec_out = e;
    *n_tuples_out = all.size();
    return GROOT_OK;
}

extern "C" int groot_host_acov_depth(uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const double *alpha, uint64_t n_tuples,
                                     const uint32_t *tuples, const uint64_t *tn, uint32_t path, uint32_t path_len, double *depth)
{
    if ((n_ec && !off) || !alpha || (n_tuples && (!tuples || !tn)) || (path_len && !depth) || path >= n_paths) return set_error(GROOT_E_INVALID, "bad argument");
    std::vector<Tuple> t;
    if (int rc = tuples_by_path(n_paths, n_ec, off, ids, n_tuples, tuples, tn, t)) return rc;
    size_t lo = 0;
    while (lo < t.size() && t[lo].path < path) lo++;
    size_t hi = lo;
    while (hi < t.size() && t[hi].path == path) hi++;
    std::vector<double> D;
    std::vector<int64_t> diff;
    depth_of(t, lo, hi, off, ids, alpha, path, path_len, D, diff);
    std::copy(D.begin(), D.end(), depth);
    return GROOT_OK;
}

static int calls_from_table(const groot_index_view *ix, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, const double *alpha,
                            uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn, double min_reads, double call_depth, double cov_cutoff,
                            const char *out_path, uint64_t *n_lines, uint64_t *n_called, const Support *sup)
{
    if (!ix) return set_error(GROOT_E_INVALID, "null argument");
    const uint32_t n = ix->n_paths;
    std::vector<const char *> name_ptr(n);
    std::vector<uint32_t> name_len(n);
    for (uint32_t p = 0; p < n; p++) {
        name_ptr[p] = ix->path_names + ix->path_name_off[p];
        name_len[p] = ix->path_name_off[p + 1] - ix->path_name_off[p];
    }
    return write_calls(n, name_ptr.data(), name_len.data(), ix->path_len, n_ec, off, ids, count, alpha, n_tuples, tuples, tn, min_reads, call_depth, cov_cutoff,
                       out_path, n_lines, n_called, sup);
}

extern "C" int groot_host_calls_from_table(const groot_index_view *ix, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                                           const double *alpha, uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn, double min_reads,
                                           double call_depth, double cov_cutoff, const char *out_path, uint64_t *n_lines, uint64_t *n_called)
{
    return calls_from_table(ix, n_ec, off, ids, count, alpha, n_tuples, tuples, tn, min_reads, call_depth, cov_cutoff, out_path, n_lines, n_called, nullptr);
}

extern "C" int groot_host_call_support(uint32_t n_paths, const uint32_t *path_len, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                                       uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn, uint32_t n_boot, const uint64_t *boot_count,
                                       const double *alpha, double call_depth, uint32_t n_sel, const uint32_t *sel_paths, uint32_t threads, uint32_t *covered_out)
{
    return call_support(n_paths, path_len, n_ec, off, ids, count, n_tuples, tuples, tn, n_boot, boot_count, alpha, call_depth, n_sel, sel_paths, threads,
                        covered_out);
}

extern "C" int groot_host_calls_support_from_table(const groot_index_view *ix, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count,
                                                   const double *alpha, uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn, double min_reads,
                                                   double call_depth, double cov_cutoff, uint32_t n_boot, uint64_t seed, uint32_t threads,
                                                   const uint64_t *boot_count, const double *boot_alpha, const uint32_t *covered, const char *out_path,
                                                   uint64_t *n_lines, uint64_t *n_called)
{
    if (n_boot == 0) return set_error(GROOT_E_INVALID, "no bootstrap replicates");
    const Support sup{n_boot, seed, threads, boot_count, boot_alpha, covered};
    return calls_from_table(ix, n_ec, off, ids, count, alpha, n_tuples, tuples, tn, min_reads, call_depth, cov_cutoff, out_path, n_lines, n_called, &sup);
}

namespace {
// a BAM as a table: reference names and lengths, the canonical ECs of its reads (one QNAME a read) and their tuples
struct BamTable {
    std::vector<std::string> names;
    std::vector<uint32_t> lens, ids, tup;
    std::vector<uint64_t> off{0}, count, tn;
};

int bam_table(const char *bam_path, BamTable &b)
{
    std::vector<uint64_t> read_ref;
    std::vector<std::array<uint32_t, 4>> recs;
    if (int rc = report_bam(bam_path, 0.97, 0, nullptr, nullptr, nullptr, nullptr, &read_ref, &b.names, &recs, &b.lens)) return rc;
    // S(read) as report_abundance builds it, and the read's EC
    EcMap m;
    std::vector<std::vector<uint32_t>> set_of;
    std::vector<uint32_t> v;
    for (size_t i = 0; i < read_ref.size();) {
        size_t j = i;
        v.clear();
        while (j < read_ref.size() && read_ref[j] >> 32 == read_ref[i] >> 32) v.push_back((uint32_t)read_ref[j++]);
        const uint32_t rd = (uint32_t)(read_ref[i] >> 32);
        if (set_of.size() <= rd) set_of.resize((size_t)rd + 1);
        set_of[rd] = v;
        m[v]++;
        i = j;
    }
    std::map<std::vector<uint32_t>, uint32_t> index;
    for (const auto &kv : m) {
        const uint32_t i = (uint32_t)index.size();
        index[kv.first] = i;
        b.ids.insert(b.ids.end(), kv.first.begin(), kv.first.end());
        b.off.push_back(b.ids.size());
        b.count.push_back(kv.second);
    }
    std::vector<uint32_t> ec_of(set_of.size(), 0);
    for (size_t r = 0; r < set_of.size(); r++)
        if (!set_of[r].empty()) ec_of[r] = index[set_of[r]];
    std::vector<Tuple> t;
    t.reserve(recs.size());
    for (const auto &r : recs) t.push_back(Tuple{ec_of[r[0]], r[1], r[2], r[3], 1});
    tuples_canonical(t);
    b.tup.resize(4 * t.size());
    b.tn.resize(t.size());
    for (size_t i = 0; i < t.size(); i++) {
        b.tup[4 * i] = t[i].ec; b.tup[4 * i + 1] = t[i].path; b.tup[4 * i + 2] = t[i].pos; b.tup[4 * i + 3] = t[i].last;
        b.tn[i] = t[i].n;
    }
    return GROOT_OK;
}
} // namespace

static int report_calls(const char *bam_path, double min_reads, double call_depth, double cov_cutoff, const char *out_path, uint64_t *n_lines,
                        uint64_t *n_called, uint64_t *n_tuples, const Support *sup)
{
    BamTable b;
    if (int rc = bam_table(bam_path, b)) return rc;
    if (n_tuples) *n_tuples = b.tn.size();
    std::vector<const char *> name_ptr(b.names.size());
    for (size_t r = 0; r < b.names.size(); r++) name_ptr[r] = b.names[r].c_str();
    return write_calls((uint32_t)b.names.size(), name_ptr.data(), nullptr, b.lens.data(), b.count.size(), b.off.data(), b.ids.data(), b.count.data(), nullptr,
                       b.tn.size(), b.tup.data(), b.tn.data(), min_reads, call_depth, cov_cutoff, out_path, n_lines, n_called, sup);
}

extern "C" int groot_host_report_calls(const char *bam_path, double min_reads, double call_depth, double cov_cutoff, const char *out_path, uint64_t *n_lines,
                                       uint64_t *n_called, uint64_t *n_tuples)
{
    return report_calls(bam_path, min_reads, call_depth, cov_cutoff, out_path, n_lines, n_called, n_tuples, nullptr);
}

extern "C" int groot_host_report_calls_support(const char *bam_path, double min_reads, double call_depth, double cov_cutoff, uint32_t n_boot, uint64_t seed,
                                               uint32_t threads, const char *out_path, uint64_t *n_lines, uint64_t *n_called, uint64_t *n_tuples)
{
    if (n_boot == 0) return set_error(GROOT_E_INVALID, "no bootstrap replicates");
    const Support sup{n_boot, seed, threads, nullptr, nullptr, nullptr};
    return report_calls(bam_path, min_reads, call_depth, cov_cutoff, out_path, n_lines, n_called, n_tuples, &sup);
}

// ---- rarefaction curves (groot_host.h "rarefaction curves") --------------------------------------------------------------------
extern "C" int groot_host_rarefy_depths(uint64_t n_units, uint32_t n_steps, uint64_t *m)
{
    if (n_steps == 0 || !m) return set_error(GROOT_E_INVALID, "no rarefaction steps");
    const uint64_t D = n_steps;
    for (uint64_t s = 1; s <= D; s++) m[s - 1] = (n_units / D) * s + ((n_units % D) * s) / D;
    return GROOT_OK;
}

extern "C" int groot_host_em_rarefy(uint32_t n_paths, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, uint32_t n_rep,
                                    uint32_t n_depths, const uint64_t *depths, uint64_t seed, uint32_t min_iter, uint32_t max_iter, uint32_t threads,
                                    uint64_t *rare_count, double *alpha, uint32_t *iterations)
{
    if ((n_ec && (!off || !count)) || (n_paths && !alpha) || (n_depths && !depths)) return set_error(GROOT_E_INVALID, "null argument");
    if (n_rep == 0) return set_error(GROOT_E_INVALID, "no rarefaction replicates");
    if (n_depths == 0) return set_error(GROOT_E_INVALID, "no rarefaction depths");
    if (max_iter < min_iter)
        return set_error(GROOT_E_INVALID, "number of EM iterations (%u) must be greater than minimum iterations (%u)", max_iter, min_iter);
    if (max_iter < 1) return set_error(GROOT_E_INVALID, "no EM iterations were ran");
    std::vector<uint64_t> cum(n_ec + 1, 0);
    for (uint64_t e = 0; e < n_ec; e++) {
        if (off[e + 1] < off[e] || (off[e + 1] > off[e] && !ids)) return set_error(GROOT_E_INVALID, "EC %llu: bad offsets", (unsigned long long)e);
        for (uint64_t i = off[e]; i < off[e + 1]; i++)
            if (ids[i] >= n_paths) return set_error(GROOT_E_INVALID, "EC %llu holds path %u of %u", (unsigned long long)e, ids[i], n_paths);
        cum[e + 1] = cum[e] + count[e];
        if (cum[e + 1] < cum[e]) return set_error(GROOT_E_INVALID, "the EC counts sum to 2^64 or more");
    }
    const uint64_t total = cum[n_ec];
    if (total == 0) return set_error(GROOT_E_INVALID, "rarefaction over ECs without reads");
    if (total >= groot::kRareMaxUnits) return set_error(GROOT_E_UNSUPPORTED, "rarefaction: 2^62 units and more");
    for (uint32_t d = 0; d < n_depths; d++) {
        if (depths[d] == 0 || depths[d] > total)
            return set_error(GROOT_E_INVALID, "rarefaction depth %u is %llu: not in [1, %llu]", d, (unsigned long long)depths[d], (unsigned long long)total);
        if (d && depths[d] < depths[d - 1]) return set_error(GROOT_E_INVALID, "rarefaction depth %u is below depth %u", d, d - 1);
    }
    const uint32_t h = groot::rare_half_bits(total);
    std::atomic<uint32_t> next_b{0};
    std::atomic<int> failed{0};
    auto work = [&]() {
        std::vector<uint64_t> run(n_ec);               // the counts of the draws so far: the depths are nested
        for (uint32_t b; (b = next_b.fetch_add(1)) < n_rep;) {
            std::fill(run.begin(), run.end(), 0);
            const uint64_t key = groot::rare_key(seed, b);
            uint64_t j = 0;
            for (uint32_t d = 0; d < n_depths; d++) {
                for (; j < depths[d]; j++) {
                    const uint64_t t = groot::rare_pi(key, h, total, j);
                    run[(std::upper_bound(cum.begin(), cum.end(), t) - cum.begin()) - 1]++;     // cum[e] <= t < cum[e + 1]
                }
                const size_t v = (size_t)b * n_depths + d;
                if (rare_count) std::copy(run.begin(), run.end(), rare_count + v * n_ec);
                if (groot_host_em(n_paths, n_ec, off, ids, run.data(), min_iter, max_iter, alpha + v * n_paths, iterations ? iterations + v : nullptr)) failed = 1;
            }
        }
    };
    const uint32_t nt = std::max(1u, std::min(threads, n_rep));
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nt; t++) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    if (failed) return set_error(GROOT_E_INVALID, "the EM of a rarefaction replicate failed");
    return GROOT_OK;
}

namespace {

// what the rarefaction writer gets ready-made (NULL = computed on `threads` host threads), and the calls table when the called columns are wanted
struct Rarefy {
    uint32_t n_rep = 0, n_steps = 0;
    uint64_t seed = 1;
    uint32_t threads = 1;
    const uint64_t *rare_count = nullptr;
    const double *rare_alpha = nullptr;
    bool calls = false;
    uint64_t n_tuples = 0;
    const uint32_t *tuples = nullptr;
    const uint64_t *tn = nullptr;
    double call_depth = 1.0, cov_cutoff = 0.97;
    uint32_t n_sel = 0;
    const uint32_t *covered = nullptr;
    uint32_t *iter_range = nullptr;     // [2]: the fewest and the most EM iterations of the replicates computed here
};

// the rarefaction file over canonical ECs (groot_host.h)
int write_rarefy(uint32_t n_paths, const uint32_t *lens, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, double min_reads,
                 const Rarefy &r, const char *out_path, uint64_t *n_lines)
{
    if (r.n_rep == 0) return set_error(GROOT_E_INVALID, "no rarefaction replicates");
    if (r.n_steps == 0) return set_error(GROOT_E_INVALID, "no rarefaction steps");
    if (r.calls && r.cov_cutoff > 1.0) return set_error(GROOT_E_INVALID, "supplied coverage cutoff exceeds 1.0 (100%%): %g", r.cov_cutoff);
    if ((n_ec && (!off || !count)) || (r.calls && ((n_paths && !lens) || (r.n_tuples && (!r.tuples || !r.tn))))) return set_error(GROOT_E_INVALID, "null argument");
    const uint32_t R = r.n_rep, D = r.n_steps;
    uint64_t N = 0;
    for (uint64_t e = 0; e < n_ec; e++) N += count[e];
    std::vector<uint64_t> m(D), drawn;
    if (int rc = groot_host_rarefy_depths(N, D, m.data())) return rc;
    for (uint32_t s = 0; s + 1 < D; s++)
        if (m[s]) drawn.push_back(m[s]);
    const uint32_t K = (uint32_t)drawn.size();
    if ((uint64_t)R * K > 0xFFFFFFFFull) return set_error(GROOT_E_INVALID, "rarefaction: %u replicates of %u depths", R, K);
    // the replicates at the drawn depths
    std::vector<uint64_t> own_rc;
    std::vector<double> own_ra;
    const uint64_t *rc_ = r.rare_count;
    const double *ra = r.rare_alpha;
    if (K && !ra) {
        own_rc.resize((size_t)R * K * n_ec);
        own_ra.resize((size_t)R * K * n_paths);
        std::vector<uint32_t> its((size_t)R * K);
        if (int rc = groot_host_em_rarefy(n_paths, n_ec, off, ids, count, R, K, drawn.data(), r.seed, GROOT_EM_MIN_ITER, GROOT_EM_MAX_ITER, r.threads, own_rc.data(),
                                          own_ra.data(), its.data()))
            return rc;
        if (r.iter_range) {
            r.iter_range[0] = *std::min_element(its.begin(), its.end());
            r.iter_range[1] = *std::max_element(its.begin(), its.end());
        }
        rc_ = own_rc.data(); ra = own_ra.data();
    }
    // the number of paths among sel (all paths: sel NULL) that are detected in alpha, and called when cov (covered bases, in sel's order) is given
    auto tally = [&](const double *alpha, const std::vector<uint32_t> *sel, const uint32_t *cov, uint64_t &args, uint64_t &called) {
        args = called = 0;
        const size_t n = sel ? sel->size() : n_paths;
        for (size_t i = 0; i < n; i++) {
            const uint32_t p = sel ? (*sel)[i] : (uint32_t)i;
            if (!(alpha[p] >= min_reads)) continue;
            args++;
            if (!cov) continue;
            const double breadth = lens[p] ? (double)cov[i] / (double)lens[p] : 0.0;
            called += breadth >= r.cov_cutoff ? 1u : 0u;
        }
    };
    std::vector<uint64_t> args((size_t)R * K, 0), called((size_t)R * K, 0);
    if (K && r.calls) {
        std::vector<uint8_t> seen(n_paths, 0);
        for (size_t v = 0; v < (size_t)R * K; v++)
            for (uint32_t p = 0; p < n_paths; p++)
                if (ra[v * n_paths + p] >= min_reads) seen[p] = 1;
        std::vector<uint32_t> sel;
        for (uint32_t p = 0; p < n_paths; p++)
            if (seen[p]) sel.push_back(p);
        std::vector<uint32_t> own_cov;
        const uint32_t *cov = r.covered;
        if (cov && r.n_sel != sel.size()) return set_error(GROOT_E_INVALID, "rarefaction: covered has %u paths a replicate, %zu are detected", r.n_sel, sel.size());
        if (!cov && !sel.empty()) {
            if (!rc_) return set_error(GROOT_E_INVALID, "rarefaction: the called columns need rare_count or covered");
            own_cov.resize((size_t)R * K * sel.size());
            if (int rc = call_support(n_paths, lens, n_ec, off, ids, count, r.n_tuples, r.tuples, r.tn, R * K, rc_, ra, r.call_depth, (uint32_t)sel.size(), sel.data(),
                                      r.threads, own_cov.data()))
                return rc;
            cov = own_cov.data();
        }
        for (size_t v = 0; v < (size_t)R * K; v++) tally(ra + v * n_paths, &sel, sel.empty() ? nullptr : cov + v * sel.size(), args[v], called[v]);
    } else {
        for (size_t v = 0; v < (size_t)R * K; v++) tally(ra + v * n_paths, nullptr, nullptr, args[v], called[v]);
    }
    // the step s = D: the point estimate, and with calls its pileup through the same code (boot_count = count: f = w)
    uint64_t args_all = 0, called_all = 0;
    if (N) {
        std::vector<double> alpha(n_paths);
        if (int rc = groot_host_em(n_paths, n_ec, off, ids, count, GROOT_EM_MIN_ITER, GROOT_EM_MAX_ITER, alpha.data(), nullptr)) return rc;
        if (r.calls) {
            std::vector<uint32_t> sel;
            for (uint32_t p = 0; p < n_paths; p++)
                if (alpha[p] >= min_reads) sel.push_back(p);
            std::vector<uint32_t> cov(sel.size() + 1);
            if (!sel.empty())
                if (int rc = call_support(n_paths, lens, n_ec, off, ids, count, r.n_tuples, r.tuples, r.tn, 1, count, alpha.data(), r.call_depth, (uint32_t)sel.size(),
                                          sel.data(), 1, cov.data()))
                    return rc;
            tally(alpha.data(), &sel, cov.data(), args_all, called_all);
        } else {
            tally(alpha.data(), nullptr, nullptr, args_all, called_all);
        }
    }
    FILE *out = out_path ? fopen(out_path, "w") : stdout;
    if (!out) return set_error(GROOT_E_IO, "cannot create %s", out_path);
    uint64_t lines = 0;
    std::vector<uint64_t> v(R);
    const uint32_t q = (uint32_t)((25ull * (R - 1)) / 1000);
    // mean (summed in replicate order), v[q] and v[R - 1 - q] of the sorted integers
    auto columns = [&](const std::vector<uint64_t> &x, uint32_t k) {
        double s = 0.0;
        for (uint32_t b = 0; b < R; b++) { v[b] = x[(size_t)b * K + k]; s += (double)v[b]; }
        std::sort(v.begin(), v.end());
        fprintf(out, "\t%.2f\t%llu\t%llu", s / (double)R, (unsigned long long)v[q], (unsigned long long)v[R - 1 - q]);
    };
    uint32_t k = 0;
    for (uint32_t s = 1; s <= D; s++) {
        if (m[s - 1] == 0) continue;
        fprintf(out, "%.4f\t%llu", (double)s / (double)D, (unsigned long long)m[s - 1]);
        if (s < D) {
            columns(args, k);
            if (r.calls) columns(called, k);
            k++;
        } else {
            fprintf(out, "\t%.2f\t%llu\t%llu", (double)args_all, (unsigned long long)args_all, (unsigned long long)args_all);
            if (r.calls) fprintf(out, "\t%.2f\t%llu\t%llu", (double)called_all, (unsigned long long)called_all, (unsigned long long)called_all);
        }
        fputc('\n', out);
        lines++;
    }
    if (out_path) fclose(out); else fflush(out);
    if (n_lines) *n_lines = lines;
    return GROOT_OK;
}

} // namespace

extern "C" int groot_host_rarefy_from_ecs(const groot_index_view *ix, uint64_t n_ec, const uint64_t *off, const uint32_t *ids, const uint64_t *count, double min_reads,
                                          uint32_t n_rep, uint32_t n_steps, uint64_t seed, uint32_t threads, const uint64_t *rare_count, const double *rare_alpha,
                                          int with_calls, uint64_t n_tuples, const uint32_t *tuples, const uint64_t *tn, double call_depth, double cov_cutoff,
                                          uint32_t n_sel, const uint32_t *covered, const char *out_path, uint64_t *n_lines)
{
    if (!ix || (n_ec && (!off || !count))) return set_error(GROOT_E_INVALID, "null argument");
    Rarefy r;
    r.n_rep = n_rep; r.n_steps = n_steps; r.seed = seed; r.threads = threads; r.rare_count = rare_count; r.rare_alpha = rare_alpha;
    if (with_calls) {
        r.calls = true; r.n_tuples = n_tuples; r.tuples = tuples; r.tn = tn; r.call_depth = call_depth; r.cov_cutoff = cov_cutoff; r.n_sel = n_sel; r.covered = covered;
        return write_rarefy(ix->n_paths, ix->path_len, n_ec, off, ids, count, min_reads, r, out_path, n_lines);
    }
    EcMap m;
    if (int rc = canonical_ecs(ix->n_paths, n_ec, off, ids, count, m)) return rc;
    std::vector<uint64_t> c_off{0}, c_cnt;
    std::vector<uint32_t> c_ids;
    for (const auto &kv : m) {
        c_ids.insert(c_ids.end(), kv.first.begin(), kv.first.end());
        c_off.push_back(c_ids.size());
        c_cnt.push_back(kv.second);
    }
    return write_rarefy(ix->n_paths, ix->path_len, m.size(), c_off.data(), c_ids.data(), c_cnt.data(), min_reads, r, out_path, n_lines);
}

extern "C" int groot_host_report_rarefy(const char *bam_path, double min_reads, uint32_t n_rep, uint32_t n_steps, uint64_t seed, uint32_t threads, int with_calls,
                                        double call_depth, double cov_cutoff, const char *out_path, uint64_t *n_lines, uint32_t *iter_range)
{
    if (n_rep == 0) return set_error(GROOT_E_INVALID, "no rarefaction replicates");
    if (n_steps == 0) return set_error(GROOT_E_INVALID, "no rarefaction steps");
    BamTable b;
    if (int rc = bam_table(bam_path, b)) return rc;
    Rarefy r;
    r.n_rep = n_rep; r.n_steps = n_steps; r.seed = seed; r.threads = threads; r.iter_range = iter_range;
    if (iter_range) iter_range[0] = iter_range[1] = 0;
    if (with_calls) {
        r.calls = true; r.n_tuples = b.tn.size(); r.tuples = b.tup.data(); r.tn = b.tn.data(); r.call_depth = call_depth; r.cov_cutoff = cov_cutoff;
    }
    return write_rarefy((uint32_t)b.names.size(), b.lens.data(), b.count.size(), b.off.data(), b.ids.data(), b.count.data(), min_reads, r, out_path, n_lines);
}

// ---- reading an abundance file back (align --assignFrom; groot_host.h "assignment") ------------------------------------------
extern "C" int groot_host_abundance_read(const groot_index_view *ix, const char *path, double *alpha_out, uint64_t *n_named)
{
    if (!ix || !path || (ix->n_paths && !alpha_out)) return set_error(GROOT_E_INVALID, "null argument");
    const uint32_t n = ix->n_paths;
    constexpr uint32_t kAmbiguous = 0xFFFFFFFFu;
    std::unordered_map<std::string, uint32_t> by_name;         // the name as the report prints it -> path (kAmbiguous: two paths share it)
    for (uint32_t p = 0; p < n; p++) {
        const char *nm = ix->path_names + ix->path_name_off[p];
        size_t nl = ix->path_name_off[p + 1] - ix->path_name_off[p];
        if (nl && nm[0] == '*') { nm++; nl--; }
        auto ins = by_name.emplace(std::string(nm, nl), p);
        if (!ins.second) ins.first->second = kAmbiguous;
    }
    FILE *f = fopen(path, "r");
    if (!f) return set_error(GROOT_E_IO, "cannot open %s", path);
    std::string text;
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return set_error(GROOT_E_IO, "cannot read %s", path);
    for (uint32_t p = 0; p < n; p++) alpha_out[p] = 0.0;
    std::vector<uint8_t> seen(n, 0);
    uint64_t lines = 0, line_no = 0;
    for (size_t at = 0; at < text.size();) {
        size_t end = text.find('\n', at);
        if (end == std::string::npos) end = text.size();
        std::string line = text.substr(at, end - at);
        at = end + 1;
        line_no++;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const size_t t1 = line.find('\t'), t2 = t1 == std::string::npos ? t1 : line.find('\t', t1 + 1);
        if (t2 == std::string::npos || t2 + 1 >= line.size())
            return set_error(GROOT_E_FORMAT, "%s line %llu: fewer than 3 columns", path, (unsigned long long)line_no);
        const std::string name = line.substr(0, t1);
        size_t t3 = line.find('\t', t2 + 1);
        if (t3 == std::string::npos) t3 = line.size();
        const std::string val = line.substr(t2 + 1, t3 - t2 - 1);
        char *ep = nullptr;
        const double v = strtod(val.c_str(), &ep);
        if (val.empty() || ep != val.c_str() + val.size() || !(v >= 0.0 && v <= 1e300))
            return set_error(GROOT_E_FORMAT, "%s line %llu: em_reads '%s' is not a finite number in [0, 1e300]", path, (unsigned long long)line_no, val.c_str());
        const auto it = by_name.find(name);
        if (it == by_name.end()) return set_error(GROOT_E_FORMAT, "%s line %llu: '%s' is not a reference of the index", path, (unsigned long long)line_no, name.c_str());
        if (it->second == kAmbiguous) return set_error(GROOT_E_FORMAT, "%s line %llu: two references of the index are called '%s'", path, (unsigned long long)line_no, name.c_str());
        if (seen[it->second]) return set_error(GROOT_E_FORMAT, "%s line %llu: '%s' is given twice", path, (unsigned long long)line_no, name.c_str());
        seen[it->second] = 1;
        alpha_out[it->second] = v;
        lines++;
    }
    if (n_named) *n_named = lines;
    return GROOT_OK;
}
