// rescue_fold.hpp -- what rescue.hip folds on the host at collect, as plain host functions: the path bitmaps of a batch's slow rescued
// and slow gap-rescued reads into the host map of equivalence classes, and the log of their kept placements into the host map of assigned
// coverage.  No HIP runtime call and no ctx: tools/rescue_fold_check.cpp runs both on a CPU under the sanitizers.
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

#include "device_types.hpp"   // uint4

namespace groot {

using EcHost = std::map<std::vector<uint32_t>, uint64_t>;                                              // Counters::ec_host
using AcovHost = std::map<std::vector<uint32_t>, std::map<std::array<uint32_t, 3>, uint64_t>>;         // Counters::acov_host

// bits[n][bw], one bitmap per slow read -> every row's ascending list of the IDs below n_paths.  A row with a list is one read of that
// class in ec_host; every row, with a list or without, is one of `slow`.
inline std::vector<std::vector<uint32_t>> unfold_rows(const uint64_t *bits, uint32_t n, uint32_t bw, uint32_t n_paths, EcHost &ec_host, uint64_t &slow)
{
    std::vector<std::vector<uint32_t>> rows(n);
    for (uint32_t i = 0; i < n; i++) {
        for (uint32_t w = 0; w < bw; w++)
            for (uint64_t m = bits[(size_t)i * bw + w]; m; m &= m - 1) {
                const uint32_t id = w * 64 + (uint32_t)__builtin_ctzll(m);
                if (id < n_paths) rows[i].push_back(id);
            }
        if (!rows[i].empty()) ec_host[rows[i]]++;
    }
    slow += n;
    return rows;
}

// log[n_log] = (row | second, path, Pos, last): every entry one record of acov_host under its row's ID list, and one of `records`; an entry
// without the flag `second` (kGapAcovSecond for the gapped records, 0 for a log that has no such flag) one of `placements` too.
// -> -1, or the row of the first entry that names no row of `rows` or an empty one (the entries ahead of it are folded, none behind it)
inline int64_t fold_log(const uint4 *log, size_t n_log, const std::vector<std::vector<uint32_t>> &rows, uint32_t second, AcovHost &acov_host, uint64_t &records,
                        uint64_t &placements)
{
    for (size_t i = 0; i < n_log; i++) {
        const uint4 &e = log[i];
        const uint32_t row = e.x & ~second;
        if (row >= rows.size() || rows[row].empty()) return row;
        acov_host[rows[row]][{e.y, e.z, e.w}]++;
        records++;
        if (!(e.x & second)) placements++;
    }
    return -1;
}

// The log of the fragments on bitmaps (rescued mates in assigned coverage over fragments): log[n_log] = (row | exact, path, Pos, last).  An
// entry whose path is in its row's ID list is one record of acov_host under that list; any other is left out.  count[] gets the exact
// records counted / left out and the kept placements counted / left out (`exact` is the flag that tells the two kinds apart).
// -> -1, or the row of the first entry that names no row of `rows` or an empty one (the entries ahead of it are folded, none behind it)
inline int64_t fold_log_units(const uint4 *log, size_t n_log, const std::vector<std::vector<uint32_t>> &rows, uint32_t exact, AcovHost &acov_host, uint64_t (&count)[4])
{
    for (size_t i = 0; i < n_log; i++) {
        const uint4 &e = log[i];
        const uint32_t row = e.x & ~exact, kind = (e.x & exact) ? 0u : 2u;
        if (row >= rows.size() || rows[row].empty()) return row;
        if (!std::binary_search(rows[row].begin(), rows[row].end(), e.y)) { count[kind + 1]++; continue; }
        acov_host[rows[row]][{e.y, e.z, e.w}]++;
        count[kind]++;
    }
    return -1;
}

} // namespace groot
