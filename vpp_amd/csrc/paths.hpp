// Reachability paths (pg_reach_paths): one well-defined shortest path per (src, dst) query over a
// pg_reach_closure out_hops, and per end point the number of those paths that pass through it,
// written once for both sides like closure.hpp -- the gfx950 kernels (paths.hip) and the host twin
// (pg_debug_reach_paths_host, tests only) run the same predecessor search, the same path store, the
// same partition and the same plan.
//
// hops is n x n uint16_t, row-major, 0 = not reachable; edge(a, b) <=> hops(a, b) == 1. The path of
// (i, j) with d = hops(i, j) > 0 is p_0 = i .. p_d = j, and for t = d .. 2 the *least predecessor*
//   p_{t-1} = the least k with hops(i, k) == t - 1 and hops(k, p_t) == 1.
// It depends on (i, p_t) only, so the paths of one src form a tree. The search reads row i of hops
// (staged once per src) and the column p_t of the edge relation; the column comes from the transposed
// edge bit matrix ET, built once per call: bit r of ET[c][r / 32] is hops(r, c) == 1, rows of
// closure_stride(n) words, padding bits and padding words zero. A set bit of ET therefore always names
// a k below n, on any input. A step that finds no k (an input no closure wrote) makes the query
// *broken*.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "blobwalk.hpp"
#include "closure.hpp"

namespace pg {

constexpr uint32_t kPathsMaxN = kClosureMaxN, kPathsMaxLen = 1u << 15;
constexpr uint64_t kPathsMaxQueries = 1ull << 24;
constexpr uint32_t kPathsNone = 0xFFFFu;       // a nodes entry behind the path; every entry of a row without one
constexpr uint32_t kPathsNoPred = 0xFFFFFFFFu;  // paths_word_pred: no set bit of the word is a predecessor
constexpr uint32_t kPathsBlock = 256, kPathsWaves = kPathsBlock / 64;
// the bit-words of an ET row one pass of a wave covers (a lane one word): 2048 columns
constexpr uint32_t kPathsPassWords = 64;
// the queries of one src a work item holds at most: a wave takes every kPathsWaves-th of them. 256: an
// all-pairs call over 4096 end points is 65,536 items, and 64 sources with all targets still give
// every CU four
constexpr uint32_t kPathsChunkQueries = 256;
// out_via is counted in LDS, n words beside the staged row, up to this many end points (48 KiB with the row:
// three workgroups a CU); beyond, by adds to out_via itself
constexpr uint32_t kPathsViaLdsMaxN = 8192;
// the edge kernel: a workgroup transposes 64 columns x 4 bit-words (128 rows), a wave one word
constexpr uint32_t kPathsEdgeCols = 64, kPathsEdgeWords = 4;
static_assert(kPathsEdgeWords == kPathsWaves, "k_paths_edges_t: one bit-word per wave");

// The predecessor search over one bit-word: `bits` is word w of ET[p_t], row is row i of hops, want
// is t - 1. -> the least k of the word with row[k] == want, or kPathsNoPred. (Every set bit names a
// k < n: the reads of row stay inside it.)
PG_HD uint32_t paths_word_pred(uint32_t bits, uint32_t w, const uint16_t* row, uint32_t want) {
    for (; bits; bits &= bits - 1u) {
        const uint32_t k = 32u * w + (uint32_t)__builtin_ctz(bits);
        if (row[k] == want) return k;
    }
    return kPathsNoPred;
}

// The path store. A found node goes to its place as it is found; entries [from, end) of a nodes row
// get kPathsNone, `lane` of `lanes` writers taking every lanes-th: the tail behind a path (from = d
// + 1), or the whole row of a query without one (from = 0).
PG_HD void paths_store(uint16_t* nrow, uint32_t t, uint32_t node) { nrow[t] = (uint16_t)node; }
PG_HD void paths_fill(uint16_t* nrow, uint32_t from, uint32_t end, uint32_t lane, uint32_t lanes) {
    for (uint32_t t = from + lane; t < end; t += lanes) nrow[t] = (uint16_t)kPathsNone;
}

// bit-word w (rows 32 w ..) of ET[c] from the hops column, as k_paths_edges_t's lane builds it
PG_HD uint32_t paths_edge_word(const uint16_t* hops, uint32_t n, uint32_t c, uint32_t w) {
    uint32_t bits = 0;
    PG_UNROLL
    for (uint32_t b = 0; b < 32u; b++) {
        const uint32_t r = 32u * w + b;
        if (r < n && hops[(size_t)r * n + c] == 1u) bits |= 1u << b;
    }
    return bits;
}

// what the workgroups add up: pg_reach_paths_result, and its words in the scratch block
struct PathsResult {
    uint64_t n_found, n_unreachable, n_too_long, n_broken, n_via;
    uint32_t longest;
};
constexpr uint32_t kPathsResultWords = 6;  // u64: the five sums, and the maximum

// ---- the partition and the plan (host only) ------------------------------------------------------
// How a call is cut: a work item is at most chunk_queries queries of one src; a workgroup stages that
// src's row of hops in LDS: row_bytes (the row, and 16 B so that the staged row can take the global
// row's alignment), the waves' counters, and with out_via up to kPathsViaLdsMaxN end points via_bytes
// for its counts; lds_bytes is all of it, the most a workgroup takes. The one function the launch, the
// host twin and pg_debug_reach_paths_plan use.
struct PathsPlan {
    uint32_t chunk_queries, lds_bytes, row_bytes, via_bytes;
};
inline PathsPlan paths_plan(uint32_t n) {
    const uint32_t row = ((2u * n + 15u) & ~15u) + 16u;
    const uint32_t via = n <= kPathsViaLdsMaxN ? ((4u * n + 15u) & ~15u) : 0u;
    return PathsPlan{kPathsChunkQueries, row + kPathsWaves * kPathsResultWords * (uint32_t)sizeof(uint64_t) + via, row, via};
}

struct PathsItem {
    uint32_t src, q0, q1;  // sorted queries [q0, q1), all of this src
};
// dst, pos: the queries sorted by src (a stable counting sort), their dst and their position in the
// caller's arrays, where the outputs go; items: in (src, position) order, so consecutive items share
// a src
struct PathsPartition {
    std::vector<uint32_t> dst, pos;
    std::vector<PathsItem> items;
};
inline PathsPartition paths_partition(const uint32_t* src, const uint32_t* dst, uint64_t n_queries, uint32_t n,
                                      uint32_t chunk_queries) {
    PathsPartition p;
    const uint32_t nq = (uint32_t)n_queries;  // (<= 2^24)
    std::vector<uint32_t> start((size_t)n + 1, 0);
    for (uint32_t q = 0; q < nq; q++) start[src[q] + 1]++;
    for (uint32_t i = 0; i < n; i++) start[i + 1] += start[i];
    p.dst.resize(nq), p.pos.resize(nq);
    std::vector<uint32_t> at(start.begin(), start.end() - 1);
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t o = at[src[q]]++;
        p.dst[o] = dst[q], p.pos[o] = q;
    }
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t q = start[i]; q < start[i + 1]; q += chunk_queries)
            p.items.push_back(PathsItem{i, q, q + chunk_queries < start[i + 1] ? q + chunk_queries : start[i + 1]});
    return p;
}

// device.hpp-style API of paths.hip
struct PathsSpecDev {
    const uint16_t* hops;  // device
    uint32_t n;            // >= 1
    uint32_t max_len;      // (read with out_nodes only)
    uint64_t n_queries;
    const PathsPartition* part;  // host; null when n_queries == 0
};
// out_len device; out_nodes / out_via device or null; *res host. 0, -1 (a HIP error) or -2 (the
// scratch allocation failed); synchronises the stream
int dev_reach_paths(uint32_t blocks_per_cu, const PathsSpecDev& spec, uint16_t* out_len, uint16_t* out_nodes,
                    uint32_t* out_via, PathsResult* res, void* stream, std::string* err);

}  // namespace pg
