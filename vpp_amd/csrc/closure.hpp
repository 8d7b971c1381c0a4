// Reachability closure (pg_reach_closure): multi-hop reach and hop counts over the ALLOW graph of a
// square pg_reach_matrix result, written once for both sides like diff.hpp -- the gfx950 kernels
// (closure.hip) and the host twin (pg_debug_reach_closure_host, tests only) run the same per-word
// code.
//
// The input is the audits' layout: 2 bits per cell, 16 cells per word, n_svc slices of n rows of
// reach_row_words(n) words. The working form is 1 bit per cell: a *bit-word* holds 32 cells, two
// input words make one, a row has closure_bit_words(n) of them and is padded to closure_stride(n)
// (a multiple of 4, so a lane's 1, 2 or 4 adjacent words are one aligned load). Padding bits of the
// input are masked (closure_valid), never trusted; padding bits and padding words of the working
// matrices are zero.
//
// There is an edge i -> j when some selected slice holds PG_CONN_ALLOW in cell (i, j). Level 1 is
// the edges; level k + 1 is F' = (F (x) A) & ~R, R |= F': the cells first reached by k + 1 edges.
#pragma once
#include <cstdint>
#include <string>

#include "blobwalk.hpp"

namespace pg {

constexpr uint32_t kClosureMaxN = 1u << 15, kClosureMaxSvc = 4096;
constexpr uint32_t kClosureLow = 0x55555555u;
// a level's workgroup of 16 waves owns 16 rows of the output, one per wave; a wave's 64 lanes own 1, 2 or 4
// adjacent bit-words of the row each
constexpr uint32_t kClosureStepBlock = 1024, kClosureWaves = kClosureStepBlock / 64, kClosureWaveRows = 1;
constexpr uint32_t kClosureTileRows = kClosureWaves * kClosureWaveRows;
constexpr uint32_t kClosureBlock = 256;  // the edge and pack kernels

PG_HD uint32_t closure_bit_words(uint32_t n) { return (n + 31u) / 32u; }
PG_HD uint32_t closure_stride(uint32_t n) { return (closure_bit_words(n) + 3u) & ~3u; }

// the cells of a 2-bit word that hold PG_CONN_ALLOW (2), one bit per cell at the cell's low bit
PG_HD uint32_t closure_allow(uint32_t x) { return (x >> 1) & ~x & kClosureLow; }

// 16 cells at the even bit positions -> 16 adjacent bits
PG_HD uint32_t closure_compact(uint32_t m) {
    m &= kClosureLow;
    m = (m | m >> 1) & 0x33333333u;
    m = (m | m >> 2) & 0x0F0F0F0Fu;
    m = (m | m >> 4) & 0x00FF00FFu;
    return (m | m >> 8) & 0xFFFFu;
}

// bit-word w of a row from its two input words (the second 0 where the row has none)
PG_HD uint32_t closure_bits(uint32_t lo, uint32_t hi) {
    return closure_compact(closure_allow(lo)) | closure_compact(closure_allow(hi)) << 16;
}

// the cells of bit-word w of a row that are below n (0 for a padding word)
PG_HD uint32_t closure_valid(uint32_t n, uint32_t w) {
    if (32u * w >= n) return 0u;
    const uint32_t left = n - 32u * w;
    return left >= 32u ? 0xFFFFFFFFu : (1u << left) - 1u;
}

// 16 bits -> a 2-bit word: PG_CONN_ALLOW where the bit is set, PG_CONN_DENY_SYN (0) elsewhere
PG_HD uint32_t closure_expand(uint32_t h) {
    h &= 0xFFFFu;
    h = (h | h << 8) & 0x00FF00FFu;
    h = (h | h << 4) & 0x0F0F0F0Fu;
    h = (h | h << 2) & 0x33333333u;
    h = (h | h << 1) & kClosureLow;
    return h << 1;
}

// one level on one output word: what the products reached that was not reached before
PG_HD uint32_t closure_new(uint32_t acc, uint32_t reached) { return acc & ~reached; }

// How a level's launch cuts the n x n output: a workgroup owns tile_rows rows x tile_cols columns,
// a lane lane_words adjacent bit-words (the narrowest of 1, 2, 4 at which one column tile covers the
// row, 4 beyond). The one function the launch and pg_debug_reach_closure_plan use. Host only.
struct ClosurePlan {
    uint32_t lane_words, tile_rows, tile_cols, row_tiles, col_tiles, grid;
};
inline ClosurePlan closure_plan(uint32_t n) {
    const uint32_t bw = closure_bit_words(n);
    const uint32_t lw = bw <= 64u ? 1u : bw <= 128u ? 2u : 4u;
    const uint32_t tile_words = 64u * lw;
    ClosurePlan p{lw, kClosureTileRows, 32u * tile_words, (n + kClosureTileRows - 1) / kClosureTileRows,
                  (bw + tile_words - 1) / tile_words, 0};
    p.grid = p.row_tiles * p.col_tiles;
    return p;
}

// device.hpp-style API of closure.hip
struct ClosureSpecDev {
    const uint32_t* matrix;    // device
    uint32_t n, n_svc;         // n >= 1
    const uint32_t* svc_list;  // host: the selected slices, ascending
    uint32_t n_list;
    uint32_t max_hops;
};
struct ClosureResult {  // pg_reach_closure_result
    uint32_t levels;
    uint64_t n_edges, n_reachable;
};
// out_packed device; out_hops / out_count device or null; *res host. 0, -1 (a HIP error) or -2 (the
// scratch allocation failed); synchronises the stream
int dev_reach_closure(const ClosureSpecDev& spec, uint32_t* out_packed, uint16_t* out_hops, uint32_t* out_count,
                      ClosureResult* res, void* stream, std::string* err);

}  // namespace pg
