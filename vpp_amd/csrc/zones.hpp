// Reachability zones (pg_reach_zones): the end points of a pg_reach_closure result that can all
// reach each other, and the graph of those zones, written once for both sides like classes.hpp --
// the gfx950 kernels (zones.hip) and the host twin (pg_debug_reach_zones_host, tests only) run the
// same per-word code over the same plan in the same work-item order.
//
// The input is the audits' layout: n rows of reach_row_words(n) words, 2 bits per cell.
//   R(i, j)   cell (i, j) holds PG_CONN_ALLOW; every other code is "no". Padding bits are masked
//             (closure_valid), never trusted; cell (i, i) is a cell like any other.
//   M(i, j)   R(i, j) and R(j, i): mutual reach.
//   label(i)  the least member of {i} u { j : M(i, j) }. Over a full closure R is transitive and
//             label(i) is the least member of i's strongly connected component; an end point on no
//             cycle is a zone of its own.
//   zones     the distinct values of label[], ascending, get the ids 0, 1, ..: first-appearance
//             numbering as in classes.hpp, so zone[0] == 0 and the representatives ascend.
//   broken    an end point with label(label(i)) != label(i): none where R is transitive. On any input
//             the labels are the formula above and every access stays inside its array.
// The working form is the closure's (closure.hpp): 1 bit per cell, bit-words of 32 cells, rows padded
// to closure_stride(n), padding bits and padding words zero. B holds R, BT its transpose; both come
// from one read of the input.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#include "closure.hpp"

namespace pg {

constexpr uint32_t kZonesBlock = 256, kZonesWaves = kZonesBlock / 64;
// the transpose tile of a workgroup: 128 rows x 32 bit-words (1024 columns). A half wave reads 256
// contiguous bytes of an input row; a BT row leaves the tile as one 16-B store (128 rows = 4 bit-words)
constexpr uint32_t kZonesTileRows = 128, kZonesTileWords = 32, kZonesTileCols = 32u * kZonesTileWords;
constexpr uint32_t kZonesTilePitch = kZonesTileWords + 1u;  // LDS words of a tile row: a column read has no bank conflict
// a label work item: the rows one workgroup takes at once, a wave each
constexpr uint32_t kZonesLabelRows = kZonesWaves;
// k_zones_number: one workgroup; with at most this many zones their sizes are counted in LDS
constexpr uint32_t kZonesNumberBlock = 1024, kZonesLdsZones = 4096;
// the result words in scratch, in pg_reach_zones_result's order
constexpr uint32_t kZonesResultWords = 5;

// bit-word w of row `row` (reach_row_words(n) = rw input words): R as bits, padding masked
PG_HD uint32_t zones_bit_word(const uint32_t* row, uint32_t rw, uint32_t n, uint32_t w) {
    const uint32_t valid = closure_valid(n, w);
    if (!valid) return 0u;
    return closure_bits(row[2u * w], 2u * w + 1u < rw ? row[2u * w + 1u] : 0u) & valid;
}

// what the lane that holds bit-word x of its row gives to the ballot of column k of the word
PG_HD bool zones_ballot_bit(uint32_t x, uint32_t k) { return (x >> k) & 1u; }

// the label of row i from the first non-zero word m = B[i][w] & BT[i][w] of the row (w <= i / 32)
PG_HD uint32_t zones_label(uint32_t i, uint32_t w, uint32_t m) {
    const uint32_t j = 32u * w + (uint32_t)__builtin_ctz(m);
    return j < i ? j : i;
}

// bit j of a row of the working form
PG_HD uint32_t zones_bit(const uint32_t* row, uint32_t j) { return (row[j >> 5] >> (j & 31u)) & 1u; }

// A word of the zone graph from row rep[a] of B: cell k is the row's bit rep[k], for the first
// `left` of the word's 16 cells; ALLOW where set, DENY_SYN elsewhere, padding zero.
PG_HD uint32_t zones_dag_word(const uint32_t* row, const uint32_t* rep, uint32_t left) {
    uint32_t h = 0;
    PG_UNROLL
    for (uint32_t k = 0; k < 16; k++)
        if (k < left) h |= zones_bit(row, rep[k]) << k;
    return closure_expand(h);
}

// How the launches cut the work: the transpose tiles (tile_rows x tile_cols cells, row tiles x column
// tiles of them), the label work items (label_rows rows each) and the most workgroups the zone graph
// can need (one per zone). The one function the launch, the host twin and pg_debug_reach_zones_plan
// use. Host only.
struct ZonesPlan {
    uint32_t tile_rows, tile_cols, row_tiles, col_tiles, bits_grid;
    uint32_t label_rows, label_grid, dag_grid;
};
inline ZonesPlan zones_plan(uint32_t n) {
    ZonesPlan p{kZonesTileRows, kZonesTileCols, (n + kZonesTileRows - 1u) / kZonesTileRows,
                (closure_stride(n) + kZonesTileWords - 1u) / kZonesTileWords, 0, kZonesLabelRows,
                (n + kZonesLabelRows - 1u) / kZonesLabelRows, n};
    p.bits_grid = p.row_tiles * p.col_tiles;
    return p;
}

// device.hpp-style API of zones.hip
struct ZonesOutDev {  // device, each null or as include/policygpu.h says; zone is required
    uint32_t *zone, *rep, *size, *reaches, *reached_by, *dag;
};
struct ZonesResult {  // pg_reach_zones_result
    uint32_t n_zones, n_cyclic, n_multi, largest, n_broken;
};
// matrix device, n >= 1. 0, -1 (a HIP error) or -2 (the scratch allocation failed); synchronises the
// stream once, at its end
int dev_reach_zones(uint32_t blocks_per_cu, const uint32_t* matrix, uint32_t n, const ZonesOutDev& out, ZonesResult* result,
                    void* stream, std::string* err);

}  // namespace pg
