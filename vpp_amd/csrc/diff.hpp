// Reachability diff (pg_reach_diff): the cells in which two packed audit results differ, written
// once for both sides like reach.hpp -- the gfx950 kernels (diff.hip) and the host twin
// (pg_debug_reach_diff_host, tests only) run the same per-word code.
//
// Both audits write one layout: 2 bits per cell, 16 cells per word, rows of reach_row_words(n_cols)
// words, padding zero (pg_reach_matrix: row = (service, src), cell = dst; pg_reach_ports: row = (src,
// dst), cell = interval). A diff never looks at a table: it is a pass over two word arrays.
//
// Masks here carry one bit per cell, the low bit of the cell's two (kDiffLow positions): the cells
// of a word that are inside the row (diff_valid), that hold code c (diff_eq), that are selected
// (diff_selected: the two codes differ and bit 4 * before + after of `transitions` is set). Padding
// bits are masked, never trusted. The 4 x 4 histogram counts every valid cell, the diagonal included
// and whatever `transitions` selects.
#pragma once
#include <cstdint>
#include <string>

#include "blobwalk.hpp"

namespace pg {

constexpr uint32_t kDiffLow = 0x55555555u;
constexpr uint32_t kDiffOffDiag = 0xFFFFu & ~0x8421u;  // the twelve transitions that change the code
constexpr uint32_t kDiffMaxCols = 1u << 20;
// a workgroup of 256 lanes takes a tile of 1024 words, 4 consecutive words (one 16-B load) per lane
constexpr uint32_t kDiffBlock = 256, kDiffLaneWords = 4, kDiffTile = kDiffBlock * kDiffLaneWords;

struct DiffShape {
    uint32_t n_words;  // n_rows * row_words < 2^32 (the host checks)
    uint32_t row_words, n_cols, transitions;
};

// the cells of word jw of a row that are below n_cols
PG_HD uint32_t diff_valid(uint32_t n_cols, uint32_t jw) {
    const uint32_t left = n_cols - 16u * jw;  // >= 1: jw < row_words
    return left >= 16u ? kDiffLow : kDiffLow & ((1u << (2u * left)) - 1u);
}

// m[c]: the cells of x that hold code c
struct DiffEq {
    uint32_t m[4];
};
PG_HD DiffEq diff_eq(uint32_t x) {
    const uint32_t lo = x & kDiffLow, hi = (x >> 1) & kDiffLow;
    return DiffEq{{~(lo | hi) & kDiffLow, lo & ~hi, hi & ~lo, lo & hi}};
}

// the selected cells of one word; `transitions` is the same in every lane, so its branches are uniform
PG_HD uint32_t diff_selected(const DiffEq& b, const DiffEq& a, uint32_t x /* before ^ after */, uint32_t valid,
                             uint32_t transitions) {
    const uint32_t t = transitions & kDiffOffDiag;
    if (t == kDiffOffDiag) return (x | (x >> 1)) & valid;
    uint32_t sel = 0;
    if (t) {
        PG_UNROLL
        for (uint32_t bc = 0; bc < 4; bc++) {
            PG_UNROLL
            for (uint32_t ac = 0; ac < 4; ac++)
                if (bc != ac && (t >> (4u * bc + ac) & 1u)) sel |= b.m[bc] & a.m[ac];
        }
    }
    return sel & valid;
}

// h[4 * before + after] += the valid cells of the word with those codes
PG_HD void diff_hist(const DiffEq& b, const DiffEq& a, uint32_t valid, uint32_t (&h)[16]) {
    PG_UNROLL
    for (uint32_t bc = 0; bc < 4; bc++) {
        const uint32_t vb = b.m[bc] & valid;
        PG_UNROLL
        for (uint32_t ac = 0; ac < 4; ac++) h[4u * bc + ac] += (uint32_t)__builtin_popcount(vb & a.m[ac]);
    }
}

// the same for a word that is equal on both sides, the common one in an audit: only the diagonal moves
PG_HD void diff_hist_same(const DiffEq& e, uint32_t valid, uint32_t (&h)[16]) {
    PG_UNROLL
    for (uint32_t c = 0; c < 4; c++) h[5u * c] += (uint32_t)__builtin_popcount(e.m[c] & valid);
}

// pg_reach_change.cell of the cell at bit position `bit` (even) of word jw
PG_HD uint32_t diff_cell(uint32_t jw, uint32_t bit, uint32_t bword, uint32_t aword) {
    return (16u * jw + (bit >> 1)) | ((bword >> bit) & 3u) << 28 | ((aword >> bit) & 3u) << 30;
}

// How a launch cuts n_words: every workgroup owns one contiguous chunk, a multiple of the tile, and
// no workgroup is empty. resident: the workgroups the device holds at once. The one function the
// launch and pg_debug_reach_diff_plan use. Host only.
struct DiffPlan {
    uint32_t tile_words, grid;
    uint64_t chunk_words;
};
inline DiffPlan diff_plan(uint64_t n_words, uint32_t resident) {
    const uint64_t tiles = (n_words + kDiffTile - 1) / kDiffTile;
    const uint64_t g = tiles < resident ? tiles : resident;
    if (!g) return DiffPlan{kDiffTile, 1u, kDiffTile};
    const uint64_t per = (tiles + g - 1) / g;
    return DiffPlan{kDiffTile, (uint32_t)((tiles + per - 1) / per), per * kDiffTile};
}

// device.hpp-style API of diff.hip
struct DiffSpecDev {
    const uint32_t* before;  // device
    const uint32_t* after;
    uint32_t n_rows, n_cols, transitions;
    uint64_t cap;
};
struct DiffEntry {  // pg_reach_change
    uint32_t row, cell;
};
// the plan of a launch over n_words under blocks_per_cu (0 = occupancy) on the current device
DiffPlan dev_diff_plan(uint64_t n_words, uint32_t blocks_per_cu);
// changes / row_changes device or null, n_changes / trans host (trans may be null); synchronises
// the stream
int dev_reach_diff(uint32_t blocks_per_cu, const DiffSpecDev& spec, DiffEntry* changes, uint32_t* row_changes,
                   uint64_t* n_changes, uint64_t* trans, void* stream, std::string* err);

}  // namespace pg
