// Reachability dominators (pg_reach_dominators): the end points every walk from an entry set E to an
// end point v must cross, over the ALLOW graph of a square pg_reach_matrix result, written once for
// both sides like closure.hpp -- the gfx950 kernels (dominators.hip) and the host twin
// (pg_debug_reach_dominators_host, tests only) run the same per-word code over the same plan.
//
// The input and the edge rule are the closure's (closure.hpp): i -> j when some selected slice holds
// PG_CONN_ALLOW in cell (i, j); padding bits are masked (closure_valid), never trusted.
//   Avoid(v)  { k : some walk from E to v contains no k }. Avoid(e) = all \ {e} for e in E, fixed;
//             otherwise the least fixed point of Avoid(v) = (U over edges p -> v of Avoid(p)) \ {v}.
//   reached   column n, which no end point owns: set in the entries' rows, it rides the same product,
//             so bit n of Avoid(v) says that some walk from E ends in v (a chain's last end point is
//             reached although nothing avoids it). An Avoid row therefore has n + 1 columns.
//   Dom(v)    reached(v) ? ~Avoid(v) : {} over the columns below n.
// A round is semi-naive: D'(v) = (U over p in ET[v] with D(p) != {} of D(p)) & ~Avoid(v) & ~bit v,
// Avoid(v) |= D'(v). The sets grow as in the synchronous iteration Avoid' = Avoid | ((ET (x) Avoid)
// minus the diagonal), round for round, so `rounds` -- the rounds in which some set grew -- is the
// same number.
//
// Working form: bit-words of 32 cells. ET (bit p of ET[v]: p -> v) has n rows of closure_stride(n)
// words; Avoid, D and D' have n rows of dom_stride(n) = closure_stride(n + 1) words. Padding bits
// and padding words are zero.
#pragma once
#include <cstdint>
#include <string>

#include "closure.hpp"

namespace pg {

constexpr uint32_t kDomMaxN = kClosureMaxN, kDomMaxSvc = kClosureMaxSvc, kDomMaxEntry = 1u << 15;
constexpr uint32_t kDomNone = 0xFFFFFFFFu;
constexpr uint16_t kDomNoIdom = 0xFFFFu;
// a round's workgroup of 16 waves owns 16 rows of Avoid, one per wave; a wave's 64 lanes own 1, 2 or 4
// adjacent bit-words of the row each
constexpr uint32_t kDomRoundBlock = 1024, kDomWaves = kDomRoundBlock / 64, kDomTileRows = kDomWaves;
static_assert(kDomTileRows == 16, "a tile word of ET covers 16 rows: half a bit-word of end points");
// the edge / transpose tile of a workgroup: 128 rows x 32 bit-words (1024 columns) of the edge matrix,
// which leave as 1024 rows x 4 words of ET
constexpr uint32_t kDomBlock = 256, kDomBlockWaves = kDomBlock / 64;
constexpr uint32_t kDomTRows = 128, kDomTWords = 32, kDomTCols = 32u * kDomTWords, kDomTPitch = kDomTWords + 1u;
// the cut tile of a workgroup: 64 rows x 32 bit-words of Dom
constexpr uint32_t kDomCutRows = 64, kDomCutWords = 32, kDomCutPitch = kDomCutWords + 1u;
constexpr uint32_t kDomResultBlock = 1024;
// the result words in scratch: n_reached, n_chokes, top, top_cut, depth
constexpr uint32_t kDomResultWords = 5;

PG_HD uint32_t dom_cols(uint32_t n) { return n + 1u; }  // the end points and the reached column
PG_HD uint32_t dom_bit_words(uint32_t n) { return closure_bit_words(dom_cols(n)); }
PG_HD uint32_t dom_stride(uint32_t n) { return closure_stride(dom_cols(n)); }

// bit-word w of row i of the edge matrix: the selected slices' ALLOW cells ORed, padding masked.
// rw = reach_row_words(n), slice = n * rw words
PG_HD uint32_t dom_edge_word(const uint32_t* matrix, const uint32_t* list, uint32_t n_list, uint32_t n, uint32_t rw,
                             uint32_t i, uint32_t w) {
    const uint32_t valid = closure_valid(n, w);
    if (!valid) return 0u;
    const uint64_t slice = (uint64_t)n * rw, off = (uint64_t)i * rw + 2u * w;
    const bool two = 2u * w + 1u < rw;
    uint32_t a = 0;
    for (uint32_t k = 0; k < n_list; k++) {
        const uint32_t* base = matrix + list[k] * slice;
        a |= closure_bits(base[off], two ? base[off + 1u] : 0u);
    }
    return a & valid;
}

// what the lane that holds bit-word x of its row gives to the ballot of column k of the word
PG_HD bool dom_ballot_bit(uint32_t x, uint32_t k) { return (x >> k) & 1u; }

// bit v within word w of a row
PG_HD uint32_t dom_self(uint32_t v, uint32_t w) { return (v >> 5) == w ? 1u << (v & 31u) : 0u; }

// word w of an entry's row of Avoid (and of its first D): every column but its own, reached set
PG_HD uint32_t dom_entry_word(uint32_t n, uint32_t e, uint32_t w) { return closure_valid(dom_cols(n), w) & ~dom_self(e, w); }

// one round on one word of row v: what the products brought that Avoid(v) did not hold
PG_HD uint32_t dom_new(uint32_t acc, uint32_t avoid, uint32_t v, uint32_t w) { return acc & ~avoid & ~dom_self(v, w); }

// is v reached: column n of its Avoid row
PG_HD bool dom_reached(const uint32_t* avoid_row, uint32_t n) { return (avoid_row[n >> 5] >> (n & 31u)) & 1u; }

// word w of Dom(v) from the word of Avoid(v)
PG_HD uint32_t dom_word(uint32_t avoid, bool reached, uint32_t n, uint32_t w) { return reached ? ~avoid & closure_valid(n, w) : 0u; }

// the dominators of v form a chain with distinct sizes: k in Dom(v) \ {v} is the immediate one iff
PG_HD bool dom_is_idom(uint32_t size_k, uint32_t size_v) { return size_k + 1u == size_v; }

// the order of the top choke point: the largest cut, then the least end point (cut > 0)
PG_HD uint64_t dom_top_key(uint32_t cut, uint32_t v) { return (uint64_t)cut << 32 | (uint32_t)~v; }
PG_HD uint32_t dom_top_of(uint64_t key) { return key ? ~(uint32_t)key : kDomNone; }

// How the launches cut the work: a round (a workgroup owns tile_rows rows x tile_cols columns of Avoid,
// a lane lane_words adjacent bit-words: the narrowest of 1, 2, 4 at which one column tile covers the
// row, 4 beyond), the edge / transpose tiles, the cut tiles and the per-row kernels of the finish. The
// one function the launch, the host twin and pg_debug_reach_dominators_plan use. Host only.
struct DomPlan {
    uint32_t lane_words, tile_rows, tile_cols, row_tiles, col_tiles, round_grid;
    uint32_t t_rows, t_cols, t_row_tiles, t_col_tiles, t_grid;
    uint32_t cut_rows, cut_cols, cut_row_tiles, cut_col_tiles, cut_grid;
    uint32_t finish_grid;  // the most workgroups the size and idom kernels can need: one per row
};
inline DomPlan dom_plan(uint32_t n) {
    const uint32_t bw = dom_bit_words(n);
    const uint32_t lw = bw <= 64u ? 1u : bw <= 128u ? 2u : 4u;
    const uint32_t tile_words = 64u * lw;
    DomPlan p{};
    p.lane_words = lw, p.tile_rows = kDomTileRows, p.tile_cols = 32u * tile_words;
    p.row_tiles = (n + kDomTileRows - 1u) / kDomTileRows, p.col_tiles = (bw + tile_words - 1u) / tile_words;
    p.round_grid = p.row_tiles * p.col_tiles;
    p.t_rows = kDomTRows, p.t_cols = kDomTCols;
    p.t_row_tiles = (n + kDomTRows - 1u) / kDomTRows, p.t_col_tiles = (closure_stride(n) + kDomTWords - 1u) / kDomTWords;
    p.t_grid = p.t_row_tiles * p.t_col_tiles;
    p.cut_rows = kDomCutRows, p.cut_cols = 32u * kDomCutWords;
    p.cut_row_tiles = (n + kDomCutRows - 1u) / kDomCutRows;
    p.cut_col_tiles = (closure_bit_words(n) + kDomCutWords - 1u) / kDomCutWords;
    p.cut_grid = p.cut_row_tiles * p.cut_col_tiles;
    p.finish_grid = n;
    return p;
}

// device.hpp-style API of dominators.hip
struct DomSpecDev {
    const uint32_t* matrix;    // device
    uint32_t n, n_svc;         // n >= 1
    const uint32_t* svc_list;  // host: the selected slices, ascending
    uint32_t n_list;
    const uint32_t* entry;     // host: n_entry ids, each < n
    uint32_t n_entry;
};
struct DomResult {  // pg_reach_dominators_result
    uint32_t n_reached, n_chokes, top, top_cut, depth, rounds;
};
// out_dom / out_idom / out_cut device or null; *res host. 0, -1 (a HIP error) or -2 (the scratch
// allocation failed); synchronises the stream after every round and at the end
int dev_reach_dominators(uint32_t blocks_per_cu, const DomSpecDev& spec, uint32_t* out_dom, uint16_t* out_idom,
                         uint32_t* out_cut, DomResult* res, void* stream, std::string* err);

}  // namespace pg
