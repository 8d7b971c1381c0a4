// Reachability cut (pg_reach_cut): the fewest end points whose quarantine leaves no route from an
// entry set E to a target set T, over the ALLOW graph of a square pg_reach_matrix result, written
// once for both sides like dominators.hpp -- the gfx950 kernels (cut.hip) and the host twin
// (pg_debug_reach_cut_host, tests only) run the same per-word code over the same plan.
//
// The input and the edge rule are the closure's (closure.hpp): i -> j when some selected slice holds
// PG_CONN_ALLOW in cell (i, j); padding bits are masked (closure_valid), never trusted. Self edges,
// edges into members of E and edges out of members of T never matter and nothing below sees them.
//   separates   a set C of end points outside E u T separates when no walk leads from a member of E
//               to a member of T in the graph without C.
//   inseparable E n T is not empty or some edge e -> t joins them directly. n_direct counts the
//               distinct pairs (e, t) with e == t or an edge e -> t.
//   cut_size    the least |C| over separating C. By Menger's theorem the largest number of E -> T
//               paths that share no end point outside E u T; each has the form e, interior end
//               points outside E u T, t.
//   near, far   among the minimum cuts exactly one has a retained region Reach(C) -- the end points
//               reachable from E without C, E included -- that lies inside that of every other: the
//               near cut, the quarantine closest to the attacker. Exactly one minimises the region
//               that can still reach T in the same sense: the far cut. Both are properties of the
//               graph, not of the algorithm.
//   capped      max_cut bounds the search: it stops as soon as max_cut + 1 disjoint paths exist, and
//               the paths are the proof that no cut of that size exists.
//
// Split graph: every v outside E u T becomes v_in -> v_out of capacity 1, an edge u -> v becomes
// u_out -> v_in of unbounded capacity, the source feeds every e_out, every t_in feeds the sink. After
// any maximum flow
//   near = { v : v_in is residual-reachable from the source, v_out is not }
//   far  = { v : v_out residual-reaches the sink, v_in does not }
// (the residual-reachable sets of a maximum flow do not depend on which maximum flow it is).
//
// The flow is a set of paths, kept per interior end point as its predecessor and successor (prev,
// next; kCutNone off the paths; an interior end point carries flow iff next != kCutNone). Shortest
// augmenting paths, one per search, each search level by level over bit sets. One level follows one
// residual arc from every half reached at the level before -- four kinds:
//   edge      u_out -> v_in for an edge u -> v, always; the only step that touches the matrix. Pull
//             form: v_in takes the least u of the frontier with an edge to it (cut_scan_word,
//             cut_first) -- the parent rule "least id"
//   forward   v_in -> v_out, v without flow
//   back      v_out -> v_in, v with flow (the internal arc of an end point that carries flow)
//   edge-back v_in -> u_out, u = prev[v] (the edge arc to its flow predecessor)
// Where a half is reached by two arcs in one level, the back arc wins over the edge arc. When several
// targets are reached at the same level the least id wins. cut_augment walks the parents from that
// target, flips the flow and counts the back and edge-back arcs: `reroutes`.
//
// The same level runs every search of the call, with the roles handed in (CutLevel):
//   forward   X = in halves, Y = out halves, the rows of the transposed edge matrix, link = next.
//             X blocked for E, Y blocked for T, Y of E the first frontier
//   backward  from the sink: X = out halves, Y = in halves, the rows of the edge matrix, link = prev.
//             X blocked for T, Y blocked for E, Y of T the first frontier
//   plain     Reach(C): one bit per end point (Y mirrors X), edge arcs only, E u C blocked, E the
//             first frontier
// `levels` counts every level of every search of the call.
//
// Working form: bit-words of 32 end points; a bit vector has closure_stride(n) words, padding zero.
#pragma once
#include <cstdint>
#include <string>

#include "dominators.hpp"

namespace pg {

constexpr uint32_t kCutMaxN = kClosureMaxN, kCutMaxSvc = kClosureMaxSvc, kCutMaxList = 1u << 15, kCutMaxCut = 1u << 15;
constexpr uint32_t kCutNoSize = 0xFFFFFFFFu;
constexpr uint16_t kCutNone = 0xFFFFu;
// out_cut's flags
constexpr uint8_t kCutNear = 1, kCutFar = 2, kCutNearReach = 4, kCutFarReach = 8;
// a level's workgroup of 16 waves owns the 32 end points of one bit-word, two per wave; a wave's 64
// lanes read 1, 2 or 4 adjacent bit-words of a row each per step
constexpr uint32_t kCutLevelBlock = 1024, kCutWaves = kCutLevelBlock / 64, kCutGroupNodes = 32, kCutWaveNodes = kCutGroupNodes / kCutWaves;
static_assert(kCutWaveNodes == 2, "a workgroup owns one bit-word of every bit vector");
constexpr uint32_t kCutFinishBlock = 1024;
static_assert(kCutMaxN / 32u <= kCutFinishBlock, "the finish holds a bit vector at a word per thread");
// a level's status: {0 = nothing grew, the least target reached or kCutNoTarget}; two slots, a level
// clears the slot of the next
constexpr uint32_t kCutNoTarget = 0xFFFFFFFFu, kCutStatusWords = 4;
// the words of a search state's head: X reached, Y reached, Y frontier, X frontier, the status slots
PG_HD uint32_t cut_head_words(uint32_t stride) { return 4u * stride + kCutStatusWords; }
// the result words in scratch: n_direct, reroutes, |near|, |far|, |Reach(near)|, |Reach(far)|
constexpr uint32_t kCutResultWords = 6;

PG_HD bool cut_bit(const uint32_t* vec, uint32_t v) { return (vec[v >> 5] >> (v & 31u)) & 1u; }

// word w of row v of the level's matrix against the same word of the frontier: the frontier's end
// points with an edge arc to v, v itself never
PG_HD uint32_t cut_scan_word(uint32_t m, uint32_t f, uint32_t v, uint32_t w) { return m & f & ~dom_self(v, w); }
// the least end point of a non-zero scan word
PG_HD uint32_t cut_first(uint32_t x, uint32_t w) { return 32u * w + (uint32_t)__builtin_ctz(x); }

// the back arc into X of v: v carries flow and its Y half is in the frontier
PG_HD bool cut_x_back(uint16_t link_v, bool y_front) { return link_v != kCutNone && y_front; }
// where the Y half of v is reached from: its own X half without flow (forward), else the X half of
// its link (edge-back)
PG_HD uint32_t cut_y_source(uint16_t link_v, uint32_t v) { return link_v == kCutNone ? v : link_v; }

// word w of the pairs of entry e: its edges and itself, against the targets
PG_HD uint32_t cut_direct_word(uint32_t a, uint32_t t, uint32_t e, uint32_t w) { return (a | dom_self(e, w)) & t; }

// the canonical cuts from the residual searches: (in, out) reached from the source; (out, in) that
// reach the sink; e and t are the words of E and T
PG_HD uint32_t cut_near_word(uint32_t s_in, uint32_t s_out, uint32_t e, uint32_t t) { return s_in & ~s_out & ~e & ~t; }
PG_HD uint32_t cut_far_word(uint32_t b_out, uint32_t b_in, uint32_t e, uint32_t t) { return b_out & ~b_in & ~e & ~t; }
// Reach(C) from the plain search's reached word, in which C was blocked
PG_HD uint32_t cut_reach_word(uint32_t reached, uint32_t c) { return reached & ~c; }
PG_HD uint8_t cut_flags(bool near, bool far, bool near_reach, bool far_reach) {
    return (uint8_t)((near ? kCutNear : 0) | (far ? kCutFar : 0) | (near_reach ? kCutNearReach : 0) | (far_reach ? kCutFarReach : 0));
}

// One augmentation: from the in half of target t along the parents of the forward search (p_in[v]:
// the u of the edge arc u_out -> v_in, or v itself for the back arc; p_out[v]: v itself for the
// forward arc, else the w of the edge-back arc w_in -> v_out) to an entry, the flow flipped on the way.
// -> the back and edge-back arcs on the path. `steps` bounds the walk (2 n + 2 halves: reached only
// by broken parents)
PG_HD uint32_t cut_augment(uint32_t t, const uint16_t* p_in, const uint16_t* p_out, const uint32_t* e_bits, const uint32_t* t_bits,
                           uint16_t* prev, uint16_t* next, uint32_t steps) {
    uint32_t reroutes = 0, v = t;
    bool in = true;
    for (; steps; steps--) {
        if (in) {
            const uint32_t p = p_in[v];
            if (p == v) {  // back: v gives up its flow, both neighbours follow on the path
                prev[v] = kCutNone, next[v] = kCutNone;
                reroutes++, in = false;
                continue;
            }
            const bool v_inner = !cut_bit(e_bits, v) && !cut_bit(t_bits, v);
            if (v_inner) prev[v] = (uint16_t)p;
            if (cut_bit(e_bits, p)) break;
            next[p] = (uint16_t)v;
            v = p, in = false;
        } else {
            const uint32_t q = p_out[v];
            if (q != v) reroutes++, v = q;  // edge-back: the flow v -> q goes; what q gets follows on the path
            in = true;
        }
    }
    return reroutes;
}

// How the launches cut the work: a level (a workgroup of `level_block` threads owns group_nodes end
// points, a lane reads lane_words adjacent bit-words of a row per step: the narrowest of 1, 2, 4 at
// which one step covers the row, 4 beyond; row_steps of them cover a row), the edge / transpose tiles
// and the finish. The one function the launch, the host twin and pg_debug_reach_cut_plan use. Host only.
struct CutPlan {
    uint32_t lane_words, level_block, group_nodes, row_steps, level_grid;
    uint32_t t_rows, t_cols, t_row_tiles, t_col_tiles, t_grid;
    uint32_t finish_block, finish_grid;
};
inline CutPlan cut_plan(uint32_t n) {
    const uint32_t bw = closure_bit_words(n);
    const uint32_t lw = bw <= 64u ? 1u : bw <= 128u ? 2u : 4u;
    CutPlan p{};
    p.lane_words = lw, p.level_block = kCutLevelBlock, p.group_nodes = kCutGroupNodes;
    p.row_steps = (bw + 64u * lw - 1u) / (64u * lw), p.level_grid = bw;
    p.t_rows = kDomTRows, p.t_cols = kDomTCols;
    p.t_row_tiles = (n + kDomTRows - 1u) / kDomTRows, p.t_col_tiles = (closure_stride(n) + kDomTWords - 1u) / kDomTWords;
    p.t_grid = p.t_row_tiles * p.t_col_tiles;
    p.finish_block = kCutFinishBlock, p.finish_grid = 1;
    return p;
}

// device.hpp-style API of cut.hip
struct CutSpecDev {
    const uint32_t* matrix;    // device
    uint32_t n, n_svc;         // n >= 1
    const uint32_t* svc_list;  // host: the selected slices, ascending
    uint32_t n_list;
    const uint32_t* entry;     // host: the distinct entries, ascending
    uint32_t n_entry;
    const uint32_t* e_bits;    // host: E and T as bit vectors of closure_stride(n) words
    const uint32_t* t_bits;
    uint32_t max_cut;
};
struct CutResult {  // pg_reach_cut_result
    uint32_t separable, capped, n_direct, cut_size, n_paths, near_reach, far_reach, levels, reroutes;
};
// out_cut / out_prev / out_next device or null; *res host. 0, -1 (a HIP error) or -2 (the scratch
// allocation failed); synchronises the stream after every level and at the end
int dev_reach_cut(uint32_t blocks_per_cu, const CutSpecDev& spec, uint8_t* out_cut, uint16_t* out_prev, uint16_t* out_next,
                  CutResult* res, void* stream, std::string* err);

}  // namespace pg
