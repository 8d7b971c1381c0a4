// Reachability cost (pg_reach_cost): the cheapest walks from listed sources under per-end-point
// costs, their least predecessors, lengths and weighted choke points, over the ALLOW graph of a
// square pg_reach_matrix result, written once for both sides like cut.hpp -- the gfx950 kernel
// (cost.hip) and the host twin (pg_debug_reach_cost_host, tests only) run the same per-word code
// over the same plan.
//
// The input and the edge rule are the closure's (closure.hpp): i -> j when some selected slice holds
// PG_CONN_ALLOW in cell (i, j); cell (i, i) is a cell like any other; padding bits are masked
// (closure_valid), never trusted. weight[v] in 1..65535 is what it costs to take end point v.
//   cost(s, v)  the least sum of weight[p_t], t = 1..k, over walks s = p_0 -> .. -> p_k = v of k >= 1
//               edges: the source is held and costs nothing, cost(s, s) is the cheapest cycle through
//               s. At most n * 65535 < 2^31. With max_cost != 0 a cell is reached only when its cost
//               is <= max_cost; every prefix of a cheapest walk is cheaper, so dropping the candidates
//               above max_cost during the search equals filtering the unlimited answer.
//   base(s, p)  0 for p == s, else cost(s, p).
//   pred(s, v)  the least p with an edge p -> v, base(s, p) defined and base(s, p) + weight[v] ==
//               cost(s, v): pg_reach_paths' least predecessor, weighted.
//   path, len   v, pred(s, v), pred(s, pred(s, v)), .. up to the first predecessor equal to s; costs
//               strictly fall along it. len = its edges; its intermediates are its end points other than
//               the start and v.
//
// Push, then pull. The search is label-correcting by whole-frontier sweeps: every end point of the
// frontier offers base + weight[v] to the ends of its edges (cost_offer), a minimum keeps the least,
// and an end point whose cost fell joins the next frontier. After round r every cell whose cheapest
// walk has <= r edges is final whatever the order inside a round, so the loop ends within n rounds and
// its fixed point does not depend on the schedule; n + 1 bounds it. A push cannot name the *least*
// tying predecessor deterministically, so a pull pass over the rows of the transposed matrix does:
// cost_ties on every held predecessor, the first hit in ascending order. cost_walk then follows the
// predecessors of every reached cell for len and the intermediates.
//
// Working form: bit-words of 32 end points; a bit vector has closure_stride(n) words, padding zero.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#include "dominators.hpp"

namespace pg {

constexpr uint32_t kCostMaxN = kClosureMaxN, kCostMaxSvc = kClosureMaxSvc, kCostMaxSrc = 1u << 15, kCostMaxCells = 1u << 28;
constexpr uint32_t kCostNone = 0xFFFFFFFFu;
constexpr uint16_t kCostNoPred = 0xFFFFu;
// one workgroup of 16 waves per source at a time; a wave's 64 lanes read 1, 2 or 4 adjacent bit-words
// of a row each per step
constexpr uint32_t kCostBlock = 1024, kCostWaves = kCostBlock / 64;
constexpr uint32_t kCostLdsMax = 160u << 10;
// the control words of a workgroup behind its two bit vectors: the two "some cost fell" flags of the
// rounds, then per source the reached cells, the largest cost, the longest path, the intermediates
constexpr uint32_t kCostCtlWords = 8;
enum { kCostFlag0 = 0, kCostFlag1 = 1, kCostCtlReached = 2, kCostCtlMax = 3, kCostCtlLongest = 4, kCostCtlVia = 5 };

// what the end of an edge p -> v is offered: base(p) + weight[v]; false when max_cost drops it
PG_HD bool cost_offer(uint32_t base, uint32_t weight_v, uint32_t max_cost, uint32_t* nd) {
    *nd = base + weight_v;
    return !max_cost || *nd <= max_cost;
}
// base(s, p) from p's cell of the row
PG_HD uint32_t cost_base(uint32_t cost_p, uint32_t p, uint32_t s) { return p == s ? 0u : cost_p; }
// is v held when the search is over: reached, or the source. Exactly the p with base(s, p) defined
PG_HD bool cost_held(uint32_t cost_v, uint32_t v, uint32_t s) { return cost_v != kCostNone || v == s; }
// does a held p with an edge to v tie for pred(s, v)
PG_HD bool cost_ties(uint32_t base, uint32_t weight_v, uint32_t cost_v) { return base + weight_v == cost_v; }
// the end points of bit-word w, least first
PG_HD uint32_t cost_first(uint32_t x, uint32_t w) { return 32u * w + (uint32_t)__builtin_ctz(x); }

// The path of a reached cell (s, v) from its end: pred_at(u) gives pred(s, u), via(k) is called once
// per intermediate. -> len. `steps` (n) bounds the walk: reached only by broken predecessors, as is an
// id at or above n
template <class P, class V>
PG_HD uint32_t cost_walk(uint32_t v, uint32_t s, uint32_t n, P pred_at, V via) {
    uint32_t len = 0, u = v;
    for (uint32_t steps = n; steps; steps--) {
        const uint32_t p = pred_at(u);
        if (p >= n) break;
        len++;
        if (p == s) break;
        via(p);
        u = p;
    }
    return len;
}

// How the launch is laid out, from n and the budget ("cost_lds_bytes") alone: the adjacent bit-words
// of a row a lane reads per step (the narrowest of 1, 2, 4 at which one step covers the row, 4
// beyond, as closure_plan), the workgroup, its dynamic LDS -- always the two bit vectors and the
// control words; the cost row (n x u32) where it fits under the budget beside them, and then the
// weights (n x u16) where they fit in what is left: the weights are dropped first, then the row --
// and the edge / transpose tiles. The one function the launch, the host twin and
// pg_debug_reach_cost_plan use. Host only.
struct CostPlan {
    uint32_t lane_words, block, lds_bytes, row_in_lds, weights_in_lds;
    uint32_t t_rows, t_cols, t_row_tiles, t_col_tiles, t_grid;
};
PG_HD uint32_t cost_fixed_bytes(uint32_t n) { return 4u * (2u * closure_stride(n) + kCostCtlWords); }
PG_HD uint32_t cost_row_bytes(uint32_t n) { return 4u * ((n + 3u) & ~3u); }
PG_HD uint32_t cost_weight_bytes(uint32_t n) { return (2u * n + 15u) & ~15u; }
inline CostPlan cost_plan(uint32_t n, uint32_t lds_budget) {
    const uint32_t bw = closure_bit_words(n);
    CostPlan p{};
    p.lane_words = bw <= 64u ? 1u : bw <= 128u ? 2u : 4u;
    p.block = kCostBlock;
    const uint32_t fixed = cost_fixed_bytes(n);  // (at most 8224)
    uint32_t left = std::min(lds_budget, kCostLdsMax - fixed);
    if (cost_row_bytes(n) <= left) p.row_in_lds = 1, left -= cost_row_bytes(n);
    if (p.row_in_lds && cost_weight_bytes(n) <= left) p.weights_in_lds = 1;
    p.lds_bytes = fixed + (p.row_in_lds ? cost_row_bytes(n) : 0u) + (p.weights_in_lds ? cost_weight_bytes(n) : 0u);
    p.t_rows = kDomTRows, p.t_cols = kDomTCols;
    p.t_row_tiles = (n + kDomTRows - 1u) / kDomTRows, p.t_col_tiles = (closure_stride(n) + kDomTWords - 1u) / kDomTWords;
    p.t_grid = p.t_row_tiles * p.t_col_tiles;
    return p;
}

// device.hpp-style API of cost.hip
struct CostSpecDev {
    const uint32_t* matrix;    // device
    uint32_t n, n_svc;         // n >= 1
    const uint32_t* svc_list;  // host: the selected slices, ascending
    uint32_t n_list;
    const uint32_t* src;       // host: n_src >= 1 ids, each < n
    uint32_t n_src;
    const uint16_t* weight;    // host: n weights, each >= 1
    uint32_t max_cost;
};
struct CostKnobs {
    uint32_t blocks_per_cu, lds_bytes;  // lds_bytes: "cost_lds_bytes"
};
struct CostResult {  // pg_reach_cost_result
    uint64_t n_reached, n_via;
    uint32_t max_cost, longest;
};
// every output device or null; *res host. 0, -1 (a HIP error) or -2 (the scratch allocation failed);
// synchronises the stream once, at its end
int dev_reach_cost(const CostKnobs& knobs, const CostSpecDev& spec, uint32_t* out_cost, uint16_t* out_pred, uint16_t* out_len,
                   uint32_t* out_via, CostResult* res, void* stream, std::string* err);

}  // namespace pg
