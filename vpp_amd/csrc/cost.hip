// gfx950 kernels of the reachability cost (pg_reach_cost; cost.hpp has the definitions, the per-word
// code and the plan).
//
// One scratch block: A and ET (n x closure_stride(n) bit-words: bit j of A[i] and bit i of ET[j] say
// i -> j), the result words, the lists and the weights (one copy in), and per workgroup a row of
// predecessors when out_pred is null and a cost row when the plan gives it no LDS and out_cost is null.
//  k_edges_t    edge_tiles.hpp, shared with dominators.hip and cut.hip: A, and ET through LDS ballots.
//  k_cost_rows  the sources cut into one contiguous run per resident workgroup (run_grid). A workgroup
//               of 16 waves takes one source at a time and runs its whole search inside the launch:
//               no host read and no launch per round. In LDS: two frontier bit vectors, the control
//               words, the cost row (n x u32) and the weights (n x u16) where the plan fits them.
//                 relax   wave k owns the end points p with p % 16 == k: every wave scans the frontier
//                         words masked to its two bits of each, so a frontier of adjacent end points is
//                         spread over all waves. For such a p the lanes read LW adjacent words of row p
//                         of A each (one aligned 4-, 8- or 16-B load) and offer base + weight[v] to every
//                         set bit v (cost_offer): a plain read of cost[v] skips what does not improve,
//                         else an atomic min, and where that returned more an atomic OR of v into the
//                         next frontier and a store to the round's flag. A barrier; everyone reads the
//                         flag and leaves together or clears, swaps and meets at a second barrier. The
//                         flag has two slots: a round clears the slot of the next. n + 1 rounds at most.
//                 store   a wave per 64 end points: out_cost, the counts, and by one ballot the bit
//                         vector of the held end points (cost_held) over the first frontier vector.
//                 pull    a wave per target v: the lanes AND LW words of row v of ET with the held bits
//                         and test their end points in ascending order (cost_ties); a ballot finds the
//                         first lane with a hit: the least predecessor. Rows go to out_pred or scratch.
//                 walk    after a barrier, which makes the workgroup's own global stores visible to it,
//                         a lane per reached v follows the predecessors (cost_walk): out_len, and one
//                         add per intermediate into n counters that reuse the cost row's LDS; the
//                         non-zero ones are flushed with global atomic adds.
//               The counts and maxima of a source leave with one atomic each per workgroup.
//               Without an LDS row the same code keeps the row in out_cost (or scratch) through
//               agent-scope loads and global atomics, and the intermediates go straight to out_via.
// Every barrier is reached by the whole workgroup: the source loop, the round loop and its exit are
// uniform in it. No kernel waits on another workgroup. Integer minima and sums: the same bytes on
// every run.
//
// No kernel reads a table or touches a hit counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "audit_launch.hpp"
#include "cost.hpp"
#include "edge_tiles.hpp"

namespace pg {

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
    for (int d = 32; d; d >>= 1) x = max(x, (uint32_t)__shfl_xor(x, d, 64));
    return x;
}

// LW adjacent words at a pointer aligned to LW words: one 4-, 8- or 16-B access
template <uint32_t LW>
__device__ __forceinline__ void load_words(const uint32_t* p, uint32_t (&v)[LW]) {
    if constexpr (LW == 4) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else if constexpr (LW == 2) {
        const uint2 q = *reinterpret_cast<const uint2*>(p);
        v[0] = q.x, v[1] = q.y;
    } else {
        v[0] = *p;
    }
}

// a cell of the cost row: in LDS plainly; in global memory past the L1, which the atomics do not go through
template <bool ROW_LDS>
__device__ __forceinline__ uint32_t row_get(const uint32_t* row, uint32_t v) {
    if constexpr (ROW_LDS) return row[v];
    else return __hip_atomic_load(row + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool ROW_LDS>
__device__ __forceinline__ void row_set(uint32_t* row, uint32_t v, uint32_t x) {
    if constexpr (ROW_LDS) row[v] = x;
    else __hip_atomic_store(row + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a predecessor another wave of the workgroup stored before the last barrier
__device__ __forceinline__ uint32_t pred_get(const uint16_t* pred, uint32_t v) {
    return __hip_atomic_load(pred + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

struct CostArgs {
    const uint32_t *A, *ET;
    const uint16_t* weight;
    const uint32_t* src;
    uint32_t* out_cost;  // the outputs, or null
    uint16_t* out_pred;
    uint16_t* out_len;
    uint32_t* out_via;
    uint32_t* rows;      // a row per workgroup: the cost row when it has neither LDS nor out_cost
    uint16_t* preds;     // a row per workgroup: the predecessors when out_pred is null
    unsigned long long* sums;  // n_reached, n_via
    uint32_t* maxima;          // max_cost, longest
    uint32_t n, stride, n_src, per, max_cost;
};

template <uint32_t LW, bool ROW_LDS, bool W_LDS>
__global__ __launch_bounds__(kCostBlock) void k_cost_rows(CostArgs a) {
    constexpr uint32_t kStep = 64u * LW;
    // [frontier | next frontier | control words | cost row | weights] (cost_plan)
    extern __shared__ __attribute__((aligned(16))) uint32_t cost_lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t n = a.n, stride = a.stride, bw = closure_bit_words(n);
    uint32_t* const ctl = cost_lds + 2u * stride;
    uint32_t* const lds_row = ctl + kCostCtlWords;
    const uint16_t* wts = a.weight;
    if constexpr (W_LDS) {
        uint16_t* staged = reinterpret_cast<uint16_t*>(lds_row + ((n + 3u) & ~3u));
        for (uint32_t v = threadIdx.x; v < n; v += kCostBlock) staged[v] = a.weight[v];
        wts = staged;
    }
    const uint32_t q0 = blockIdx.x * a.per, q1 = min(q0 + a.per, a.n_src);
    for (uint32_t q = q0; q < q1; q++) {
        const uint32_t s = __builtin_amdgcn_readfirstlane(a.src[q]);
        if (s >= n) continue;  // (checked on the host; uniform in the workgroup)
        uint32_t* row;
        if constexpr (ROW_LDS) row = lds_row;
        else row = a.out_cost ? a.out_cost + (size_t)q * n : a.rows + (size_t)blockIdx.x * n;
        uint16_t* const pred = a.out_pred ? a.out_pred + (size_t)q * n : a.preds + (size_t)blockIdx.x * n;

        for (uint32_t v = threadIdx.x; v < n; v += kCostBlock) row_set<ROW_LDS>(row, v, kCostNone);
        for (uint32_t w = threadIdx.x; w < stride; w += kCostBlock) cost_lds[w] = dom_self(s, w), cost_lds[stride + w] = 0u;
        if (threadIdx.x < kCostCtlWords) ctl[threadIdx.x] = 0u;
        __syncthreads();

        // ---- relax: the source is the first frontier, its base 0 ----
        uint32_t fo = 0, no = stride;
        const uint32_t mine = 0x00010001u << wave;
        for (uint32_t round = 0; round <= n; round++) {
            for (uint32_t b0 = 0; b0 < bw; b0 += 64u) {
                const uint32_t fw = b0 + lane;
                const uint32_t x = fw < bw ? cost_lds[fo + fw] & mine : 0u;
                unsigned long long some = __ballot(x != 0u);
                while (some) {  // (uniform in the wave)
                    const int from = __builtin_ctzll(some);
                    some &= some - 1ull;
                    uint32_t px = __builtin_amdgcn_readfirstlane((uint32_t)__shfl((int)x, from, 64));
                    for (; px; px &= px - 1u) {
                        const uint32_t p = cost_first(px, b0 + (uint32_t)from);  // (< n: the frontier has no padding bit)
                        const uint32_t d = cost_base(__builtin_amdgcn_readfirstlane(row_get<ROW_LDS>(row, p)), p, s);
                        const uint32_t* arow = a.A + (size_t)p * stride;
                        for (uint32_t base = 0; base < bw; base += kStep) {
                            const uint32_t w0 = base + lane * LW;
                            if (w0 >= stride) continue;  // (stride is a multiple of 4: all LW words or none)
                            uint32_t m[LW];
                            load_words<LW>(arow + w0, m);
#pragma unroll
                            for (uint32_t k = 0; k < LW; k++)
                                for (uint32_t e = m[k]; e; e &= e - 1u) {
                                    const uint32_t v = cost_first(e, w0 + k);  // (< n: A's padding is zero)
                                    uint32_t nd;
                                    if (!cost_offer(d, wts[v], a.max_cost, &nd)) continue;
                                    if (nd >= row_get<ROW_LDS>(row, v)) continue;
                                    if (atomicMin(&row[v], nd) > nd) {
                                        atomicOr(&cost_lds[no + (v >> 5)], 1u << (v & 31u));
                                        ctl[round & 1u] = 1u;
                                    }
                                }
                        }
                    }
                }
            }
            __syncthreads();
            // one flag, read by everyone after the barrier: the whole workgroup leaves or stays
            if (!ctl[round & 1u]) break;
            for (uint32_t w = threadIdx.x; w < stride; w += kCostBlock) cost_lds[fo + w] = 0u;
            if (threadIdx.x == 0) ctl[(round + 1u) & 1u] = 0u;
            const uint32_t t = fo;
            fo = no, no = t;
            __syncthreads();
        }

        // ---- store: out_cost, the counts, the held bits over the first vector ----
        {
            uint32_t cnt = 0, mx = 0;
            for (uint32_t v0 = 64u * wave; v0 < 32u * stride; v0 += kCostBlock) {
                const uint32_t v = v0 + lane;
                const uint32_t c = v < n ? row_get<ROW_LDS>(row, v) : kCostNone;
                if constexpr (ROW_LDS)
                    if (a.out_cost && v < n) a.out_cost[(size_t)q * n + v] = c;
                if (c != kCostNone) cnt++, mx = max(mx, c);
                const unsigned long long held = __ballot(v < n && cost_held(c, v, s));
                // (32 * stride is a multiple of 128: both words are inside the vector)
                if (lane == 0) cost_lds[v0 >> 5] = (uint32_t)held, cost_lds[(v0 >> 5) + 1u] = (uint32_t)(held >> 32);
            }
            cnt = wave_sum(cnt), mx = wave_max(mx);
            if (lane == 0) {
                if (cnt) atomicAdd(&ctl[kCostCtlReached], cnt);
                if (mx) atomicMax(&ctl[kCostCtlMax], mx);
            }
        }
        __syncthreads();

        // ---- pull: the least tying predecessor of every reached end point ----
        for (uint32_t v = wave; v < n; v += kCostWaves) {
            const uint32_t cv = __builtin_amdgcn_readfirstlane(row_get<ROW_LDS>(row, v));
            uint32_t pv = kCostNoPred;
            if (cv != kCostNone) {  // (uniform in the wave)
                const uint32_t wv = wts[v];
                const uint32_t* trow = a.ET + (size_t)v * stride;
                for (uint32_t base = 0; base < bw; base += kStep) {
                    const uint32_t w0 = base + lane * LW;
                    uint32_t found = kCostNone;
                    if (w0 < stride) {
                        uint32_t m[LW], h[LW];
                        load_words<LW>(trow + w0, m);
                        load_words<LW>(&cost_lds[w0], h);
#pragma unroll
                        for (uint32_t k = 0; k < LW; k++)
                            for (uint32_t e = m[k] & h[k]; e && found == kCostNone; e &= e - 1u) {
                                const uint32_t p = cost_first(e, w0 + k);
                                if (cost_ties(cost_base(row_get<ROW_LDS>(row, p), p, s), wv, cv)) found = p;
                            }
                    }
                    const unsigned long long hit = __ballot(found != kCostNone);
                    if (hit) {  // (uniform in the wave; the lanes hold ascending words: the first lane has the least)
                        pv = (uint32_t)__shfl((int)found, (int)__builtin_ctzll(hit), 64);
                        break;
                    }
                }
            }
            if (lane == 0) pred[v] = (uint16_t)pv;
        }
        __syncthreads();

        // ---- walk: len, and the intermediates into the counters that take the cost row's place ----
        if constexpr (ROW_LDS) {
            if (a.out_via) {
                for (uint32_t v = threadIdx.x; v < n; v += kCostBlock) row[v] = 0u;
                __syncthreads();  // (a.out_via is uniform)
            }
        }
        {
            uint32_t longest = 0, vias = 0;
            for (uint32_t v = threadIdx.x; v < n; v += kCostBlock) {
                uint32_t len = 0;
                if (pred_get(pred, v) != kCostNoPred) {
                    len = cost_walk(
                        v, s, n, [&](uint32_t u) { return pred_get(pred, u); },
                        [&](uint32_t k) {
                            if (!a.out_via) return;
                            if constexpr (ROW_LDS) atomicAdd(&row[k], 1u);
                            else atomicAdd(&a.out_via[k], 1u);
                        });
                    vias += len - 1u, longest = max(longest, len);
                }
                if (a.out_len) a.out_len[(size_t)q * n + v] = (uint16_t)len;
            }
            vias = wave_sum(vias), longest = wave_max(longest);
            if (lane == 0) {
                if (vias) atomicAdd(&ctl[kCostCtlVia], vias);
                if (longest) atomicMax(&ctl[kCostCtlLongest], longest);
            }
        }
        __syncthreads();
        if constexpr (ROW_LDS) {
            if (a.out_via)
                for (uint32_t k = threadIdx.x; k < n; k += kCostBlock)
                    if (const uint32_t c = row[k]) atomicAdd(&a.out_via[k], c);
        }
        if (threadIdx.x == 0) {
            if (ctl[kCostCtlReached]) atomicAdd(&a.sums[0], (unsigned long long)ctl[kCostCtlReached]);
            if (ctl[kCostCtlVia]) atomicAdd(&a.sums[1], (unsigned long long)ctl[kCostCtlVia]);
            if (ctl[kCostCtlMax]) atomicMax(&a.maxima[0], ctl[kCostCtlMax]);
            if (ctl[kCostCtlLongest]) atomicMax(&a.maxima[1], ctl[kCostCtlLongest]);
        }
        __syncthreads();  // (the next source starts over the same LDS)
    }
}

template <uint32_t LW, class F>
void with_row(const CostPlan& p, F f) {
    if (p.weights_in_lds) f(k_cost_rows<LW, true, true>);
    else if (p.row_in_lds) f(k_cost_rows<LW, true, false>);
    else f(k_cost_rows<LW, false, false>);
}
template <class F>
void with_kernel(const CostPlan& p, F f) {
    if (p.lane_words == 1) with_row<1>(p, f);
    else if (p.lane_words == 2) with_row<2>(p, f);
    else with_row<4>(p, f);
}

}  // namespace

int dev_reach_cost(const CostKnobs& knobs, const CostSpecDev& spec, uint32_t* out_cost, uint16_t* out_pred, uint16_t* out_len,
                   uint32_t* out_via, CostResult* res, void* stream, std::string* err) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = spec.n, stride = closure_stride(n), rw = (n + 15u) / 16u;
    if (!spec.n_src) {  // nothing to search: out_via is still every word written
        if (out_via) HIPCHK(hipMemsetAsync(out_via, 0, (size_t)n * sizeof(uint32_t), st));
        HIPCHK(hipStreamSynchronize(st));
        *res = CostResult{0, 0, 0, 0};
        return 0;
    }
    const CostPlan p = cost_plan(n, knobs.lds_bytes);
    // the run of sources of a workgroup, before the scratch: the per-workgroup rows depend on it
    Runs runs{};
    hipError_t e = hipSuccess;
    with_kernel(p, [&](auto kernel) {
        e = allow_dynamic_lds(kernel, p.lds_bytes);
        if (e == hipSuccess) runs = run_grid(kernel, (int)kCostBlock, p.lds_bytes, spec.n_src, knobs.blocks_per_cu);
    });
    HIPCHK(e);
    // (before blk: a call that leaves early still outlives the copies from and into them)
    struct Back {
        unsigned long long sums[2];
        uint32_t maxima[2];
    } back{};
    std::vector<unsigned char> h;  // the host image of LIST .. WEIGHT
    Scratch blk;
    enum { RESULT, MAT_A, MAT_ET, ROWS, PREDS, LIST, SRC, WEIGHT, END };
    const size_t mat = (size_t)n * stride * sizeof(uint32_t);
    const size_t rows = !p.row_in_lds && !out_cost ? (size_t)runs.groups * n * sizeof(uint32_t) : 0;
    const size_t preds = !out_pred ? (size_t)runs.groups * n * sizeof(uint16_t) : 0;
    const auto l = lay_out({sizeof(Back), mat, mat, rows, preds, spec.n_list * sizeof(uint32_t), spec.n_src * sizeof(uint32_t),
                            n * sizeof(uint16_t), 0});
    if (Scratch::make(&blk, l.total, err) != 0) {
        (void)hipGetLastError();
        return -2;
    }
    h.assign(l.off[END] - l.off[LIST], 0);
    l.put(h, LIST, LIST, spec.svc_list, spec.n_list);
    l.put(h, LIST, SRC, spec.src, spec.n_src);
    l.put(h, LIST, WEIGHT, spec.weight, n);
    unsigned char* d_res = l.at<unsigned char>(blk, RESULT);
    uint32_t *A = l.at<uint32_t>(blk, MAT_A), *ET = l.at<uint32_t>(blk, MAT_ET), *list = l.at<uint32_t>(blk, LIST);
    HIPCHK(hipMemsetAsync(d_res, 0, sizeof(Back), st));
    if (out_via) HIPCHK(hipMemsetAsync(out_via, 0, (size_t)n * sizeof(uint32_t), st));
    HIPCHK(hipMemcpyAsync(list, h.data(), h.size(), hipMemcpyHostToDevice, st));

    EdgeTiles S{p.t_col_tiles, p.t_grid, 0};
    const Runs tiles = run_grid(k_edges_t<true, false>, (int)kDomBlock, 0, S.items, knobs.blocks_per_cu);
    S.per = (uint32_t)tiles.per;
    hipLaunchKernelGGL((k_edges_t<true, false>), dim3((uint32_t)tiles.groups), dim3(kDomBlock), 0, st, spec.matrix, list, spec.n_list, n, rw,
                       stride, S, A, ET, (uint32_t*)nullptr);
    HIPCHK(hipGetLastError());

    CostArgs a{};
    a.A = A, a.ET = ET, a.weight = l.at<uint16_t>(blk, WEIGHT), a.src = l.at<uint32_t>(blk, SRC);
    a.out_cost = out_cost, a.out_pred = out_pred, a.out_len = out_len, a.out_via = out_via;
    a.rows = l.at<uint32_t>(blk, ROWS), a.preds = l.at<uint16_t>(blk, PREDS);
    a.sums = reinterpret_cast<unsigned long long*>(d_res), a.maxima = reinterpret_cast<uint32_t*>(d_res + offsetof(Back, maxima));
    a.n = n, a.stride = stride, a.n_src = spec.n_src, a.per = (uint32_t)runs.per, a.max_cost = spec.max_cost;
    with_kernel(p, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((uint32_t)runs.groups), dim3(kCostBlock), p.lds_bytes, st, a);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&back, d_res, sizeof(Back), hipMemcpyDeviceToHost, st));
    if (blk.finish(st, "reach cost", err) != 0) return -1;
    *res = CostResult{back.sums[0], back.sums[1], back.maxima[0], back.maxima[1]};
    return 0;
}

}  // namespace pg
