// gfx950 kernels of the reachability paths (pg_reach_paths; paths.hpp has the per-word code, the
// partition and the plan).
//
//  k_paths_edges_t  the transposed edge bit matrix ET in scratch. A workgroup takes 64 columns x 128
//                   rows of hops: a lane owns one column and its wave 32 rows, so every load is one
//                   row segment of 64 adjacent cells and no lane reads down a column. The lane
//                   collects the 32 compares into one bit-word; the four waves' words of a column meet
//                   in LDS and leave as one 16-B store. Every word of ET is written, padding zero.
//  k_paths_walk     the work items (src, chunk of queries) in order, cut into one contiguous run per
//                   workgroup, the grid the resident workgroups. Per item the workgroup stages row
//                   src of hops in LDS (16-B loads over the aligned body of the row, 2-B loads at its
//                   head and tail; the staged row sits at the global row's offset inside 16 B, so the
//                   LDS stores are aligned too) unless the item before had the same src. A wave then
//                   takes every fourth query of the item. For one step it reads ET[p_t] in passes of
//                   64 adjacent bit-words, one per lane, walks its word's set bits from the least and
//                   compares row[k] in LDS with t - 1 (paths_word_pred); the lowest lane with a match
//                   holds the least k of the pass, and the first pass with a match ends the step. Lane
//                   0 stores the node and counts it for out_via; the 0xFFFF tail follows the walk.
//                   out_via: up to kPathsViaLdsMaxN end points the workgroup counts in n words of LDS
//                   and adds its non-zero words to out_via once, at its end (a cluster's paths meet in
//                   a few hubs: millions of global adds to a handful of words otherwise); beyond, the
//                   words do not fit beside the row and lane 0 adds to out_via directly. The result's
//                   counters stay in scalar registers and go through LDS once, at the workgroup's end:
//                   one add per counter and workgroup.
// No workgroup waits on another; out_via and the counters are cleared on the stream first.
//
// No kernel reads a table or touches a hit counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "audit_launch.hpp"
#include "paths.hpp"

namespace pg {

namespace {

__global__ __launch_bounds__(kPathsBlock) void k_paths_edges_t(const uint16_t* __restrict__ hops, uint32_t n, uint32_t stride,
                                                               uint32_t* __restrict__ ET) {
    __shared__ __attribute__((aligned(16))) uint32_t sh[kPathsEdgeCols][kPathsEdgeWords];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * kPathsEdgeCols + lane;
    const uint32_t w0 = blockIdx.y * kPathsEdgeWords;  // (stride is a multiple of 4: w0 + 3 < stride)
    sh[lane][wave] = c < n ? paths_edge_word(hops, n, c, w0 + wave) : 0u;
    __syncthreads();
    const uint32_t co = blockIdx.x * kPathsEdgeCols + threadIdx.x;
    if (threadIdx.x < kPathsEdgeCols && co < n)
        *reinterpret_cast<uint4*>(ET + (size_t)co * stride + w0) = *reinterpret_cast<const uint4*>(&sh[threadIdx.x][0]);
}

struct PathsShape {
    uint32_t n, stride, bit_words, max_len;
    uint32_t n_items, per;  // all work items; those of one workgroup
    uint32_t row_bytes;     // of the LDS block: the staged row; the waves' counters follow, then the via words
};
constexpr int kViaNone = 0, kViaGlobal = 1, kViaLds = 2;

// row `g` of hops (n cells, 2-B aligned) into LDS -> where cell 0 lies: `lds` is 16-B aligned, and the
// row keeps its global offset inside 16 B
__device__ __forceinline__ const uint16_t* stage_row(uint16_t* lds, const uint16_t* __restrict__ g, uint32_t n) {
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(g) & 15u) / 2u;
    uint16_t* row = lds + shift;
    const uint32_t head = min(n, (8u - shift) & 7u), body = (n - head) / 8u;
    if (threadIdx.x < head) row[threadIdx.x] = g[threadIdx.x];
    const uint4* gb = reinterpret_cast<const uint4*>(g + head);
    uint4* lb = reinterpret_cast<uint4*>(row + head);
    for (uint32_t m = threadIdx.x; m < body; m += kPathsBlock) lb[m] = gb[m];
    for (uint32_t k = head + 8u * body + threadIdx.x; k < n; k += kPathsBlock) row[k] = g[k];  // (at most 7)
    return row;
}

template <bool NODES, int VIA>
__global__ __launch_bounds__(kPathsBlock) void k_paths_walk(const uint16_t* __restrict__ hops, const uint32_t* __restrict__ ET,
                                                            PathsShape S, const PathsItem* __restrict__ items,
                                                            const uint32_t* __restrict__ dst, const uint32_t* __restrict__ pos,
                                                            uint16_t* __restrict__ out_len, uint16_t* __restrict__ out_nodes,
                                                            uint32_t* __restrict__ out_via,
                                                            unsigned long long* __restrict__ result) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    uint16_t* lds_row = reinterpret_cast<uint16_t*>(lds);
    uint32_t* via_lds = reinterpret_cast<uint32_t*>(lds + S.row_bytes + kPathsWaves * kPathsResultWords * sizeof(uint64_t));
    if constexpr (VIA == kViaLds)  // (the first item's barriers stand between this and the first add)
        for (uint32_t i = threadIdx.x; i < S.n; i += kPathsBlock) via_lds[i] = 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t it0 = blockIdx.x * S.per, it1 = min(it0 + S.per, S.n_items);
    // (wave-uniform: scalar registers)
    uint32_t n_found = 0, n_unreachable = 0, n_too_long = 0, n_broken = 0, longest = 0;
    uint64_t n_via = 0;
    const uint16_t* row = lds_row;
    uint32_t cur_src = kPathsNoPred;
    for (uint32_t it = it0; it < it1; it++) {
        // (the item is the same in every lane of the workgroup: the barriers are uniform)
        const uint32_t src = __builtin_amdgcn_readfirstlane(items[it].src);
        const uint32_t q0 = __builtin_amdgcn_readfirstlane(items[it].q0), q1 = __builtin_amdgcn_readfirstlane(items[it].q1);
        if (src != cur_src) {
            __syncthreads();  // (every wave has left the row of the item before)
            row = stage_row(lds_row, hops + (size_t)src * S.n, S.n);
            __syncthreads();
            cur_src = src;
        }
        for (uint32_t q = q0 + wave; q < q1; q += kPathsWaves) {
            const uint32_t j = __builtin_amdgcn_readfirstlane(dst[q]), o = __builtin_amdgcn_readfirstlane(pos[q]);
            const uint32_t d = __builtin_amdgcn_readfirstlane((uint32_t)row[j]);
            const bool fits = d <= S.max_len;
            uint16_t* nrow = NODES ? out_nodes + (size_t)o * (S.max_len + 1u) : nullptr;
            bool broken = false;
            uint32_t cur = j;
            for (uint32_t t = d; t >= 2u; t--) {
                const uint32_t* __restrict__ et = ET + (size_t)cur * S.stride;
                uint32_t k = kPathsNoPred;
                for (uint32_t wp = 0; wp < S.bit_words; wp += kPathsPassWords) {
                    const uint32_t w = wp + lane;
                    const uint32_t mine = paths_word_pred(w < S.bit_words ? et[w] : 0u, w, row, t - 1u);
                    const unsigned long long hit = __ballot(mine != kPathsNoPred);
                    if (hit) {
                        k = (uint32_t)__builtin_amdgcn_readlane((int)mine, __builtin_amdgcn_readfirstlane(__builtin_ctzll(hit)));
                        break;
                    }
                }
                if (k == kPathsNoPred) {
                    broken = true;
                    break;
                }
                if (lane == 0) {
                    if (NODES && fits) paths_store(nrow, t - 1u, k);
                    if constexpr (VIA == kViaGlobal) atomicAdd(out_via + k, 1u);
                    if constexpr (VIA == kViaLds) atomicAdd(via_lds + k, 1u);
                }
                cur = k;
            }
            const bool found = d != 0u && !broken;
            if (lane == 0) out_len[o] = (uint16_t)(found ? d : 0u);
            if constexpr (NODES) {
                const bool written = found && fits;
                if (written && lane == 0) paths_store(nrow, 0u, src), paths_store(nrow, d, j);
                // (a broken query's nodes so far are overwritten: they have to land first)
                if (broken) __threadfence();
                paths_fill(nrow, written ? d + 1u : 0u, S.max_len + 1u, lane, 64u);
            }
            if (found) {
                n_found++, n_via += d - 1u, longest = max(longest, d);
                if (NODES && !fits) n_too_long++;
            } else if (broken) {
                n_broken++;
            } else {
                n_unreachable++;
            }
        }
    }
    // the workgroup's counters: one add each
    uint64_t* sh = reinterpret_cast<uint64_t*>(lds + S.row_bytes);  // [kPathsWaves][kPathsResultWords]
    if (lane == 0) {
        uint64_t* mine = sh + wave * kPathsResultWords;
        mine[0] = n_found, mine[1] = n_unreachable, mine[2] = n_too_long, mine[3] = n_broken, mine[4] = n_via, mine[5] = longest;
    }
    __syncthreads();
    if (threadIdx.x < kPathsResultWords) {
        uint64_t s = 0;
#pragma unroll
        for (uint32_t v = 0; v < kPathsWaves; v++) {
            const uint64_t x = sh[v * kPathsResultWords + threadIdx.x];
            s = threadIdx.x == 5u ? max(s, x) : s + x;
        }
        if (s) {
            if (threadIdx.x == 5u) atomicMax(result + 5, (unsigned long long)s);
            else atomicAdd(result + threadIdx.x, (unsigned long long)s);
        }
    }
    if constexpr (VIA == kViaLds)  // (behind the barrier above: every wave has finished its queries)
        for (uint32_t i = threadIdx.x; i < S.n; i += kPathsBlock) {
            const uint32_t c = via_lds[i];
            if (c) atomicAdd(out_via + i, c);
        }
}

template <bool NODES, int VIA>
int launch_walk(uint32_t blocks_per_cu, PathsShape S, uint32_t lds, hipStream_t st, const uint16_t* hops, const uint32_t* ET,
                const PathsItem* items, const uint32_t* dst, const uint32_t* pos, uint16_t* out_len, uint16_t* out_nodes,
                uint32_t* out_via, unsigned long long* result, std::string* err) {
    auto kernel = k_paths_walk<NODES, VIA>;
    // (a row of 2^15 cells and its 16 B pass 64 KiB of LDS)
    HIPCHK(allow_dynamic_lds(kernel, lds));
    const Runs runs = run_grid(kernel, (int)kPathsBlock, lds, S.n_items, blocks_per_cu);
    S.per = (uint32_t)runs.per;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)runs.groups), dim3(kPathsBlock), lds, st, hops, ET, S, items, dst, pos, out_len,
                       out_nodes, out_via, result);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace

int dev_reach_paths(uint32_t blocks_per_cu, const PathsSpecDev& spec, uint16_t* out_len, uint16_t* out_nodes,
                    uint32_t* out_via, PathsResult* res, void* stream, std::string* err) {
    hipStream_t st = (hipStream_t)stream;
    *res = PathsResult{0, 0, 0, 0, 0, 0};
    const uint32_t n = spec.n, stride = closure_stride(n);
    if (out_via) HIPCHK(hipMemsetAsync(out_via, 0, (size_t)n * sizeof(uint32_t), st));
    if (!spec.n_queries) {
        HIPCHK(hipStreamSynchronize(st));
        return 0;
    }
    const PathsPartition& P = *spec.part;
    const PathsPlan plan = paths_plan(n);
    const uint32_t nq = (uint32_t)spec.n_queries, n_items = (uint32_t)P.items.size();
    // RESULT: kPathsResultWords u64 in 64 B, cleared whole; ET: n x stride; the last three are one host
    // image and one copy
    enum { RESULT, MAT_ET, DST, POS, ITEMS };
    const auto l = lay_out({64, (size_t)n * stride * sizeof(uint32_t), (size_t)nq * sizeof(uint32_t), (size_t)nq * sizeof(uint32_t),
                            (size_t)n_items * sizeof(PathsItem)});
    // (before blk: a call that leaves early still outlives the copy out of it)
    std::vector<unsigned char> host(l.total - l.off[DST], 0);
    l.put(host, DST, DST, P.dst.data(), nq), l.put(host, DST, POS, P.pos.data(), nq), l.put(host, DST, ITEMS, P.items);
    Scratch blk;
    if (Scratch::make(&blk, l.total, err) != 0) {
        (void)hipGetLastError();
        return -2;
    }
    unsigned long long* result = l.at<unsigned long long>(blk, RESULT);
    uint32_t* ET = l.at<uint32_t>(blk, MAT_ET);
    HIPCHK(hipMemsetAsync(result, 0, 64, st));
    HIPCHK(hipMemcpyAsync(l.at<unsigned char>(blk, DST), host.data(), host.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_paths_edges_t, dim3((n + kPathsEdgeCols - 1u) / kPathsEdgeCols, stride / kPathsEdgeWords), dim3(kPathsBlock),
                       0, st, spec.hops, n, stride, ET);
    HIPCHK(hipGetLastError());
    const PathsShape S{n, stride, closure_bit_words(n), out_nodes ? spec.max_len : 0u, n_items, 0, plan.row_bytes};
    const bool via_lds = out_via && plan.via_bytes;
    const uint32_t lds = plan.lds_bytes - (via_lds ? 0u : plan.via_bytes);
    const PathsItem* items = l.at<PathsItem>(blk, ITEMS);
    const uint32_t *dst = l.at<uint32_t>(blk, DST), *pos = l.at<uint32_t>(blk, POS);
    int rc;
#define PG_WALK(NODES, VIA) \
    launch_walk<NODES, VIA>(blocks_per_cu, S, lds, st, spec.hops, ET, items, dst, pos, out_len, out_nodes, out_via, result, err)
    if (out_nodes) rc = !out_via ? PG_WALK(true, kViaNone) : via_lds ? PG_WALK(true, kViaLds) : PG_WALK(true, kViaGlobal);
    else rc = !out_via ? PG_WALK(false, kViaNone) : via_lds ? PG_WALK(false, kViaLds) : PG_WALK(false, kViaGlobal);
#undef PG_WALK
    if (rc != 0) return rc;
    uint64_t r[kPathsResultWords] = {0};
    HIPCHK(hipMemcpyAsync(r, result, sizeof r, hipMemcpyDeviceToHost, st));
    if (blk.finish(st, "reach paths", err) != 0) return -1;
    *res = PathsResult{r[0], r[1], r[2], r[3], r[4], (uint32_t)r[5]};
    return 0;
}

}  // namespace pg
