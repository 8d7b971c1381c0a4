// gfx950 kernels of the observed reachability (pg_reach_observed; observed.hpp has the tables, the
// per-flow code and the plan).
//
//  k_observed        the streaming scatter. The flows are cut into tiles of one step of a workgroup
//                    (256 lanes x 8 flows on the vector path, 256 x 1 on the scalar one), one contiguous
//                    run of tiles per workgroup, the grid the resident workgroups. A workgroup first
//                    stages the service table and -- where the plan says so -- the address tables in
//                    LDS (16-B copies), and clears its LDS counters. Per tile a lane loads its flows
//                    with the non-temporal policy (VEC: two 16-B loads per address array, one per port
//                    array, 8 B of protocols; the ragged last group and the scalar path: one element at
//                    a time), runs obs_flow on each, and marks a cell by a no-return relaxed agent-scope
//                    atomic OR -- with "observed_test_first" only after a load of the word has not
//                    shown the bit (1: a plain load, 2: a relaxed agent-scope load, which the CU's L1
//                    does not answer; a stale answer only costs a redundant atomic). The status bytes
//                    leave as one 8-B store per lane (VEC, out_flow 8-B aligned) or, on the scalar
//                    path, as one word per four lanes gathered by shuffles (out_flow 4-B aligned), else
//                    as bytes. Statuses are counted in registers and summed per wave by shuffles, the
//                    matched flows per service key by LDS atomics (one per flow, whatever the services
//                    that share the key); at its end a workgroup flushes with one u64 atomic per status
//                    and per service with a count.
//  k_observed_cells  the ALLOW cells of out_packed: grid-stride over the words (16-B loads where the
//                    array is 16-B aligned), summed per wave and workgroup, one u64 atomic each.
// No workgroup waits on another. The host reads nothing back before the end: one synchronisation.
//
// No kernel reads a table of the policy or touches a hit counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "audit_launch.hpp"
#include "observed.hpp"

namespace pg {

namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

struct ObsArgs {
    // HBM: the address tables and index arrays, the service part [keys 2 n_svc | starts n_svc + 1 | indices n_svc]
    const uint32_t *src_tab, *dst_tab, *src_idx, *dst_idx, *svc;
    uint32_t src_mask, dst_mask, nk, n_svc, n_src, row_words;
    uint32_t match_src_port, test_first;
    // one launch's piece of the flows
    const uint32_t *f_src, *f_dst;
    const uint16_t *f_sport, *f_dport;
    const uint8_t* f_proto;
    uint32_t n, tiles, per;  // flows; tiles; tiles of a workgroup
    uint32_t* out;
    uint8_t* out_flow;
    unsigned long long* counters;  // [4 statuses | cells | n_svc]
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// n words (a multiple of 4, both sides 16-B aligned) from HBM into LDS
__device__ __forceinline__ void stage_words(uint32_t* __restrict__ to, const uint32_t* __restrict__ from, uint32_t n) {
    for (uint32_t w = 4u * threadIdx.x; w < n; w += 4u * kObsBlock)
        *reinterpret_cast<v4u*>(to + w) = *reinterpret_cast<const v4u*>(from + w);
}

template <bool VEC, bool SRC_LDS, bool DST_LDS>
__global__ __launch_bounds__(kObsBlock) void k_observed(ObsArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t obs_lds[];
    constexpr uint32_t Q = VEC ? kObsVecFlows : 1u;
    // LDS: [keys | starts | indices | key counters n_svc | status counters 4] obs_svc_words, then the staged tables
    uint32_t* const l_keys = obs_lds;
    uint32_t* const l_start = l_keys + 2u * A.n_svc;
    uint32_t* const l_sidx = l_start + A.n_svc + 1u;
    uint32_t* const l_kcnt = l_sidx + A.n_svc;
    uint32_t* const l_stat = l_kcnt + A.n_svc;
    uint32_t* const l_src = obs_lds + obs_svc_words(A.n_svc);
    uint32_t* const l_dst = l_src + (SRC_LDS ? kObsCellWords * (A.src_mask + 1u) : 0u);
    for (uint32_t w = threadIdx.x; w < 4u * A.n_svc + 1u; w += kObsBlock) obs_lds[w] = A.svc[w];
    for (uint32_t w = threadIdx.x; w < A.n_svc + 4u; w += kObsBlock) l_kcnt[w] = 0u;
    if constexpr (SRC_LDS) stage_words(l_src, A.src_tab, kObsCellWords * (A.src_mask + 1u));
    if constexpr (DST_LDS) stage_words(l_dst, A.dst_tab, kObsCellWords * (A.dst_mask + 1u));
    __syncthreads();

    ObsView<const uint32_t*> T;
    if constexpr (SRC_LDS) T.src_tab = l_src;
    else T.src_tab = A.src_tab;
    if constexpr (DST_LDS) T.dst_tab = l_dst;
    else T.dst_tab = A.dst_tab;
    T.src_idx = A.src_idx, T.dst_idx = A.dst_idx;
    T.skeys = l_keys, T.sstart = l_start, T.sidx = l_sidx;
    T.src_mask = A.src_mask, T.dst_mask = A.dst_mask, T.nk = A.nk;
    T.n_src = A.n_src, T.row_words = A.row_words, T.match_src_port = A.match_src_port != 0u;

    const uint32_t test_first = A.test_first;
    uint32_t* const out = A.out;
    auto mark = [&](uint32_t w, uint32_t bit) {
        uint32_t* p = out + w;
        if (test_first == 1u) {
            if (*p & bit) return;
        } else if (test_first) {
            if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) return;
        }
        (void)__hip_atomic_fetch_or(p, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };

    const uint32_t lane = threadIdx.x & 63u;
    const bool flow_vec = VEC && ((uintptr_t)A.out_flow & 7u) == 0, flow_words = ((uintptr_t)A.out_flow & 3u) == 0;
    uint32_t cnt[4] = {0, 0, 0, 0};
    const uint32_t tile1 = min(blockIdx.x * A.per + A.per, A.tiles);
    for (uint32_t tile = blockIdx.x * A.per; tile < tile1; tile++) {
        // (n < 2^30 and a tile starts below n: no wrap)
        const uint32_t t0 = tile * (kObsBlock * Q) + threadIdx.x * Q;
        uint32_t src[Q], dst[Q], sport[Q], dport[Q], proto[Q];
        const bool whole = t0 + Q <= A.n;
        if (VEC && whole) {
            const v4u s0 = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(A.f_src + t0));
            const v4u s1 = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(A.f_src + t0) + 1);
            const v4u d0 = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(A.f_dst + t0));
            const v4u d1 = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(A.f_dst + t0) + 1);
            const v4u dp = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(A.f_dport + t0));
            const v2u pr = __builtin_nontemporal_load(reinterpret_cast<const v2u*>(A.f_proto + t0));
            v4u sp = {0, 0, 0, 0};
            if (T.match_src_port) sp = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(A.f_sport + t0));
#pragma unroll
            for (uint32_t q = 0; q < Q; q++) {
                src[q] = q < 4 ? s0[q & 3u] : s1[q & 3u];
                dst[q] = q < 4 ? d0[q & 3u] : d1[q & 3u];
                dport[q] = (dp[q >> 1] >> (16u * (q & 1u))) & 0xFFFFu;
                sport[q] = (sp[q >> 1] >> (16u * (q & 1u))) & 0xFFFFu;
                proto[q] = (pr[(q >> 2) & 1u] >> (8u * (q & 3u))) & 0xFFu;
            }
        } else {
#pragma unroll
            for (uint32_t q = 0; q < Q; q++) {
                const bool in = t0 + q < A.n;
                src[q] = in ? __builtin_nontemporal_load(A.f_src + t0 + q) : 0u;
                dst[q] = in ? __builtin_nontemporal_load(A.f_dst + t0 + q) : 0u;
                dport[q] = in ? __builtin_nontemporal_load(A.f_dport + t0 + q) : 0u;
                proto[q] = in ? __builtin_nontemporal_load(A.f_proto + t0 + q) : 0u;
                sport[q] = in && T.match_src_port ? __builtin_nontemporal_load(A.f_sport + t0 + q) : 0u;
            }
        }
        uint32_t st[Q];
#pragma unroll
        for (uint32_t q = 0; q < Q; q++) {
            st[q] = 0u;
            if (t0 + q < A.n) {
                uint32_t k = 0;
                st[q] = obs_flow(T, src[q], dst[q], sport[q], dport[q], proto[q], &k, mark);
                if (st[q] == kObsMatched) atomicAdd(&l_kcnt[k], 1u);
#pragma unroll
                for (uint32_t s = 0; s < 4; s++) cnt[s] += st[q] == s;
            }
        }
        if (A.out_flow) {
            if constexpr (VEC) {
                if (flow_vec && whole) {
                    v2u w = {0, 0};
#pragma unroll
                    for (uint32_t q = 0; q < Q; q++) w[q >> 2] |= st[q] << (8u * (q & 3u));
                    __builtin_nontemporal_store(w, reinterpret_cast<v2u*>(A.out_flow + t0));
                } else {
#pragma unroll
                    for (uint32_t q = 0; q < Q; q++)
                        if (t0 + q < A.n) A.out_flow[t0 + q] = (uint8_t)st[q];
                }
            } else {
                // four lanes' bytes in the first one's word (every lane of the wave is here: the loop bounds are uniform)
                const uint32_t s = st[0];
                const uint32_t w = s | (uint32_t)__shfl_down(s, 1, 64) << 8 | (uint32_t)__shfl_down(s, 2, 64) << 16 |
                                   (uint32_t)__shfl_down(s, 3, 64) << 24;
                if (flow_words && (t0 | 3u) < A.n) {
                    if (!(lane & 3u)) *reinterpret_cast<uint32_t*>(A.out_flow + t0) = w;
                } else if (t0 < A.n) {
                    A.out_flow[t0] = (uint8_t)s;
                }
            }
        }
    }
#pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        const uint32_t c = wave_sum(cnt[s]);
        if (lane == 0 && c) atomicAdd(&l_stat[s], c);
    }
    __syncthreads();
    // (a workgroup sees fewer than 2^30 flows: its 32-bit LDS counts are exact)
    if (threadIdx.x < 4u && l_stat[threadIdx.x]) atomicAdd(A.counters + threadIdx.x, (unsigned long long)l_stat[threadIdx.x]);
    for (uint32_t k = threadIdx.x; k < A.nk; k += kObsBlock) {
        const uint32_t c = l_kcnt[k];
        if (!c) continue;
        for (uint32_t q = l_start[k]; q < l_start[k + 1u]; q++) atomicAdd(A.counters + kObsCntSvc + l_sidx[q], (unsigned long long)c);
    }
}

__global__ __launch_bounds__(kObsBlock) void k_observed_cells(const uint32_t* __restrict__ words, uint64_t n_words,
                                                             unsigned long long* __restrict__ cells) {
    __shared__ uint32_t sh[kObsBlock / 64];
    const uint64_t tid = (uint64_t)blockIdx.x * kObsBlock + threadIdx.x, step = (uint64_t)gridDim.x * kObsBlock;
    // (a lane sees n_words / step + 4 words of 16 cells at most: 32 bits hold its sum for any n_words < 2^32)
    uint32_t c = 0;
    uint64_t done = 0;
    if (((uintptr_t)words & 15u) == 0) {
        const uint64_t quads = n_words / 4u;
        for (uint64_t q = tid; q < quads; q += step) {
            const v4u x = *reinterpret_cast<const v4u*>(words + 4u * q);
            c += obs_allow_cells(x[0]) + obs_allow_cells(x[1]) + obs_allow_cells(x[2]) + obs_allow_cells(x[3]);
        }
        done = 4u * quads;
    }
    for (uint64_t w = done + tid; w < n_words; w += step) c += obs_allow_cells(words[w]);
    c = wave_sum(c);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (uint32_t v = 0; v < kObsBlock / 64; v++) s += sh[v];
        if (s) atomicAdd(cells, s);
    }
}

// f(k_observed<VEC, SRC_LDS, DST_LDS>) of the plan's staging and the path
template <bool VEC, class F>
void with_tables(const ObservedPlan& p, F f) {
    if (p.src_in_lds && p.dst_in_lds) f(k_observed<VEC, true, true>);
    else if (p.src_in_lds) f(k_observed<VEC, true, false>);
    else if (p.dst_in_lds) f(k_observed<VEC, false, true>);
    else f(k_observed<VEC, false, false>);
}
template <class F>
void with_kernel(bool vec, const ObservedPlan& p, F f) {
    if (vec) with_tables<true>(p, f);
    else with_tables<false>(p, f);
}

}  // namespace

ObservedPlan dev_observed_plan(uint32_t n_src, uint32_t n_dst, uint32_t n_svc, uint32_t lds_budget, uint32_t blocks_per_cu) {
    ObservedPlan p = observed_plan(n_src, n_dst, n_svc, lds_budget);
    with_kernel(true, p, [&](auto kernel) {
        (void)allow_dynamic_lds(kernel, p.lds_bytes);
        p.grid = (uint32_t)grid_resident(kernel, (int)kObsBlock, p.lds_bytes, (uint64_t)1 << 40, blocks_per_cu);
        (void)hipGetLastError();  // (a failed query is answered by grid_resident's fall-back)
    });
    return p;
}

int dev_reach_observed(const ObservedKnobs& knobs, const ObservedSpecDev& spec, uint32_t* out_packed, uint8_t* out_flow,
                       uint64_t* out_svc_flows, ObservedResult* result, void* stream, std::string* err) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t rw = (spec.n_dst + 15u) / 16u, nv = spec.n_svc;
    const uint64_t n_words = (uint64_t)nv * spec.n_src * rw;  // < 2^32 (the caller checks)
    const ObservedPlan plan = observed_plan(spec.n_src, spec.n_dst, nv, knobs.lds_bytes);
    const bool sport = (spec.flags & kObsMatchSrcPort) != 0;
    const bool vec = (((uintptr_t)spec.f_src | (uintptr_t)spec.f_dst | (uintptr_t)spec.f_dport | (uintptr_t)spec.f_proto |
                       (sport ? (uintptr_t)spec.f_sport : 0)) & 15u) == 0;
    // (before blk: a call that leaves early still outlives the copies from and into them)
    std::vector<unsigned char> image;
    unsigned long long back[kObsCntSvc] = {};
    Scratch blk;
    enum { SRC_TAB, SRC_IDX, DST_TAB, DST_IDX, SVC, CNT };
    const size_t svc_words = 4u * (size_t)nv + 1u, n_cnt = kObsCntSvc + (size_t)nv;
    const auto l = lay_out({spec.src->tab.size() * 4, spec.src->idx.size() * 4, spec.dst->tab.size() * 4, spec.dst->idx.size() * 4,
                            svc_words * 4, n_cnt * sizeof(uint64_t)});
    if (Scratch::make(&blk, l.total, err) != 0) {
        (void)hipGetLastError();
        return -2;
    }
    image.assign(l.off[CNT], 0);
    l.put(image, SRC_TAB, SRC_TAB, spec.src->tab), l.put(image, SRC_TAB, SRC_IDX, spec.src->idx);
    l.put(image, SRC_TAB, DST_TAB, spec.dst->tab), l.put(image, SRC_TAB, DST_IDX, spec.dst->idx);
    uint32_t* hs = l.in<uint32_t>(image, SRC_TAB, SVC);
    std::copy(spec.svc->keys.begin(), spec.svc->keys.end(), hs);
    std::copy(spec.svc->start.begin(), spec.svc->start.end(), hs + 2u * nv);
    std::copy(spec.svc->idx.begin(), spec.svc->idx.end(), hs + 3u * nv + 1u);
    HIPCHK(hipMemcpyAsync(blk.at<unsigned char>(0), image.data(), image.size(), hipMemcpyHostToDevice, st));
    unsigned long long* d_cnt = l.at<unsigned long long>(blk, CNT);
    HIPCHK(hipMemsetAsync(d_cnt, 0, n_cnt * sizeof(uint64_t), st));
    if (n_words && !(spec.flags & kObsAccumulate)) HIPCHK(hipMemsetAsync(out_packed, 0, n_words * sizeof(uint32_t), st));

    ObsArgs A{};
    A.src_tab = l.at<uint32_t>(blk, SRC_TAB), A.src_idx = l.at<uint32_t>(blk, SRC_IDX);
    A.dst_tab = l.at<uint32_t>(blk, DST_TAB), A.dst_idx = l.at<uint32_t>(blk, DST_IDX), A.svc = l.at<uint32_t>(blk, SVC);
    A.src_mask = spec.src->cap - 1u, A.dst_mask = spec.dst->cap - 1u, A.nk = spec.svc->nk, A.n_svc = nv;
    A.n_src = spec.n_src, A.row_words = rw, A.match_src_port = sport, A.test_first = knobs.test_first;
    A.out = out_packed, A.counters = d_cnt;
    // pieces of at most kObsMaxLaunchFlows (or "launch_max_tuples") flows, in order on the stream
    const uint64_t cap = knobs.launch_max ? std::min<uint64_t>(knobs.launch_max, kObsMaxLaunchFlows) : kObsMaxLaunchFlows;
    const uint32_t tile_flows = kObsBlock * (vec ? kObsVecFlows : 1u);
    for (uint64_t at = 0; at < spec.n; at += cap) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(cap, spec.n - at);
        A.f_src = spec.f_src + at, A.f_dst = spec.f_dst + at, A.f_dport = spec.f_dport + at, A.f_proto = spec.f_proto + at;
        A.f_sport = sport ? spec.f_sport + at : nullptr;
        A.out_flow = out_flow ? out_flow + at : nullptr;
        A.n = n, A.tiles = (n + tile_flows - 1u) / tile_flows;
        hipError_t e = hipSuccess;
        with_kernel(vec, plan, [&](auto kernel) {
            e = allow_dynamic_lds(kernel, plan.lds_bytes);
            if (e != hipSuccess) return;
            const Runs runs = run_grid(kernel, (int)kObsBlock, plan.lds_bytes, A.tiles, knobs.blocks_per_cu);
            A.per = (uint32_t)runs.per;
            hipLaunchKernelGGL(kernel, dim3((uint32_t)runs.groups), dim3(kObsBlock), plan.lds_bytes, st, A);
        });
        HIPCHK(e);
        HIPCHK(hipGetLastError());
    }
    if (n_words) {
        const int grid = grid_resident(k_observed_cells, (int)kObsBlock, 0, (n_words + 3u) / 4u, knobs.blocks_per_cu);
        (void)hipGetLastError();
        hipLaunchKernelGGL(k_observed_cells, dim3(grid), dim3(kObsBlock), 0, st, out_packed, n_words, d_cnt + kObsCntCells);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(back, d_cnt, sizeof(back), hipMemcpyDeviceToHost, st));
    if (out_svc_flows)
        HIPCHK(hipMemcpyAsync(out_svc_flows, d_cnt + kObsCntSvc, (size_t)nv * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
    if (blk.finish(st, "reach observed", err) != 0) return -1;
    *result = ObservedResult{back[kObsMatched], back[kObsNoSrc], back[kObsNoDst], back[kObsNoSvc], back[kObsCntCells]};
    return 0;
}

}  // namespace pg
