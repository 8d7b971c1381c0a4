// gfx950 kernels of the reachability cut (pg_reach_cut; cut.hpp has the definitions, the per-word
// code and the plan).
//
// One scratch block: A and AT (n x closure_stride(n) bit-words: bit j of A[i] and bit i of AT[j] say
// i -> j), prev / next (the flow; the caller's out_prev / out_next when given), the parents of the
// forward search, and per search a state: a head (X reached, Y reached, Y frontier, X frontier, two
// status slots -- cut_head_words) and a tail (the next level's two frontiers). The heads of the
// forward and the backward search are made on the host and go in with the lists in one copy; the
// forward one is a template that a device copy puts in place before every search.
//  k_edges_t      edge_tiles.hpp, shared with dominators.hip: A, and AT through LDS ballots.
//  k_cut_direct   a workgroup per distinct entry: its pairs with the targets (cut_direct_word),
//                 popcounts added by an integer atomic.
//  k_cut_level    one level of a search, the hot kernel. A workgroup of 16 waves owns the 32 end points
//                 of one bit-word of every bit vector, a wave two of them. The Y frontier is staged
//                 once per workgroup in LDS (n / 8 bytes, at most 4 KiB). For an end point whose X half
//                 is not reached the wave takes the back arc if there is one, else it pulls: its lanes
//                 read LW adjacent words of the row each, ANDed with the frontier from LDS
//                 (cut_scan_word); a ballot finds the first lane with a non-zero word and a
//                 count-trailing-zeros gives the least parent (cut_first); the wave leaves the row at its
//                 first hit. The Y half looks at one bit of the X frontier (cut_y_source). Lane 0 notes
//                 the hits in LDS and stores the parents; thread 0 then stores the workgroup's word of
//                 both new frontiers, ORs it into the reached words -- which no other workgroup reads --
//                 and reports: an atomic OR of "grew", an atomic min of the least target reached. No
//                 parent goes through an atomic: every run gives the same bytes. Workgroup 0 clears the
//                 status slot of the next level.
//  k_cut_augment  one thread: cut_augment from the target the host read back; adds `reroutes`.
//  k_cut_sets     one workgroup: the near and far words from the reached sets of the last forward and of
//                 the backward search, and the heads of the two plain searches.
//  k_cut_finish   one workgroup: the two Reach sets, the four counts, and out_cut.
// One launch per level; the host reads the level's status slot back after each. No kernel waits on
// another workgroup.
//
// No kernel reads a table or touches a hit counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>

#include "audit_launch.hpp"
#include "cut.hpp"
#include "edge_tiles.hpp"

namespace pg {

namespace {

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d, 64);
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

__global__ __launch_bounds__(kDomBlock) void k_cut_direct(const uint32_t* __restrict__ A, const uint32_t* __restrict__ entry,
                                                          const uint32_t* __restrict__ t_bits, uint32_t n, uint32_t stride,
                                                          uint32_t* __restrict__ result) {
    __shared__ uint32_t sh[kDomBlockWaves];
    const uint32_t e = __builtin_amdgcn_readfirstlane(entry[blockIdx.x]);
    if (e >= n) return;  // (checked on the host)
    const uint32_t bw = closure_bit_words(n);
    uint32_t cnt = 0;
    for (uint32_t w = threadIdx.x; w < bw; w += kDomBlock)
        cnt += (uint32_t)__builtin_popcount(cut_direct_word(A[(size_t)e * stride + w], t_bits[w], e, w));
    const uint32_t ws = wave_sum(cnt);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = ws;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t k = 0; k < kDomBlockWaves; k++) s += sh[k];
        if (s) atomicAdd(&result[0], s);
    }
}

// one level of one search: the roles of cut.hpp's header comment
struct CutLevel {
    const uint32_t* M;     // the rows X pulls along
    const uint16_t* link;  // next (forward) or prev (backward); unused when plain
    uint32_t *RX, *RY;     // reached, updated
    const uint32_t *FX, *FY;
    uint32_t *NX, *NY;     // the new frontiers, every word written
    uint16_t *PX, *PY;     // the parents; null when nobody walks them
    const uint32_t* stop;  // the targets, or null
    uint32_t *status, *status_next;
    uint32_t n, stride, plain;
};

template <uint32_t LW>
__global__ __launch_bounds__(kCutLevelBlock) void k_cut_level(CutLevel a) {
    constexpr uint32_t kStep = 64u * LW;
    __shared__ __attribute__((aligned(16))) uint32_t sF[kCutMaxN / 32u];
    __shared__ uint32_t sNew[2];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t bw = closure_bit_words(a.n), cover = (bw + kStep - 1u) / kStep * kStep;  // (<= kCutMaxN / 32)
    for (uint32_t w = threadIdx.x; w < cover; w += kCutLevelBlock) sF[w] = w < bw ? a.FY[w] : 0u;
    if (threadIdx.x < 2) sNew[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t g = blockIdx.x;  // (< bw)
    const uint32_t rx = a.RX[g], ry = a.RY[g];
    for (uint32_t k = 0; k < kCutWaveNodes; k++) {
        const uint32_t b = wave + kCutWaves * k, v = 32u * g + b;
        if (v >= a.n) continue;  // (uniform in the wave)
        const uint16_t link_v = a.plain ? kCutNone : a.link[v];
        bool hx = false, hy = false;
        uint32_t px = v, py = v;
        if (!((rx >> b) & 1u)) {
            if (cut_x_back(link_v, (sF[g] >> b) & 1u)) {
                hx = true;
            } else {
                const uint32_t* __restrict__ row = a.M + (size_t)v * a.stride;
                for (uint32_t base = 0; base < bw; base += kStep) {
                    const uint32_t w0 = base + lane * LW;
                    uint32_t x[LW], any = 0;
#pragma unroll
                    for (uint32_t q = 0; q < LW; q++) x[q] = 0;
                    if (w0 < a.stride) {  // (stride is a multiple of 4: all LW words or none)
                        uint32_t m[LW], f[LW];
                        load_words<LW>(row + w0, m);
                        load_words<LW>(&sF[w0], f);
#pragma unroll
                        for (uint32_t q = 0; q < LW; q++) x[q] = cut_scan_word(m[q], f[q], v, w0 + q), any |= x[q];
                    }
                    const unsigned long long hit = __ballot(any != 0u);
                    if (hit) {  // (uniform in the wave)
                        uint32_t mine = kCutNoTarget;
#pragma unroll
                        for (uint32_t q = LW; q-- > 0;)
                            if (x[q]) mine = cut_first(x[q], w0 + q);
                        px = (uint32_t)__shfl((int)mine, (int)__builtin_ctzll(hit), 64);
                        hx = true;
                        break;
                    }
                }
            }
        }
        if (a.plain) {
            hy = hx;
        } else if (!((ry >> b) & 1u)) {
            py = cut_y_source(link_v, v);
            hy = cut_bit(a.FX, py);
        }
        if (lane == 0) {
            if (hx) {
                atomicOr(&sNew[0], 1u << b);
                if (a.PX) a.PX[v] = (uint16_t)px;
            }
            if (hy) {
                atomicOr(&sNew[1], 1u << b);
                if (a.PY) a.PY[v] = (uint16_t)py;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t nx = sNew[0], ny = sNew[1];
        a.NX[g] = nx, a.NY[g] = ny;
        if (nx) a.RX[g] = rx | nx;
        if (ny) a.RY[g] = ry | ny;
        if (nx | ny) atomicOr(&a.status[0], 1u);
        if (a.stop) {
            const uint32_t at = nx & a.stop[g];
            if (at) atomicMin(&a.status[1], cut_first(at, g));
        }
        if (g == 0) a.status_next[0] = 0u, a.status_next[1] = kCutNoTarget;
    }
}

__global__ void k_cut_augment(uint32_t t, const uint16_t* __restrict__ p_in, const uint16_t* __restrict__ p_out,
                              const uint32_t* __restrict__ e_bits, const uint32_t* __restrict__ t_bits, uint16_t* prev,
                              uint16_t* next, uint32_t n, uint32_t* __restrict__ result) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && t < n) result[1] += cut_augment(t, p_in, p_out, e_bits, t_bits, prev, next, 2u * n + 2u);
}

// a head's vectors
struct CutHead {
    uint32_t *RX, *RY, *FY, *FX, *status;
};
__host__ __device__ inline CutHead head_of(uint32_t* h, uint32_t stride) {
    return CutHead{h, h + stride, h + 2u * stride, h + 3u * stride, h + 4u * stride};
}
__device__ __forceinline__ void plain_head(const CutHead& h, uint32_t w, uint32_t e, uint32_t c) {
    h.RX[w] = e | c, h.RY[w] = e | c, h.FY[w] = e, h.FX[w] = 0u;
    if (w < kCutStatusWords) h.status[w] = (w & 1u) ? kCutNoTarget : 0u;
}

__global__ __launch_bounds__(kCutFinishBlock) void k_cut_sets(const uint32_t* __restrict__ fwd, const uint32_t* __restrict__ bwd,
                                                              const uint32_t* __restrict__ e_bits, const uint32_t* __restrict__ t_bits,
                                                              uint32_t stride, uint32_t* __restrict__ near, uint32_t* __restrict__ far,
                                                              uint32_t* __restrict__ head_near, uint32_t* __restrict__ head_far) {
    const uint32_t w = threadIdx.x;
    if (w >= stride) return;
    const uint32_t e = e_bits[w], t = t_bits[w];
    const uint32_t nr = cut_near_word(fwd[w], fwd[stride + w], e, t), fr = cut_far_word(bwd[w], bwd[stride + w], e, t);
    near[w] = nr, far[w] = fr;
    plain_head(head_of(head_near, stride), w, e, nr);
    plain_head(head_of(head_far, stride), w, e, fr);
}

__global__ __launch_bounds__(kCutFinishBlock) void k_cut_finish(const uint32_t* __restrict__ near, const uint32_t* __restrict__ far,
                                                                const uint32_t* __restrict__ reached_near,
                                                                const uint32_t* __restrict__ reached_far, uint32_t n, uint32_t stride,
                                                                uint8_t* __restrict__ out_cut, uint32_t* __restrict__ result) {
    constexpr uint32_t kWaves = kCutFinishBlock / 64;
    __shared__ uint32_t sh_w[4][kCutFinishBlock];
    __shared__ uint32_t sh_red[4][kWaves];
    const uint32_t w = threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t x[4] = {0, 0, 0, 0};
    if (w < stride) {
        x[0] = near[w], x[1] = far[w];
        x[2] = cut_reach_word(reached_near[w], x[0]), x[3] = cut_reach_word(reached_far[w], x[1]);
    }
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
        sh_w[k][w] = x[k];
        const uint32_t s = wave_sum((uint32_t)__builtin_popcount(x[k]));
        if (lane == 0) sh_red[k][wave] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t s = 0;
        for (uint32_t k = 0; k < kWaves; k++) s += sh_red[threadIdx.x][k];
        result[2u + threadIdx.x] = s;
    }
    if (out_cut)
        for (uint32_t v = threadIdx.x; v < n; v += kCutFinishBlock) {
            const uint32_t i = v >> 5, b = v & 31u;
            out_cut[v] = cut_flags((sh_w[0][i] >> b) & 1u, (sh_w[1][i] >> b) & 1u, (sh_w[2][i] >> b) & 1u, (sh_w[3][i] >> b) & 1u);
        }
}

// a search's state in scratch, and its run: level after level until a target is reached (*target) or
// nothing grows (*target = kCutNoTarget)
struct Search {
    uint32_t *head, *tail;
    const uint32_t* M;
    const uint16_t* link;
    uint16_t *PX, *PY;
    const uint32_t* stop;
    bool plain;
};
int run_search(const CutPlan& p, hipStream_t st, const Search& s, uint32_t n, uint32_t stride, uint32_t* levels, uint32_t* target,
               std::string* err) {
    const CutHead h = head_of(s.head, stride);
    uint32_t *FX = h.FX, *FY = h.FY, *NX = s.tail, *NY = s.tail + stride;
    // (a level that grows adds a bit to one of two sets of n bits: the loop ends by itself)
    for (uint32_t level = 0;; level++) {
        uint32_t *now = h.status + 2u * (level & 1u), *then = h.status + 2u * (~level & 1u);
        const CutLevel a{s.M, s.link, h.RX, h.RY, FX, FY, NX, NY, s.PX, s.PY, s.stop, now, then, n, stride, s.plain ? 1u : 0u};
        if (p.lane_words == 1) hipLaunchKernelGGL(k_cut_level<1>, dim3(p.level_grid), dim3(kCutLevelBlock), 0, st, a);
        else if (p.lane_words == 2) hipLaunchKernelGGL(k_cut_level<2>, dim3(p.level_grid), dim3(kCutLevelBlock), 0, st, a);
        else hipLaunchKernelGGL(k_cut_level<4>, dim3(p.level_grid), dim3(kCutLevelBlock), 0, st, a);
        HIPCHK(hipGetLastError());
        uint32_t status[2] = {0, kCutNoTarget};
        HIPCHK(hipMemcpyAsync(status, now, sizeof status, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ++*levels;
        *target = status[1];
        if (status[1] != kCutNoTarget || !status[0]) return 0;
        std::swap(FX, NX), std::swap(FY, NY);
    }
}

}  // namespace

int dev_reach_cut(uint32_t blocks_per_cu, const CutSpecDev& spec, uint8_t* out_cut, uint16_t* out_prev, uint16_t* out_next,
                  CutResult* res, void* stream, std::string* err) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = spec.n, stride = closure_stride(n), rw = (n + 15u) / 16u;
    const CutPlan p = cut_plan(n);
    // (before blk: a call that leaves early still outlives the copies out of it)
    uint32_t words[kCutResultWords] = {};
    std::vector<unsigned char> h;  // the host image of LIST .. BWD_H
    Scratch blk;
    // RESULT .. NEXT are adjacent: cleared one by one. LIST .. BWD_H are adjacent: one copy fills them.
    enum { RESULT, MAT_A, MAT_AT, PREV, NEXT, P_IN, P_OUT, NEAR, FAR, FWD_H, FWD_N, BWD_N, RN_H, RN_N, RF_H, RF_N,
           LIST, ENTRY, E_BITS, T_BITS, FWD_T, BWD_H, END };
    const size_t mat = (size_t)n * stride * sizeof(uint32_t), vec = (size_t)stride * sizeof(uint32_t), ids = (size_t)n * sizeof(uint16_t);
    const size_t head = cut_head_words(stride) * sizeof(uint32_t), tail = 2u * vec;
    const auto l = lay_out({kCutResultWords * sizeof(uint32_t), mat, mat, ids, ids, ids, ids, vec, vec, head, tail, tail, head, tail, head, tail,
                            spec.n_list * sizeof(uint32_t), spec.n_entry * sizeof(uint32_t), vec, vec, head, head, 0});
    if (Scratch::make(&blk, l.total, err) != 0) {
        (void)hipGetLastError();
        return -2;
    }
    uint32_t *d_res = l.at<uint32_t>(blk, RESULT), *A = l.at<uint32_t>(blk, MAT_A), *AT = l.at<uint32_t>(blk, MAT_AT);
    uint16_t *prev = out_prev ? out_prev : l.at<uint16_t>(blk, PREV), *next = out_next ? out_next : l.at<uint16_t>(blk, NEXT);
    uint16_t *p_in = l.at<uint16_t>(blk, P_IN), *p_out = l.at<uint16_t>(blk, P_OUT);
    uint32_t *near = l.at<uint32_t>(blk, NEAR), *far = l.at<uint32_t>(blk, FAR);
    uint32_t *list = l.at<uint32_t>(blk, LIST), *entry = l.at<uint32_t>(blk, ENTRY), *e_bits = l.at<uint32_t>(blk, E_BITS),
             *t_bits = l.at<uint32_t>(blk, T_BITS);
    uint32_t *fwd_h = l.at<uint32_t>(blk, FWD_H), *fwd_t = l.at<uint32_t>(blk, FWD_T), *bwd_h = l.at<uint32_t>(blk, BWD_H);
    uint32_t *rn_h = l.at<uint32_t>(blk, RN_H), *rf_h = l.at<uint32_t>(blk, RF_H);

    h.assign(l.off[END] - l.off[LIST], 0);
    l.put(h, LIST, LIST, spec.svc_list, spec.n_list);
    l.put(h, LIST, ENTRY, spec.entry, spec.n_entry);
    l.put(h, LIST, E_BITS, spec.e_bits, stride);
    l.put(h, LIST, T_BITS, spec.t_bits, stride);
    {   // the heads: forward X blocked for E, Y for E u T, E the frontier; backward with E and T swapped
        const CutHead f = head_of(l.in<uint32_t>(h, LIST, FWD_T), stride), b = head_of(l.in<uint32_t>(h, LIST, BWD_H), stride);
        for (uint32_t w = 0; w < stride; w++) {
            const uint32_t e = spec.e_bits[w], t = spec.t_bits[w];
            f.RX[w] = e, f.RY[w] = e | t, f.FY[w] = e;
            b.RX[w] = t, b.RY[w] = e | t, b.FY[w] = t;
        }
        f.status[1] = f.status[3] = b.status[1] = b.status[3] = kCutNoTarget;
    }
    HIPCHK(hipMemsetAsync(d_res, 0, kCutResultWords * sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(prev, 0xFF, ids, st));
    HIPCHK(hipMemsetAsync(next, 0xFF, ids, st));
    if (out_cut) HIPCHK(hipMemsetAsync(out_cut, 0, n, st));
    HIPCHK(hipMemcpyAsync(list, h.data(), h.size(), hipMemcpyHostToDevice, st));

    EdgeTiles S{p.t_col_tiles, p.t_grid, 0};
    const Runs runs = run_grid(k_edges_t<true, false>, (int)kDomBlock, 0, S.items, blocks_per_cu);
    S.per = (uint32_t)runs.per;
    hipLaunchKernelGGL((k_edges_t<true, false>), dim3((uint32_t)runs.groups), dim3(kDomBlock), 0, st, spec.matrix, list, spec.n_list, n, rw,
                       stride, S, A, AT, (uint32_t*)nullptr);
    HIPCHK(hipGetLastError());
    if (spec.n_entry) {
        hipLaunchKernelGGL(k_cut_direct, dim3(spec.n_entry), dim3(kDomBlock), 0, st, A, entry, t_bits, n, stride, d_res);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(words, d_res, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    // (the copies above read `h`: they are done before it goes, whatever ends the call)
    HIPCHK(hipStreamSynchronize(st));

    CutResult r{};
    r.n_direct = words[0];
    r.cut_size = kCutNoSize;
    if (!r.n_direct) {
        r.separable = 1;
        // at most min(n, max_cut + 1) augmentations: a path takes an end point outside E u T of its own
        const Search fwd{fwd_h, l.at<uint32_t>(blk, FWD_N), AT, next, p_in, p_out, t_bits, false};
        for (;;) {
            if (r.n_paths == spec.max_cut + 1u) {
                r.capped = 1;
                break;
            }
            HIPCHK(hipMemcpyAsync(fwd_h, fwd_t, head, hipMemcpyDeviceToDevice, st));
            uint32_t target = kCutNoTarget;
            if (int rc = run_search(p, st, fwd, n, stride, &r.levels, &target, err)) return rc;
            if (target == kCutNoTarget) break;
            hipLaunchKernelGGL(k_cut_augment, dim3(1), dim3(64), 0, st, target, p_in, p_out, e_bits, t_bits, prev, next, n, d_res);
            HIPCHK(hipGetLastError());
            r.n_paths++;
        }
    }
    if (r.separable && !r.capped) {
        uint32_t target = kCutNoTarget;
        const Search bwd{bwd_h, l.at<uint32_t>(blk, BWD_N), A, prev, nullptr, nullptr, nullptr, false};
        if (int rc = run_search(p, st, bwd, n, stride, &r.levels, &target, err)) return rc;
        hipLaunchKernelGGL(k_cut_sets, dim3(1), dim3(kCutFinishBlock), 0, st, fwd_h, bwd_h, e_bits, t_bits, stride, near, far, rn_h, rf_h);
        HIPCHK(hipGetLastError());
        const Search rn{rn_h, l.at<uint32_t>(blk, RN_N), AT, nullptr, nullptr, nullptr, nullptr, true};
        const Search rf{rf_h, l.at<uint32_t>(blk, RF_N), AT, nullptr, nullptr, nullptr, nullptr, true};
        if (int rc = run_search(p, st, rn, n, stride, &r.levels, &target, err)) return rc;
        if (int rc = run_search(p, st, rf, n, stride, &r.levels, &target, err)) return rc;
        hipLaunchKernelGGL(k_cut_finish, dim3(p.finish_grid), dim3(kCutFinishBlock), 0, st, near, far, head_of(rn_h, stride).RY,
                           head_of(rf_h, stride).RY, n, stride, out_cut, d_res);
        HIPCHK(hipGetLastError());
        r.cut_size = r.n_paths;
    }
    HIPCHK(hipMemcpyAsync(words, d_res, sizeof(words), hipMemcpyDeviceToHost, st));
    if (blk.finish(st, "reach cut", err) != 0) return -1;
    r.reroutes = words[1];
    if (r.separable && !r.capped) r.near_reach = words[4], r.far_reach = words[5];
    *res = r;
    return 0;
}

}  // namespace pg
