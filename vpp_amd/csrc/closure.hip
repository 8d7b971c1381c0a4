// gfx950 kernels of the reachability closure (pg_reach_closure; closure.hpp has the per-word code).
//
// Four n x stride bit matrices in one scratch block: A (edges), R (reached), F and F' (the frontier
// of this level and of the next, swapped by the host). Beside them, per 16-row tile of F, the OR of
// its rows (T: which k a chunk of the tile needs at all) and per row a live flag (is the row's
// frontier non-empty), both written by the level before.
//  k_closure_edges  a lane takes one bit-word (i, w), a workgroup 16 words of the 16 rows of a tile: the
//                   selected slices' ALLOW masks compacted and ORed (the slice list is read through
//                   scalar loads), masked to the row, stored to A, R and F; live flags, hop 1; the
//                   tile's OR to T through LDS, one u64 add of the popcounts per workgroup
//  k_closure_step   one level, F' = (F (x) A) & ~R, R |= F'. A workgroup of 16 waves owns 16 rows x
//                   64 * LW bit-words; wave w holds the accumulators of row w, a lane LW adjacent
//                   words. k goes in chunks of 32: the chunk's T word (scalar) says which A rows any
//                   row of the tile needs; zero = the chunk is skipped by every wave, no barrier;
//                   else those rows' segments are staged in LDS (two buffers: one barrier per
//                   staged chunk; fetched into registers one staged chunk ahead) and every live row
//                   walks its own frontier word, a scalar, bit by bit: one conflict-free ds_read of
//                   LW words per set bit, four in flight while the word has four bits left. Then
//                   the owner of each output word updates R, stores F', the hop counts of the new
//                   cells, the tile's new T words and live flags, and the workgroup adds its
//                   popcount once.
//  k_closure_pack   a workgroup per row: R expanded to the audits' 2-bit layout, the row's popcount
// One launch per level; the host reads the running total back after each and stops when it stands
// still or at max_hops. No kernel waits on another workgroup.
//
// No kernel reads a table or touches a hit counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "audit_launch.hpp"
#include "closure.hpp"

namespace pg {

namespace {

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;  // (lane 0 has the sum)
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
template <uint32_t LW>
__device__ __forceinline__ void store_words(uint32_t* p, const uint32_t (&v)[LW]) {
    if constexpr (LW == 4) *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
    else if constexpr (LW == 2) *reinterpret_cast<uint2*>(p) = make_uint2(v[0], v[1]);
    else *p = v[0];
}

// hop count `level` into the cells of row i that `bits` of bit-word w names
__device__ __forceinline__ void store_hops(uint16_t* __restrict__ hops, uint32_t n, uint32_t i, uint32_t w, uint32_t bits,
                                           uint32_t level) {
    uint16_t* row = hops + (size_t)i * n + 32u * w;
    for (; bits; bits &= bits - 1u) row[__builtin_ctz(bits)] = (uint16_t)level;
}

// the workgroup's sum of cnt added to *total once
template <uint32_t WAVES>
__device__ __forceinline__ void block_add(uint32_t cnt, uint64_t* sh /* WAVES */, unsigned long long* total) {
    const uint64_t ws = wave_sum(cnt);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = ws;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = 0;
#pragma unroll
        for (uint32_t v = 0; v < WAVES; v++) s += sh[v];
        if (s) atomicAdd(total, (unsigned long long)s);
    }
}

// a workgroup takes 16 adjacent bit-words of the 16 rows of a tile: lane (r, wl) the word (16 tile + r, w)
constexpr uint32_t kEdgeWords = kClosureBlock / kClosureTileRows;
static_assert(kEdgeWords == 16 && kClosureTileRows == 16, "k_closure_edges: 16 rows x 16 words per workgroup");

template <bool HOPS>
__global__ __launch_bounds__(kClosureBlock) void k_closure_edges(const uint32_t* __restrict__ matrix,
                                                                 const uint32_t* __restrict__ svc_list, uint32_t n_list,
                                                                 uint32_t n, uint32_t stride, uint32_t* __restrict__ A,
                                                                 uint32_t* __restrict__ R, uint32_t* __restrict__ F,
                                                                 uint32_t* __restrict__ T, uint32_t* __restrict__ live,
                                                                 uint16_t* __restrict__ hops,
                                                                 unsigned long long* __restrict__ total) {
    __shared__ uint32_t sh_t[kClosureTileRows][kEdgeWords];
    __shared__ uint64_t sh[kClosureBlock / 64];
    const uint32_t r = threadIdx.x / kEdgeWords, wl = threadIdx.x % kEdgeWords;
    const uint32_t w = blockIdx.x * kEdgeWords + wl, i = blockIdx.y * kClosureTileRows + r;
    const uint32_t rw = (n + 15u) / 16u;       // input words of a row
    const uint32_t slice = n * rw;             // <= 2^26 words inside a slice
    uint32_t a = 0, cnt = 0;
    if (w < stride && i < n) {
        const uint32_t valid = closure_valid(n, w);
        if (valid) {
            const uint32_t off = i * rw + 2u * w;
            const bool two = 2u * w + 1u < rw;
            for (uint32_t k = 0; k < n_list; k++) {
                const uint32_t* base = matrix + (uint64_t)svc_list[k] * slice;
                a |= closure_bits(base[off], two ? base[off + 1u] : 0u);
            }
            a &= valid;
        }
        const uint32_t o = i * stride + w;
        A[o] = a, R[o] = a, F[o] = a;
        if (a) {
            live[i] = 1u;  // (every writer stores the same value)
            cnt = (uint32_t)__builtin_popcount(a);
            if constexpr (HOPS) store_hops(hops, n, i, w, a, 1u);
        }
    }
    // the tile's T word: the OR over its 16 rows, one writer
    sh_t[r][wl] = a;
    __syncthreads();
    if (r == 0 && w < stride) {
        uint32_t t_or = 0;
#pragma unroll
        for (uint32_t k = 0; k < kClosureTileRows; k++) t_or |= sh_t[k][wl];
        T[blockIdx.y * stride + w] = t_or;
    }
    block_add<kClosureBlock / 64>(cnt, sh, total);
}

template <uint32_t LW, bool HOPS>
__global__ __launch_bounds__(kClosureStepBlock) void k_closure_step(
    const uint32_t* __restrict__ A, const uint32_t* __restrict__ F, const uint32_t* __restrict__ T,
    const uint32_t* __restrict__ live, uint32_t* __restrict__ R, uint32_t* __restrict__ Fn, uint32_t* __restrict__ Tn,
    uint32_t* __restrict__ live_n, uint16_t* __restrict__ hops, unsigned long long* __restrict__ total, uint32_t n,
    uint32_t stride, uint32_t level) {
    constexpr uint32_t kTileWords = 64u * LW;
    // two buffers of 32 A-row segments; after the k loop the first rows hold the waves' T words and sums
    __shared__ __attribute__((aligned(16))) uint32_t lds[2][32][kTileWords];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t my_w = blockIdx.x * kTileWords + lane * LW;  // this lane's first bit-word of a row
    const bool in = my_w < stride;                              // (stride is a multiple of 4: all LW words or none)
    const uint32_t row0 = blockIdx.y * kClosureTileRows + wave * kClosureWaveRows;

    uint32_t acc[kClosureWaveRows][LW];
    uint32_t alive[kClosureWaveRows];
#pragma unroll
    for (uint32_t r = 0; r < kClosureWaveRows; r++) {
#pragma unroll
        for (uint32_t q = 0; q < LW; q++) acc[r][q] = 0;
        alive[r] = row0 + r < n ? live[row0 + r] : 0u;
    }

    const uint32_t* __restrict__ t_row = T + blockIdx.y * stride;
    const uint32_t chunks = closure_bit_words(n);
    // (blockIdx and c only: `need` is the same scalar in every wave, so they skip or stage together)
    uint32_t c = 0, need = 0;
    for (; c < chunks; c++)
        if ((need = __builtin_amdgcn_readfirstlane(t_row[c])) != 0) break;
    // wave w stages the needed rows among its kStage of the chunk's 32; they are fetched one staged chunk
    // ahead, so the loads fly while the chunk before is walked
    constexpr uint32_t kStage = 32u / kClosureWaves;
    uint32_t pre[kStage][LW];
    auto fetch = [&](uint32_t cc, uint32_t nd) {
        const uint32_t mine = nd >> (kStage * wave);
#pragma unroll
        for (uint32_t j = 0; j < kStage; j++)
            if ((mine >> j & 1u) && in) load_words<LW>(A + (32u * cc + kStage * wave + j) * stride + my_w, pre[j]);
    };
    if (c < chunks) fetch(c, need);
    uint32_t buf = 0;
    while (c < chunks) {
        const uint32_t mine = need >> (kStage * wave);
#pragma unroll
        for (uint32_t j = 0; j < kStage; j++)
            if ((mine >> j & 1u) && in) store_words<LW>(&lds[buf][kStage * wave + j][lane * LW], pre[j]);
        uint32_t cn = c + 1u, need_n = 0;
        for (; cn < chunks; cn++)
            if ((need_n = __builtin_amdgcn_readfirstlane(t_row[cn])) != 0) break;
        if (cn < chunks) fetch(cn, need_n);
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < kClosureWaveRows; r++) {
            if (!alive[r]) continue;
            // the frontier word of (row, chunk): wave-uniform, walked on the scalar side; four reads in
            // flight while it has four bits left
            uint32_t f = __builtin_amdgcn_readfirstlane(F[(row0 + r) * stride + c]);
            while (__builtin_popcount(f) >= 4) {
                uint32_t v[4][LW];
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) {
                    load_words<LW>(&lds[buf][__builtin_ctz(f)][lane * LW], v[u]);
                    f &= f - 1u;
                }
#pragma unroll
                for (uint32_t q = 0; q < LW; q++) acc[r][q] |= (v[0][q] | v[1][q]) | (v[2][q] | v[3][q]);
            }
            for (; f; f &= f - 1u) {
                uint32_t v[LW];
                load_words<LW>(&lds[buf][__builtin_ctz(f)][lane * LW], v);
#pragma unroll
                for (uint32_t q = 0; q < LW; q++) acc[r][q] |= v[q];
            }
        }
        buf ^= 1u;  // (the next staging writes the other buffer: a wave still reading this one is safe)
        c = cn, need = need_n;
    }

    uint32_t t_or[LW], cnt = 0;
#pragma unroll
    for (uint32_t q = 0; q < LW; q++) t_or[q] = 0;
#pragma unroll
    for (uint32_t r = 0; r < kClosureWaveRows; r++) {
        const uint32_t i = row0 + r;
        if (i >= n) break;  // (uniform)
        uint32_t any_new = 0;
        if (in) {
            uint32_t nw[LW], any_acc = 0;
#pragma unroll
            for (uint32_t q = 0; q < LW; q++) nw[q] = 0, any_acc |= acc[r][q];
            uint32_t* rp = R + i * stride + my_w;
            if (any_acc) {
                uint32_t reached[LW];
                load_words<LW>(rp, reached);
#pragma unroll
                for (uint32_t q = 0; q < LW; q++) {
                    nw[q] = closure_new(acc[r][q], reached[q]);
                    reached[q] |= nw[q];
                    any_new |= nw[q];
                }
                if (any_new) store_words<LW>(rp, reached);  // (this lane owns these words: no atomics)
            }
            store_words<LW>(Fn + i * stride + my_w, nw);
#pragma unroll
            for (uint32_t q = 0; q < LW; q++) {
                t_or[q] |= nw[q];
                cnt += (uint32_t)__builtin_popcount(nw[q]);
                if constexpr (HOPS)
                    if (nw[q]) store_hops(hops, n, i, my_w + q, nw[q], level);
            }
        }
        if (__any(any_new != 0) && lane == 0) live_n[i] = 1u;  // (every writer stores the same value)
    }

    // the tile's new T words: the OR over the waves, through the staging buffer
    __syncthreads();  // (every wave has left the k loop)
    uint32_t* sh_t = &lds[0][0][0];                                         // [waves][kTileWords]
    uint64_t* sh_c = reinterpret_cast<uint64_t*>(&lds[1][0][0]);            // [waves]
    store_words<LW>(sh_t + wave * kTileWords + lane * LW, t_or);
    __syncthreads();
    if (wave == 0 && in) {
#pragma unroll
        for (uint32_t v = 1; v < kClosureWaves; v++) {
            uint32_t o[LW];
            load_words<LW>(sh_t + v * kTileWords + lane * LW, o);
#pragma unroll
            for (uint32_t q = 0; q < LW; q++) t_or[q] |= o[q];
        }
        store_words<LW>(Tn + blockIdx.y * stride + my_w, t_or);
    }
    block_add<kClosureWaves>(cnt, sh_c, total);
}

template <bool COUNT>
__global__ __launch_bounds__(kClosureBlock) void k_closure_pack(const uint32_t* __restrict__ R, uint32_t n, uint32_t stride,
                                                                uint32_t* __restrict__ out_packed,
                                                                uint32_t* __restrict__ out_count) {
    __shared__ uint32_t sh[kClosureBlock / 64];
    const uint32_t i = blockIdx.x, rw = (n + 15u) / 16u;
    uint32_t cnt = 0;
    for (uint32_t jw = threadIdx.x; jw < rw; jw += kClosureBlock) {
        const uint32_t h = (R[i * stride + (jw >> 1)] >> (16u * (jw & 1u))) & 0xFFFFu;  // (padding bits of R are zero)
        out_packed[i * rw + jw] = closure_expand(h);
        cnt += (uint32_t)__builtin_popcount(h);
    }
    if constexpr (COUNT) {
        const uint32_t ws = (uint32_t)wave_sum(cnt);
        if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = ws;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t s = 0;
#pragma unroll
            for (uint32_t v = 0; v < kClosureBlock / 64; v++) s += sh[v];
            out_count[i] = s;
        }
    }
}

struct StepArgs {
    const uint32_t *A, *F, *T, *live;
    uint32_t *R, *Fn, *Tn, *live_n;
    uint16_t* hops;
    unsigned long long* total;
    uint32_t n, stride, level;
};
template <uint32_t LW>
void launch_step(const ClosurePlan& p, hipStream_t st, const StepArgs& a) {
    const dim3 grid(p.col_tiles, p.row_tiles);
    if (a.hops)
        hipLaunchKernelGGL((k_closure_step<LW, true>), grid, dim3(kClosureStepBlock), 0, st, a.A, a.F, a.T, a.live, a.R, a.Fn,
                           a.Tn, a.live_n, a.hops, a.total, a.n, a.stride, a.level);
    else
        hipLaunchKernelGGL((k_closure_step<LW, false>), grid, dim3(kClosureStepBlock), 0, st, a.A, a.F, a.T, a.live, a.R, a.Fn,
                           a.Tn, a.live_n, a.hops, a.total, a.n, a.stride, a.level);
}

}  // namespace

int dev_reach_closure(const ClosureSpecDev& spec, uint32_t* out_packed, uint16_t* out_hops, uint32_t* out_count,
                      ClosureResult* res, void* stream, std::string* err) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = spec.n, stride = closure_stride(n);
    const ClosurePlan p = closure_plan(n);
    // TOTAL: the running popcount, a u64 cleared as 16 B; FN / TN / LIVE_N: the next level's F / T / live
    enum { TOTAL, MAT_A, MAT_R, MAT_F, MAT_FN, TILE_T, TILE_TN, LIVE, LIVE_N, LIST };
    const size_t mat = (size_t)n * stride * sizeof(uint32_t), tiles = (size_t)p.row_tiles * stride * sizeof(uint32_t);
    const size_t flags = (((size_t)n + 3) & ~(size_t)3) * sizeof(uint32_t);  // (cleared whole)
    const auto l = lay_out({16, mat, mat, mat, mat, tiles, tiles, flags, flags, spec.n_list * sizeof(uint32_t)});
    Scratch blk;
    if (Scratch::make(&blk, l.total, err) != 0) {
        (void)hipGetLastError();
        return -2;
    }
    unsigned long long* total = l.at<unsigned long long>(blk, TOTAL);
    uint32_t *A = l.at<uint32_t>(blk, MAT_A), *R = l.at<uint32_t>(blk, MAT_R), *F = l.at<uint32_t>(blk, MAT_F),
             *Fn = l.at<uint32_t>(blk, MAT_FN), *T = l.at<uint32_t>(blk, TILE_T), *Tn = l.at<uint32_t>(blk, TILE_TN),
             *live = l.at<uint32_t>(blk, LIVE), *live_n = l.at<uint32_t>(blk, LIVE_N), *list = l.at<uint32_t>(blk, LIST);
    HIPCHK(hipMemsetAsync(total, 0, 16, st));
    HIPCHK(hipMemsetAsync(live, 0, flags, st));
    if (spec.n_list) HIPCHK(hipMemcpyAsync(list, spec.svc_list, spec.n_list * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (out_hops) HIPCHK(hipMemsetAsync(out_hops, 0, (size_t)n * n * sizeof(uint16_t), st));
    const dim3 eg((stride + kEdgeWords - 1) / kEdgeWords, p.row_tiles);
    if (out_hops)
        hipLaunchKernelGGL(k_closure_edges<true>, eg, dim3(kClosureBlock), 0, st, spec.matrix, list, spec.n_list, n, stride, A,
                           R, F, T, live, out_hops, total);
    else
        hipLaunchKernelGGL(k_closure_edges<false>, eg, dim3(kClosureBlock), 0, st, spec.matrix, list, spec.n_list, n, stride,
                           A, R, F, T, live, out_hops, total);
    HIPCHK(hipGetLastError());
    uint64_t reached = 0;
    HIPCHK(hipMemcpyAsync(&reached, total, sizeof reached, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    res->n_edges = reached;
    uint32_t level = reached ? 1u : 0u;
    // (a shortest path has at most n edges: the loop ends by itself)
    for (uint64_t fresh = reached; fresh && (!spec.max_hops || level < spec.max_hops);) {
        HIPCHK(hipMemsetAsync(live_n, 0, flags, st));
        const StepArgs a{A, F, T, live, R, Fn, Tn, live_n, out_hops, total, n, stride, level + 1u};
        if (p.lane_words == 1) launch_step<1>(p, st, a);
        else if (p.lane_words == 2) launch_step<2>(p, st, a);
        else launch_step<4>(p, st, a);
        HIPCHK(hipGetLastError());
        uint64_t now = 0;
        HIPCHK(hipMemcpyAsync(&now, total, sizeof now, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        fresh = now - reached;
        reached = now;
        if (fresh) level++;
        std::swap(F, Fn), std::swap(T, Tn), std::swap(live, live_n);
    }
    if (out_count) hipLaunchKernelGGL(k_closure_pack<true>, dim3(n), dim3(kClosureBlock), 0, st, R, n, stride, out_packed, out_count);
    else hipLaunchKernelGGL(k_closure_pack<false>, dim3(n), dim3(kClosureBlock), 0, st, R, n, stride, out_packed, out_count);
    HIPCHK(hipGetLastError());
    if (blk.finish(st, "reach closure", err) != 0) return -1;
    res->levels = level;
    res->n_reachable = reached;
    return 0;
}

}  // namespace pg
