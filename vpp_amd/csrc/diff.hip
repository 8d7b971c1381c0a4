// gfx950 kernels of the reachability diff (pg_reach_diff; diff.hpp has the per-word code).
//
// The word array is cut into one contiguous chunk per workgroup (diff_plan: the resident
// workgroups, chunks a multiple of the 1024-word tile). Three launches, none of which waits on
// another workgroup:
//  k_diff_count  per chunk the number of selected cells; with HIST the 16 histogram values, summed
//                per lane, across the wave by shuffles, across the waves through LDS, one u64 atomic
//                per counter per workgroup; with ROWS every word's non-zero count added to its row
//                by a u32 atomic (the array cleared on the stream first)
//  k_diff_scan   one workgroup: the exclusive scan of the chunk counts in u64, and the total
//  k_diff_emit   the same chunks again: per tile the masks recomputed, a workgroup exclusive scan
//                of the lanes' counts (wave shuffles, then LDS across the four waves) on a running
//                base, and every lane stores its words' entries in ascending column order, 8 B each;
//                entries at or past `cap` are dropped, and a workgroup stops once its base is there
// A lane owns 4 consecutive words of a tile: one 16-B load per input where both are 16-B aligned
// (VEC), four 4-B loads otherwise. Word -> (row, first column) is one 32-bit division per lane and
// tile, then a carry.
//
// No kernel reads a table or touches a hit counter. (The driver's error macro, CU count, occupancy
// query and scratch-block owner: hiputil.hpp.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "diff.hpp"
#include "hiputil.hpp"

namespace pg {

namespace {

constexpr uint32_t kDiffWaves = kDiffBlock / 64;

// a lane's 4 words of both inputs, starting at word w0 < n_words; words past the end read as 0
template <bool VEC>
__device__ __forceinline__ void diff_load(const uint32_t* __restrict__ before, const uint32_t* __restrict__ after,
                                          uint64_t w0, uint32_t n_words, uint32_t (&b)[kDiffLaneWords],
                                          uint32_t (&a)[kDiffLaneWords]) {
    if (VEC && w0 + kDiffLaneWords <= n_words) {  // (chunks and tiles start at multiples of 4 words)
        const uint4 qb = *reinterpret_cast<const uint4*>(before + w0);
        const uint4 qa = *reinterpret_cast<const uint4*>(after + w0);
        b[0] = qb.x, b[1] = qb.y, b[2] = qb.z, b[3] = qb.w;
        a[0] = qa.x, a[1] = qa.y, a[2] = qa.z, a[3] = qa.w;
    } else {
#pragma unroll
        for (uint32_t q = 0; q < kDiffLaneWords; q++) {
            const bool in = w0 + q < n_words;
            b[q] = in ? before[w0 + q] : 0u;
            a[q] = in ? after[w0 + q] : 0u;
        }
    }
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;  // (lane 0 has the sum)
}

template <bool HIST, bool ROWS, bool VEC>
__global__ __launch_bounds__(kDiffBlock) void k_diff_count(const uint32_t* __restrict__ before,
                                                           const uint32_t* __restrict__ after, DiffShape S,
                                                           uint64_t chunk_words, uint64_t* __restrict__ chunk_counts,
                                                           unsigned long long* __restrict__ trans,
                                                           uint32_t* __restrict__ row_changes) {
    __shared__ uint64_t sh[kDiffWaves][17];
    const uint64_t c0 = (uint64_t)blockIdx.x * chunk_words, c1 = c0 + chunk_words < S.n_words ? c0 + chunk_words : S.n_words;
    // a lane sees at most chunk_words / 256 words of 16 cells: its sums fit 32 bits
    uint32_t h[16] = {0}, cnt = 0;
    for (uint64_t t0 = c0; t0 < c1; t0 += kDiffTile) {
        const uint64_t w0 = t0 + kDiffLaneWords * threadIdx.x;
        if (w0 >= S.n_words) continue;
        uint32_t b[kDiffLaneWords], a[kDiffLaneWords];
        diff_load<VEC>(before, after, w0, S.n_words, b, a);
        uint32_t row = (uint32_t)w0 / S.row_words, jw = (uint32_t)w0 - row * S.row_words;
#pragma unroll
        for (uint32_t q = 0; q < kDiffLaneWords; q++) {
            if (w0 + q < S.n_words) {
                const uint32_t valid = diff_valid(S.n_cols, jw);
                if (b[q] == a[q]) {  // nothing selected, and of the histogram only the diagonal
                    if constexpr (HIST) diff_hist_same(diff_eq(b[q]), valid, h);
                } else {
                    const DiffEq eb = diff_eq(b[q]), ea = diff_eq(a[q]);
                    const uint32_t c = (uint32_t)__builtin_popcount(diff_selected(eb, ea, b[q] ^ a[q], valid, S.transitions));
                    cnt += c;
                    if constexpr (HIST) diff_hist(eb, ea, valid, h);
                    if constexpr (ROWS)
                        if (c) atomicAdd(row_changes + row, c);
                }
            }
            if (++jw == S.row_words) jw = 0, row++;
        }
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t ws = wave_sum(cnt);
    if (lane == 0) sh[wave][16] = ws;
    if constexpr (HIST) {
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            const uint64_t s = wave_sum(h[k]);
            if (lane == 0) sh[wave][k] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < 17u && (HIST || threadIdx.x == 16u)) {
        uint64_t s = 0;
#pragma unroll
        for (uint32_t v = 0; v < kDiffWaves; v++) s += sh[v][threadIdx.x];
        if (threadIdx.x == 16u) chunk_counts[blockIdx.x] = s;
        else if (s) atomicAdd(trans + threadIdx.x, (unsigned long long)s);
    }
}

// counts[0 .. n - 1] -> their exclusive prefix sums, counts[n] = the total. One workgroup: every lane
// takes ceil(n / 256) consecutive values
__global__ __launch_bounds__(kDiffBlock) void k_diff_scan(uint64_t* __restrict__ counts, uint32_t n) {
    __shared__ uint64_t sh[kDiffWaves];
    const uint32_t per = (n + kDiffBlock - 1) / kDiffBlock;
    const uint32_t i0 = threadIdx.x * per < n ? threadIdx.x * per : n, i1 = i0 + per < n ? i0 + per : n;
    uint64_t own = 0;
    for (uint32_t i = i0; i < i1; i++) own += counts[i];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(inc, d);
        if ((int)lane >= d) inc += t;
    }
    if (lane == 63u) sh[wave] = inc;
    __syncthreads();
    uint64_t run = inc - own;
    for (uint32_t v = 0; v < wave; v++) run += sh[v];
    for (uint32_t i = i0; i < i1; i++) {
        const uint64_t c = counts[i];
        counts[i] = run;
        run += c;
    }
    if (threadIdx.x == kDiffBlock - 1) counts[n] = run;  // (the last lane's prefix and its own: everything)
}

template <bool VEC>
__global__ __launch_bounds__(kDiffBlock) void k_diff_emit(const uint32_t* __restrict__ before,
                                                          const uint32_t* __restrict__ after, DiffShape S,
                                                          uint64_t chunk_words, const uint64_t* __restrict__ chunk_base,
                                                          uint64_t cap, DiffEntry* __restrict__ changes) {
    __shared__ uint32_t sh[kDiffWaves];
    const uint64_t c0 = (uint64_t)blockIdx.x * chunk_words, c1 = c0 + chunk_words < S.n_words ? c0 + chunk_words : S.n_words;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t base = chunk_base[blockIdx.x];
    // (t0, base and cap are the same in every lane: the workgroup leaves the loop together)
    for (uint64_t t0 = c0; t0 < c1 && base < cap; t0 += kDiffTile) {
        const uint64_t w0 = t0 + kDiffLaneWords * threadIdx.x;
        uint32_t b[kDiffLaneWords] = {0, 0, 0, 0}, a[kDiffLaneWords] = {0, 0, 0, 0}, sel[kDiffLaneWords] = {0, 0, 0, 0};
        uint32_t row = 0, jw = 0, c = 0;
        if (w0 < S.n_words) {
            diff_load<VEC>(before, after, w0, S.n_words, b, a);
            row = (uint32_t)w0 / S.row_words, jw = (uint32_t)w0 - row * S.row_words;
            uint32_t r = row, j = jw;
#pragma unroll
            for (uint32_t q = 0; q < kDiffLaneWords; q++) {
                if (w0 + q < S.n_words) {
                    sel[q] = diff_selected(diff_eq(b[q]), diff_eq(a[q]), b[q] ^ a[q], diff_valid(S.n_cols, j), S.transitions);
                    c += (uint32_t)__builtin_popcount(sel[q]);
                }
                if (++j == S.row_words) j = 0, r++;
            }
        }
        uint32_t inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d);
            if ((int)lane >= d) inc += t;
        }
        if (lane == 63u) sh[wave] = inc;
        __syncthreads();
        uint32_t before_me = inc - c, total = 0;
#pragma unroll
        for (uint32_t v = 0; v < kDiffWaves; v++) {
            const uint32_t s = sh[v];
            if (v < wave) before_me += s;
            total += s;
        }
        __syncthreads();  // sh is written again in the next tile
        uint64_t o = base + before_me;
#pragma unroll
        for (uint32_t q = 0; q < kDiffLaneWords; q++) {
            for (uint32_t m = sel[q]; m; m &= m - 1u) {
                const uint32_t bit = (uint32_t)__builtin_ctz(m);
                if (o < cap) *reinterpret_cast<uint2*>(changes + o) = make_uint2(row, diff_cell(jw, bit, b[q], a[q]));
                o++;
            }
            if (++jw == S.row_words) jw = 0, row++;
        }
        base += total;
    }
}

// both passes run on one partition: the occupancy of the larger count kernel and of the emit kernel
uint32_t diff_resident(uint32_t blocks_per_cu) {
    int per_cu = std::max(1, occupancy(k_diff_count<true, true, false>, kDiffBlock, 0));
    if (const int pe = occupancy(k_diff_emit<false>, kDiffBlock, 0)) per_cu = std::min(per_cu, pe);
    (void)hipGetLastError();  // (a failed query is answered by the fall-back above)
    if (blocks_per_cu) per_cu = std::min<int>(per_cu, (int)blocks_per_cu);
    return num_cus() * (uint32_t)per_cu;
}

template <bool HIST, bool ROWS>
void launch_count(bool vec, const DiffPlan& p, hipStream_t st, const uint32_t* before, const uint32_t* after,
                  const DiffShape& S, uint64_t* counts, unsigned long long* trans, uint32_t* row_changes) {
    if (vec)
        hipLaunchKernelGGL((k_diff_count<HIST, ROWS, true>), dim3(p.grid), dim3(kDiffBlock), 0, st, before, after, S,
                           p.chunk_words, counts, trans, row_changes);
    else
        hipLaunchKernelGGL((k_diff_count<HIST, ROWS, false>), dim3(p.grid), dim3(kDiffBlock), 0, st, before, after, S,
                           p.chunk_words, counts, trans, row_changes);
}

}  // namespace

DiffPlan dev_diff_plan(uint64_t n_words, uint32_t blocks_per_cu) { return diff_plan(n_words, diff_resident(blocks_per_cu)); }

int dev_reach_diff(uint32_t blocks_per_cu, const DiffSpecDev& spec, DiffEntry* changes, uint32_t* row_changes,
                   uint64_t* n_changes, uint64_t* trans, void* stream, std::string* err) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t rw = (spec.n_cols + 15u) / 16u;
    const DiffShape S{spec.n_rows * rw, rw, spec.n_cols, spec.transitions};
    const DiffPlan p = dev_diff_plan(S.n_words, blocks_per_cu);
    const bool vec = (((uintptr_t)spec.before | (uintptr_t)spec.after) & 15u) == 0;
    // one scratch block: [chunk counts, then bases, u64[grid] | total u64 | trans u64[16]]; the total
    // and the histogram come back in one copy
    const size_t n_back = 1 + (trans ? 16 : 0);
    Scratch blk;
    if (Scratch::make(&blk, ((size_t)p.grid + 17) * sizeof(uint64_t), err) != 0) return -1;
    uint64_t* d = blk.at<uint64_t>(0);
    uint64_t back[17] = {0};
    unsigned long long* dt = reinterpret_cast<unsigned long long*>(d + p.grid + 1);
    if (trans) HIPCHK(hipMemsetAsync(dt, 0, 16 * sizeof(uint64_t), st));
    if (row_changes) HIPCHK(hipMemsetAsync(row_changes, 0, (size_t)spec.n_rows * sizeof(uint32_t), st));
    if (trans && row_changes) launch_count<true, true>(vec, p, st, spec.before, spec.after, S, d, dt, row_changes);
    else if (trans) launch_count<true, false>(vec, p, st, spec.before, spec.after, S, d, dt, row_changes);
    else if (row_changes) launch_count<false, true>(vec, p, st, spec.before, spec.after, S, d, dt, row_changes);
    else launch_count<false, false>(vec, p, st, spec.before, spec.after, S, d, dt, row_changes);
    hipLaunchKernelGGL(k_diff_scan, dim3(1), dim3(kDiffBlock), 0, st, d, p.grid);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(back, d + p.grid, n_back * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (changes && spec.cap && back[0]) {
        if (vec)
            hipLaunchKernelGGL(k_diff_emit<true>, dim3(p.grid), dim3(kDiffBlock), 0, st, spec.before, spec.after, S,
                               p.chunk_words, d, spec.cap, changes);
        else
            hipLaunchKernelGGL(k_diff_emit<false>, dim3(p.grid), dim3(kDiffBlock), 0, st, spec.before, spec.after, S,
                               p.chunk_words, d, spec.cap, changes);
        HIPCHK(hipGetLastError());
    }
    // (the emit pass reads the chunk bases in the block: Scratch)
    if (blk.finish(st, "reach diff", err) != 0) return -1;
    *n_changes = back[0];
    if (trans) std::copy(back + 1, back + 17, trans);
    return 0;
}

}  // namespace pg
