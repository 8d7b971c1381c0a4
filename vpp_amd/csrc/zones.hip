// gfx950 kernels of the reachability zones (pg_reach_zones; zones.hpp has the definitions, the
// per-word code and the plan).
//
// Two n x stride bit matrices in one scratch block: B (R as bits) and BT (its transpose).
//  k_zones_bits_t  the tiles (128 rows x 32 bit-words) cut into one contiguous run per workgroup, the
//                  grid the resident workgroups. Per tile a half wave reads 64 adjacent input words of
//                  one row, a lane makes one bit-word (zones_bit_word), stores it to B and to LDS. Then
//                  a wave takes two bit-word columns of the tile at a time: its lanes read one word of
//                  64 consecutive rows each from LDS (pitch 33: no bank conflict), and one wave-wide
//                  ballot per column of the word gives 64 rows of that column, two adjacent words of a
//                  BT row. Lane k keeps the ballots of its column for both halves of the tile: four
//                  adjacent BT words, one aligned 16-B store per lane, all 64 lanes storing. The input
//                  is read once; every word of B and BT is written, padding zero.
//  k_zones_label   a wave per row i, a workgroup four rows at a time, grid-stride. A pass ANDs 64
//                  adjacent words of B[i] and BT[i]; the first pass with a bit ends the search
//                  (zones_label), and only the words 0 .. i / 32 are read. With counts the wave goes on
//                  over the whole of both rows and leaves their popcounts in scratch. mark[label] = 1:
//                  every writer stores the same value into an array cleared on the stream first.
//  k_zones_number  one workgroup of 1024: an exclusive scan of mark[] (a thread sums its run, a shuffle
//                  scan per wave, the waves' totals through LDS) gives the ids and out_rep; then
//                  out_zone[i] = id[label[i]], the sizes by integer atomics (in LDS up to 4096 zones, in
//                  scratch beyond), the popcounts gathered at the representatives, and the result words.
//  k_zones_dag     a workgroup per zone a, grid-stride up to the zone count that k_zones_number left
//                  in device memory: row rep[a] of B staged in LDS (at most 4 KiB), a lane per output
//                  word (zones_dag_word).
// No workgroup waits on another. The host reads nothing back before the end: one synchronisation.
//
// No kernel reads a table or touches a hit counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "audit_launch.hpp"
#include "zones.hpp"

namespace pg {

namespace {

struct ZonesShape {
    uint32_t n, rw, stride;          // rw: input words of a row
    uint32_t col_tiles, items, per;  // all tiles; those of one workgroup
};

__global__ __launch_bounds__(kZonesBlock) void k_zones_bits_t(const uint32_t* __restrict__ matrix, ZonesShape S,
                                                              uint32_t* __restrict__ B, uint32_t* __restrict__ BT) {
    __shared__ uint32_t sh[kZonesTileRows][kZonesTilePitch];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t wl = threadIdx.x % kZonesTileWords, ph = threadIdx.x / kZonesTileWords;
    const uint32_t it0 = blockIdx.x * S.per, it1 = min(it0 + S.per, S.items);
    for (uint32_t it = it0; it < it1; it++) {
        const uint32_t tr = it / S.col_tiles, tc = it - tr * S.col_tiles;
        const uint32_t r0 = tr * kZonesTileRows, w0 = tc * kZonesTileWords;
        __syncthreads();  // (every wave has left the tile before)
        const uint32_t w = w0 + wl;
#pragma unroll 4
        for (uint32_t r = ph; r < kZonesTileRows; r += kZonesBlock / kZonesTileWords) {
            const uint32_t i = r0 + r;
            uint32_t x = 0;
            if (i < S.n && w < S.stride) {
                x = zones_bit_word(matrix + (size_t)i * S.rw, S.rw, S.n, w);
                B[i * S.stride + w] = x;
            }
            sh[r][wl] = x;
        }
        __syncthreads();
        // words q and q + 1 of the tile: lanes 0..31 end with the columns of q, lanes 32..63 with those of q + 1
        for (uint32_t q = 2u * wave; q < kZonesTileWords; q += 2u * kZonesWaves) {
            uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
#pragma unroll
            for (uint32_t s = 0; s < 2; s++) {
                const uint32_t x0 = sh[lane][q + s], x1 = sh[64u + lane][q + s];
#pragma unroll
                for (uint32_t k = 0; k < 32; k++) {
                    const unsigned long long b0 = __ballot(zones_ballot_bit(x0, k)), b1 = __ballot(zones_ballot_bit(x1, k));
                    if (lane == 32u * s + k) v0 = (uint32_t)b0, v1 = (uint32_t)(b0 >> 32), v2 = (uint32_t)b1, v3 = (uint32_t)(b1 >> 32);
                }
            }
            const uint32_t c = 32u * (w0 + q) + lane;
            // (stride is a multiple of 4 and the tile's rows are words 4 tr .. 4 tr + 3 of a BT row: inside it, 16-B aligned)
            if (c < S.n) *reinterpret_cast<uint4*>(BT + c * S.stride + 4u * tr) = make_uint4(v0, v1, v2, v3);
        }
    }
}

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

template <bool COUNTS>
__global__ __launch_bounds__(kZonesBlock) void k_zones_label(const uint32_t* __restrict__ B, const uint32_t* __restrict__ BT,
                                                             uint32_t n, uint32_t stride, uint32_t bit_words,
                                                             uint32_t* __restrict__ label, uint32_t* __restrict__ mark,
                                                             uint32_t* __restrict__ cnt_b, uint32_t* __restrict__ cnt_bt) {
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t i = blockIdx.x * kZonesLabelRows + wave; i < n; i += gridDim.x * kZonesLabelRows) {
        const uint32_t* __restrict__ rb = B + i * stride;
        const uint32_t* __restrict__ rt = BT + i * stride;
        const uint32_t last = i >> 5, end = COUNTS ? bit_words : last + 1u;
        uint32_t lab = i, cb = 0, ct = 0;
        bool found = false;  // (the same in every lane)
        for (uint32_t w0 = 0; w0 < end; w0 += 64u) {
            const uint32_t w = w0 + lane;
            uint32_t b = 0, t = 0;
            if (w < end) b = rb[w], t = rt[w];
            if constexpr (COUNTS) cb += (uint32_t)__popc(b), ct += (uint32_t)__popc(t);
            if (!found && w0 <= last) {
                const uint32_t m = w <= last ? b & t : 0u;
                const unsigned long long hit = __ballot(m != 0u);
                if (hit) {
                    const uint32_t src = (uint32_t)__ffsll((long long)hit) - 1u;
                    lab = zones_label(i, w0 + src, (uint32_t)__shfl((int)m, (int)src, 64));
                    found = true;
                }
            }
            if (!COUNTS && found) break;
        }
        if constexpr (COUNTS) cb = wave_sum(cb), ct = wave_sum(ct);
        if (lane == 0) {
            label[i] = lab;
            mark[lab] = 1u;
            if constexpr (COUNTS) cnt_b[i] = cb, cnt_bt[i] = ct;
        }
    }
}

struct ZonesNumberArgs {
    const uint32_t *label, *mark, *B, *cnt_b, *cnt_bt;
    uint32_t *zid, *zsize;  // scratch: the id of every marked end point; the sizes beyond kZonesLdsZones zones (cleared)
    uint32_t n, stride;
    uint32_t *zone, *rep, *size, *reaches, *reached_by;  // the outputs, null where not given
    uint32_t* result;                                    // scratch, kZonesResultWords
};

__global__ __launch_bounds__(kZonesNumberBlock) void k_zones_number(ZonesNumberArgs A) {
    constexpr uint32_t kWaves = kZonesNumberBlock / 64;
    __shared__ uint32_t sh_wave[kWaves];
    __shared__ uint32_t sh_hist[kZonesLdsZones];
    __shared__ uint32_t sh_red[4][kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t per = (A.n + kZonesNumberBlock - 1u) / kZonesNumberBlock;
    const uint32_t j0 = min(threadIdx.x * per, A.n), j1 = min(j0 + per, A.n);
    uint32_t cnt = 0;
    for (uint32_t j = j0; j < j1; j++) cnt += A.mark[j] != 0u;
    // exclusive scan of the threads' counts
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63u) sh_wave[wave] = incl;
    __syncthreads();
    uint32_t base = 0, n_zones = 0;
#pragma unroll
    for (uint32_t v = 0; v < kWaves; v++) {
        if (v < wave) base += sh_wave[v];
        n_zones += sh_wave[v];
    }
    const bool lds = n_zones <= kZonesLdsZones;
    uint32_t cyclic = 0;
    uint32_t at = base + incl - cnt;
    for (uint32_t j = j0; j < j1; j++) {
        if (!A.mark[j]) continue;
        A.zid[j] = at;
        if (A.rep) A.rep[at] = j;
        if (A.reaches) A.reaches[at] = A.cnt_b[j];
        if (A.reached_by) A.reached_by[at] = A.cnt_bt[j];
        cyclic += zones_bit(A.B + j * A.stride, j);
        at++;
    }
    if (lds)
        for (uint32_t z = threadIdx.x; z < n_zones; z += kZonesNumberBlock) sh_hist[z] = 0u;
    __threadfence();
    __syncthreads();  // (the ids are out)
    uint32_t broken = 0;
    for (uint32_t i = threadIdx.x; i < A.n; i += kZonesNumberBlock) {
        const uint32_t l = A.label[i], z = A.zid[l];
        A.zone[i] = z;
        broken += A.label[l] != l;
        if (lds) atomicAdd(&sh_hist[z], 1u);
        else atomicAdd(&A.zsize[z], 1u);
    }
    __threadfence();
    __syncthreads();
    uint32_t multi = 0, largest = 0;
    for (uint32_t z = threadIdx.x; z < n_zones; z += kZonesNumberBlock) {
        const uint32_t s = lds ? sh_hist[z] : atomicAdd(&A.zsize[z], 0u);  // (read where the adds went)
        if (A.size) A.size[z] = s;
        multi += s > 1u;
        largest = max(largest, s);
    }
    cyclic = wave_sum(cyclic), multi = wave_sum(multi), broken = wave_sum(broken), largest = wave_max(largest);
    if (lane == 0) sh_red[0][wave] = cyclic, sh_red[1][wave] = multi, sh_red[2][wave] = largest, sh_red[3][wave] = broken;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0, m = 0, l = 0, b = 0;
        for (uint32_t v = 0; v < kWaves; v++) c += sh_red[0][v], m += sh_red[1][v], l = max(l, sh_red[2][v]), b += sh_red[3][v];
        A.result[0] = n_zones, A.result[1] = c, A.result[2] = m, A.result[3] = l, A.result[4] = b;
    }
}

__global__ __launch_bounds__(kZonesBlock) void k_zones_dag(const uint32_t* __restrict__ B, uint32_t stride,
                                                           const uint32_t* __restrict__ rep, const uint32_t* __restrict__ result,
                                                           uint32_t* __restrict__ dag) {
    __shared__ uint32_t row[kClosureMaxN / 32u];
    const uint32_t n_zones = __builtin_amdgcn_readfirstlane(result[0]), rwz = (n_zones + 15u) / 16u;
    for (uint32_t a = blockIdx.x; a < n_zones; a += gridDim.x) {
        __syncthreads();  // (every lane has left the row of the zone before)
        const uint32_t* __restrict__ src = B + rep[a] * stride;
        for (uint32_t w = threadIdx.x; w < stride; w += kZonesBlock) row[w] = src[w];
        __syncthreads();
        for (uint32_t ow = threadIdx.x; ow < rwz; ow += kZonesBlock) {
            const uint32_t left = n_zones - 16u * ow;
            dag[a * rwz + ow] = zones_dag_word(row, rep + 16u * ow, left < 16u ? left : 16u);
        }
    }
}

}  // namespace

int dev_reach_zones(uint32_t blocks_per_cu, const uint32_t* matrix, uint32_t n, const ZonesOutDev& out, ZonesResult* result,
                    void* stream, std::string* err) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t stride = closure_stride(n), bw = closure_bit_words(n), rw = (n + 15u) / 16u;
    const ZonesPlan plan = zones_plan(n);
    const bool counts = out.reaches || out.reached_by;
    // (before blk: a call that leaves early still outlives the copy into it)
    uint32_t res[kZonesResultWords] = {};
    Scratch blk;
    // MARK and ZSIZE are adjacent: one memset clears both (ZSIZE: the sizes beyond kZonesLdsZones zones)
    enum { MAT_B, MAT_BT, MARK, ZSIZE, LABEL, ZID, CNT_B, CNT_BT, RESULT };
    const size_t mat = (size_t)n * stride * sizeof(uint32_t), vec = (size_t)n * sizeof(uint32_t);
    const auto l = lay_out({mat, mat, vec, vec, vec, vec, vec, vec, kZonesResultWords * sizeof(uint32_t)});
    if (Scratch::make(&blk, l.total, err) != 0) {
        (void)hipGetLastError();
        return -2;
    }
    uint32_t *B = l.at<uint32_t>(blk, MAT_B), *BT = l.at<uint32_t>(blk, MAT_BT), *d_res = l.at<uint32_t>(blk, RESULT);
    uint32_t *d_mark = l.at<uint32_t>(blk, MARK), *d_label = l.at<uint32_t>(blk, LABEL);
    uint32_t *d_cb = l.at<uint32_t>(blk, CNT_B), *d_ct = l.at<uint32_t>(blk, CNT_BT);
    HIPCHK(hipMemsetAsync(d_mark, 0, l.off[LABEL] - l.off[MARK], st));

    ZonesShape S{n, rw, stride, plan.col_tiles, plan.bits_grid, 0};
    const Runs runs = run_grid(k_zones_bits_t, (int)kZonesBlock, 0, S.items, blocks_per_cu);
    S.per = (uint32_t)runs.per;
    hipLaunchKernelGGL(k_zones_bits_t, dim3((uint32_t)runs.groups), dim3(kZonesBlock), 0, st, matrix, S, B, BT);
    HIPCHK(hipGetLastError());

    auto label = [&](auto kernel) {
        const int g = grid_resident(kernel, (int)kZonesBlock, 0, (uint64_t)plan.label_grid * kZonesBlock, blocks_per_cu);
        (void)hipGetLastError();
        hipLaunchKernelGGL(kernel, dim3(g), dim3(kZonesBlock), 0, st, B, BT, n, stride, bw, d_label, d_mark, d_cb, d_ct);
    };
    if (counts) label(k_zones_label<true>);
    else label(k_zones_label<false>);
    HIPCHK(hipGetLastError());

    const ZonesNumberArgs A{d_label, d_mark, B, d_cb, d_ct, l.at<uint32_t>(blk, ZID), l.at<uint32_t>(blk, ZSIZE), n, stride,
                            out.zone, out.rep, out.size, out.reaches, out.reached_by, d_res};
    hipLaunchKernelGGL(k_zones_number, dim3(1), dim3(kZonesNumberBlock), 0, st, A);
    HIPCHK(hipGetLastError());

    if (out.dag) {
        const int grid = grid_resident(k_zones_dag, (int)kZonesBlock, 0, (uint64_t)plan.dag_grid * kZonesBlock, blocks_per_cu);
        (void)hipGetLastError();
        hipLaunchKernelGGL(k_zones_dag, dim3(grid), dim3(kZonesBlock), 0, st, B, stride, out.rep, d_res, out.dag);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(res, d_res, sizeof(res), hipMemcpyDeviceToHost, st));
    if (blk.finish(st, "reach zones", err) != 0) return -1;
    *result = ZonesResult{res[0], res[1], res[2], res[3], res[4]};
    return 0;
}

}  // namespace pg
