// gfx950 kernels of the reachability groups (pg_reach_groups; groups.hpp has the per-word code and
// the partition).
//
//  k_groups_count  the work items (service, chunk, column tile) in that order, cut into one
//                  contiguous run per workgroup, the grid the resident workgroups. Per item a lane
//                  owns one column word and walks its rows of the chunk (rows[] says which: the
//                  matrix rows sorted by src group), adjacent lanes on adjacent words, eight loads
//                  in flight, the counts in registers (groups_add). At the end of the item it adds
//                  its counts to the workgroup's LDS accumulators [dst group][code] (groups_flush:
//                  u32 LDS adds). The accumulators stay across the items of one (service, src group)
//                  and go to out_counts, one u64 atomic per non-zero cell, when that pair changes,
//                  after kGroupsRunItems items, and at the end of the run.
//  k_groups_pack   one lane per word of out_packed: the PG_GROUPS_* status of 16 pairs from their
//                  counts, padding zero. Launched only when out_packed is given.
// No workgroup waits on another; out_counts is cleared on the stream first. Loads are 4 B per lane:
// a lane that took four words would need four sets of counters, and a 4096-column row (256 words)
// would then fill one wave of a workgroup's four.
//
// No kernel reads a table or touches a hit counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "audit_launch.hpp"
#include "groups.hpp"

namespace pg {

namespace {

constexpr uint32_t kGroupsLoads = 8;  // row loads a lane keeps in flight

struct GroupsShape {
    uint32_t n_src, n_dst, row_words, n_src_groups, n_dst_groups;
    uint32_t tile_shift;  // tile_words = 1 << tile_shift
    uint32_t tiles, n_chunks;
    uint64_t items, per;  // all work items; those of one workgroup
};

__global__ __launch_bounds__(kGroupsBlock) void k_groups_count(const uint32_t* __restrict__ matrix, GroupsShape S,
                                                               const uint32_t* __restrict__ rows,
                                                               const GroupsChunk* __restrict__ chunks,
                                                               const uint16_t* __restrict__ dgrp,
                                                               unsigned long long* __restrict__ out_counts) {
    extern __shared__ __attribute__((aligned(16))) uint32_t acc_lds[];  // [n_dst_groups][4]
    const uint32_t cells = 4u * S.n_dst_groups;
    for (uint32_t i = threadIdx.x; i < cells; i += kGroupsBlock) acc_lds[i] = 0;
    __syncthreads();
    const uint32_t tile_words = 1u << S.tile_shift;
    const uint32_t col = threadIdx.x & (tile_words - 1u), phase = threadIdx.x >> S.tile_shift, phases = kGroupsBlock >> S.tile_shift;
    const uint64_t it0 = (uint64_t)blockIdx.x * S.per, it1 = it0 + S.per < S.items ? it0 + S.per : S.items;
    // (the item, its service and its chunk are the same in every lane: the barriers are uniform)
    uint32_t cur_v = 0, cur_gs = 0, since = 0;
    auto to_global = [&]() {
        unsigned long long* out = out_counts + ((uint64_t)cur_v * S.n_src_groups + cur_gs) * cells;
        for (uint32_t i = threadIdx.x; i < cells; i += kGroupsBlock) {
            const uint32_t n = acc_lds[i];
            if (n) {
                atomicAdd(out + i, (unsigned long long)n);
                acc_lds[i] = 0;
            }
        }
    };
    const uint64_t per_svc = (uint64_t)S.n_chunks * S.tiles;
    for (uint64_t it = it0; it < it1; it++) {
        const uint32_t v = (uint32_t)(it / per_svc);
        const uint64_t rem = it - (uint64_t)v * per_svc;
        const uint32_t ch = (uint32_t)(rem / S.tiles), tile = (uint32_t)(rem - (uint64_t)ch * S.tiles);
        const GroupsChunk c = chunks[ch];
        if (since && (v != cur_v || c.gs != cur_gs || since == kGroupsRunItems)) {
            __syncthreads();
            to_global();
            __syncthreads();
            since = 0;
        }
        cur_v = v, cur_gs = c.gs, since++;
        const uint32_t w = (tile << S.tile_shift) + col;
        if (w < S.row_words && c.r0 + phase < c.r1) {
            const uint32_t valid = diff_valid(S.n_dst, w);
            const uint32_t* __restrict__ base = matrix + (uint64_t)v * S.n_src * S.row_words + w;
            GroupsAcc a = {};
            uint32_t r = c.r0 + phase, n = 0;
            for (; r + (kGroupsLoads - 1u) * phases < c.r1; r += kGroupsLoads * phases) {
                uint32_t x[kGroupsLoads];
#pragma unroll
                for (uint32_t u = 0; u < kGroupsLoads; u++) x[u] = base[(uint64_t)rows[r + u * phases] * S.row_words];
#pragma unroll
                for (uint32_t u = 0; u < kGroupsLoads; u++) groups_add(a, x[u], valid);
                n += kGroupsLoads;
            }
            for (; r < c.r1; r += phases, n++) groups_add(a, base[(uint64_t)rows[r] * S.row_words], valid);
            const uint4* gp = reinterpret_cast<const uint4*>(dgrp + 16u * (size_t)w);
            const uint4 g0 = gp[0], g1 = gp[1];
            const uint32_t gw[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            groups_flush(a, n, gw, [&](uint32_t g, uint32_t code, uint32_t cnt) { atomicAdd(&acc_lds[4u * g + code], cnt); });
        }
    }
    if (since) {
        __syncthreads();
        to_global();
    }
}

__global__ __launch_bounds__(kGroupsBlock) void k_groups_pack(const uint64_t* __restrict__ counts, uint32_t n_rows,
                                                              uint32_t n_dst_groups, uint32_t* __restrict__ out_packed) {
    const uint32_t rw = (n_dst_groups + 15u) / 16u;
    const uint64_t n_words = (uint64_t)n_rows * rw;
    for (uint64_t o = (uint64_t)blockIdx.x * kGroupsBlock + threadIdx.x; o < n_words; o += (uint64_t)gridDim.x * kGroupsBlock) {
        const uint32_t row = (uint32_t)(o / rw), jw = (uint32_t)(o - (uint64_t)row * rw);
        out_packed[o] = groups_pack_word(counts + (uint64_t)row * n_dst_groups * 4u, n_dst_groups, jw);
    }
}

}  // namespace

int dev_reach_groups(uint32_t blocks_per_cu, const GroupsSpecDev& spec, uint64_t* out_counts, uint32_t* out_packed,
                     void* stream, std::string* err) {
    hipStream_t st = (hipStream_t)stream;
    const GroupsPartition& P = *spec.part;
    const uint32_t n_pair_rows = spec.n_svc * spec.n_src_groups;  // (n_svc * n_sg * n_dg < 2^30: the host checks)
    const size_t n_counts = (size_t)n_pair_rows * spec.n_dst_groups * 4u;
    HIPCHK(hipMemsetAsync(out_counts, 0, n_counts * sizeof(uint64_t), st));
    const GroupsPlan plan = groups_plan(spec.n_dst);
    GroupsShape S{spec.n_src, spec.n_dst, (spec.n_dst + 15u) / 16u, spec.n_src_groups, spec.n_dst_groups, 0, 0,
                  (uint32_t)P.chunks.size(), 0, 0};
    while ((1u << S.tile_shift) < plan.tile_words) S.tile_shift++;
    S.tiles = (S.row_words + plan.tile_words - 1u) / plan.tile_words;
    S.items = (uint64_t)spec.n_svc * S.n_chunks * S.tiles;
    std::vector<unsigned char> host;  // (before blk: a call that leaves early still outlives the copy out of it)
    Scratch blk;
    // the whole block is one host image and one copy; DGRP: the dst ids, u16 x 16 row_words
    enum { DGRP, CHUNKS, ROWS };
    const auto l =
        lay_out({P.dgrp.size() * sizeof(uint16_t), P.chunks.size() * sizeof(GroupsChunk), P.rows.size() * sizeof(uint32_t)});
    if (S.items) {
        host.assign(l.total, 0);
        l.put(host, DGRP, DGRP, P.dgrp), l.put(host, DGRP, CHUNKS, P.chunks), l.put(host, DGRP, ROWS, P.rows);
        if (Scratch::make(&blk, l.total, err) != 0) {
            (void)hipGetLastError();
            return -2;
        }
        HIPCHK(hipMemcpyAsync(blk.at<unsigned char>(0), host.data(), l.total, hipMemcpyHostToDevice, st));
        const size_t lds = (size_t)spec.n_dst_groups * 4u * sizeof(uint32_t);
        const Runs runs = run_grid(k_groups_count, (int)kGroupsBlock, lds, S.items, blocks_per_cu);
        S.per = runs.per;
        hipLaunchKernelGGL(k_groups_count, dim3((uint32_t)runs.groups), dim3(kGroupsBlock), lds, st, spec.matrix, S,
                           l.at<uint32_t>(blk, ROWS), l.at<GroupsChunk>(blk, CHUNKS), l.at<uint16_t>(blk, DGRP),
                           reinterpret_cast<unsigned long long*>(out_counts));
        HIPCHK(hipGetLastError());
    }
    if (out_packed) {
        const uint64_t n_words = (uint64_t)n_pair_rows * ((spec.n_dst_groups + 15u) / 16u);
        const uint32_t g = (uint32_t)std::min<uint64_t>((n_words + kGroupsBlock - 1) / kGroupsBlock, 4096);
        hipLaunchKernelGGL(k_groups_pack, dim3(g), dim3(kGroupsBlock), 0, st, out_counts, n_pair_rows, spec.n_dst_groups,
                           out_packed);
        HIPCHK(hipGetLastError());
    }
    // (the count kernel reads the block, and the copy into it reads `host`: Scratch)
    if (S.items) return blk.finish(st, "reach groups", err) != 0 ? -1 : 0;
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // namespace pg
