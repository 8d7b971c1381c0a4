// Reachability groups (pg_reach_groups): a pg_reach_matrix result summed into (src group, dst
// group) pairs, written once for both sides like diff.hpp -- the gfx950 kernels (groups.hip) and
// the host twin (pg_debug_reach_groups_host, tests only) run the same add, extract, flush and
// status functions.
//
// Vertical counters: a lane owns one column word (16 dst) and walks rows of one src group. Of the
// masks diff_eq gives (one bit per cell, at the even positions) it adds those of the codes 1, 2 and
// 3 into 8-bit fields: f[c - 1][q] += (m[c] >> 2q) & 0x01010101, so byte b of f[c - 1][q] counts
// column q + 4b. Code 0 is what is left of the rows walked. A field holds 255: at most
// kGroupsChunkRows rows go between two flushes. A flush hands the lane's 16 x 4 counts to an `add(dst
// group, code, count)`, columns of one group that follow each other summed first; skipped and
// padding columns (group kGroupsSkip16 in the lane's 16 ids) add nothing. Padding bits of the input
// are masked, never trusted.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "diff.hpp"

namespace pg {

constexpr uint32_t kGroupsSkip = 0xFFFFFFFFu;  // PG_GROUP_SKIP
constexpr uint32_t kGroupsSkip16 = 0xFFFFu;    // the same in the 16-bit ids the kernels read
constexpr uint32_t kGroupsMaxGroups = 4096, kGroupsMaxSide = 1u << 20, kGroupsMaxSvc = 4096;
constexpr uint32_t kGroupsBlock = 256;
// rows between two flushes (<= 255, what a field holds). 64 and not 255: at the audits' sizes the
// work items are few (an 8 x 4096 x 4096 matrix has 512 chunks of 64 rows), and a flush costs a
// lane at most 64 LDS adds, one per row walked
constexpr uint32_t kGroupsChunkRows = 64;
// a workgroup's LDS accumulators are u32: one work item adds at most 255 rows x 4096 columns to a
// cell, so they go to out_counts after at most this many items of one (service, src group)
constexpr uint32_t kGroupsRunItems = 4000;

struct GroupsAcc {
    uint32_t f[3][4];
};

// one word of a row into the lane's counters; valid: diff_valid of the word
PG_HD void groups_add(GroupsAcc& a, uint32_t x, uint32_t valid) {
    const DiffEq e = diff_eq(x & 3u * valid);
    PG_UNROLL
    for (uint32_t c = 1; c < 4; c++) {
        PG_UNROLL
        for (uint32_t q = 0; q < 4; q++) a.f[c - 1][q] += (e.m[c] >> (2u * q)) & 0x01010101u;
    }
}

// the four counts of column k (0..15) of the lane's word after `rows` rows
PG_HD void groups_extract(const GroupsAcc& a, uint32_t k, uint32_t rows, uint32_t (&cnt)[4]) {
    cnt[0] = rows;
    PG_UNROLL
    for (uint32_t c = 1; c < 4; c++) {
        cnt[c] = (a.f[c - 1][k & 3u] >> (8u * (k >> 2))) & 0xFFu;
        cnt[0] -= cnt[c];
    }
}

// The lane's counts after `rows` rows to add(dst group, code, count > 0). gw: the 16-bit group ids
// of the word's 16 columns, two per word, kGroupsSkip16 for a skipped or padding column.
template <class ADD>
PG_HD void groups_flush(const GroupsAcc& a, uint32_t rows, const uint32_t (&gw)[8], ADD&& add) {
    uint32_t run = kGroupsSkip16, sum[4] = {0, 0, 0, 0};
    auto emit = [&]() {
        if (run == kGroupsSkip16) return;
        PG_UNROLL
        for (uint32_t c = 0; c < 4; c++)
            if (sum[c]) add(run, c, sum[c]);
    };
    PG_UNROLL
    for (uint32_t k = 0; k < 16; k++) {
        const uint32_t g = (gw[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
        if (g != run) {
            emit();
            run = g, sum[0] = sum[1] = sum[2] = sum[3] = 0;
        }
        uint32_t cnt[4];
        groups_extract(a, k, rows, cnt);
        PG_UNROLL
        for (uint32_t c = 0; c < 4; c++) sum[c] += cnt[c];
    }
    emit();
}

// PG_GROUPS_* of a pair from its four counts
PG_HD uint32_t groups_status(const uint64_t* c) {
    const uint64_t cells = c[0] + c[1] + c[2] + c[3];
    return !cells ? 3u : c[2] == cells ? 2u : c[2] ? 1u : 0u;
}

// word jw of a status row: pairs (gs, 16 jw ..) of one (service, src group), whose counts start at
// `counts` (n_dst_groups x 4); padding zero
PG_HD uint32_t groups_pack_word(const uint64_t* counts, uint32_t n_dst_groups, uint32_t jw) {
    uint32_t w = 0;
    for (uint32_t k = 0; k < 16u && 16u * jw + k < n_dst_groups; k++)
        w |= groups_status(counts + 4u * (16u * jw + k)) << (2u * k);
    return w;
}

// ---- the partition (host only) -------------------------------------------------------------------
// How a launch cuts the matrix: a work item is (service, chunk, column tile). A chunk is at most
// chunk_rows rows of one src group; a tile is tile_words column words, a power of two <= 256 that
// covers a narrow row at once, and the 256 / tile_words lane rows of a workgroup then take every
// 256 / tile_words-th row of the chunk. The one function the launch, the host twin and
// pg_debug_reach_groups_plan use.
struct GroupsPlan {
    uint32_t tile_words, chunk_rows;
};
inline GroupsPlan groups_plan(uint32_t n_dst) {
    const uint32_t rw = (n_dst + 15u) / 16u;
    uint32_t t = 1;
    while (t < kGroupsBlock && t < rw) t <<= 1;
    return GroupsPlan{t, kGroupsChunkRows};
}

struct GroupsChunk {
    uint32_t gs, r0, r1;  // rows[r0 .. r1) of src group gs
};
// rows: the src indices that belong to a group, sorted by group (a stable counting sort); chunks: in
// (group, row) order; dgrp: the dst ids in 16 bits, 16 per column word, the padding kGroupsSkip16
struct GroupsPartition {
    std::vector<uint32_t> rows;
    std::vector<GroupsChunk> chunks;
    std::vector<uint16_t> dgrp;
};
inline GroupsPartition groups_partition(const uint32_t* src_group, uint32_t n_src, uint32_t n_src_groups,
                                        const uint32_t* dst_group, uint32_t n_dst, uint32_t chunk_rows) {
    GroupsPartition p;
    std::vector<uint32_t> start(n_src_groups + 1, 0);
    for (uint32_t i = 0; i < n_src; i++)
        if (src_group[i] != kGroupsSkip) start[src_group[i] + 1]++;
    for (uint32_t g = 0; g < n_src_groups; g++) start[g + 1] += start[g];
    p.rows.resize(start[n_src_groups]);
    std::vector<uint32_t> at(start.begin(), start.end() - 1);
    for (uint32_t i = 0; i < n_src; i++)
        if (src_group[i] != kGroupsSkip) p.rows[at[src_group[i]]++] = i;
    for (uint32_t g = 0; g < n_src_groups; g++)
        for (uint32_t r = start[g]; r < start[g + 1]; r += chunk_rows)
            p.chunks.push_back(GroupsChunk{g, r, r + chunk_rows < start[g + 1] ? r + chunk_rows : start[g + 1]});
    p.dgrp.assign(16u * ((n_dst + 15u) / 16u), (uint16_t)kGroupsSkip16);
    for (uint32_t j = 0; j < n_dst; j++)
        if (dst_group[j] != kGroupsSkip) p.dgrp[j] = (uint16_t)dst_group[j];
    return p;
}

// device.hpp-style API of groups.hip
struct GroupsSpecDev {
    const uint32_t* matrix;  // device
    uint32_t n_svc, n_src, n_dst, n_src_groups, n_dst_groups;
    const GroupsPartition* part;  // host
};
// out_counts device, out_packed device or null. 0, -1 (a HIP error) or -2 (the scratch allocation
// failed); synchronises the stream
int dev_reach_groups(uint32_t blocks_per_cu, const GroupsSpecDev& spec, uint64_t* out_counts, uint32_t* out_packed,
                     void* stream, std::string* err);

}  // namespace pg
