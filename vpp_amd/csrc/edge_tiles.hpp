// The edge / transpose tiles that dominators.hip, cut.hip and cost.hip share: one kernel that makes the bit-word
// edge matrix of a square pg_reach_matrix result (dominators.hpp dom_edge_word) and leaves it
// transposed, and on request as it is and as the OR of every 16 transposed rows. HIP only.
//
//  k_edges_t  the tiles (128 rows x 32 bit-words of the edge matrix) cut into one contiguous run per
//             workgroup, the grid the resident workgroups. A lane makes one bit-word from the selected
//             slices (dom_edge_word; the slice list is read through scalar loads) into LDS, and with
//             WITH_A (cut.hip, cost.hip) stores it to A as well; then a wave takes two bit-word columns of the tile at a
//             time: its lanes read one word of 64 consecutive rows each from LDS (pitch 33: no bank
//             conflict), one wave-wide ballot per column gives 64 rows of that column, and lane k keeps
//             the ballots of its column for both halves of the tile: four adjacent ET words, one
//             aligned 16-B store. With WITH_TE an OR over each 16 lanes (four shuffles) gives the same
//             four words of TE. Every word of A, ET and TE is written, padding zero. No lane reads
//             down a column.
#pragma once
#include <hip/hip_runtime.h>

#include "dominators.hpp"

namespace pg {

struct EdgeTiles {
    uint32_t col_tiles, items, per;  // all tiles; those of one workgroup
};

template <bool WITH_A, bool WITH_TE>
__global__ __launch_bounds__(kDomBlock) void k_edges_t(const uint32_t* __restrict__ matrix, const uint32_t* __restrict__ svc_list,
                                                       uint32_t n_list, uint32_t n, uint32_t rw, uint32_t stride, EdgeTiles S,
                                                       uint32_t* __restrict__ A, uint32_t* __restrict__ ET,
                                                       uint32_t* __restrict__ TE) {
    __shared__ uint32_t sh[kDomTRows][kDomTPitch];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t wl = threadIdx.x % kDomTWords, ph = threadIdx.x / kDomTWords;
    const uint32_t it0 = blockIdx.x * S.per, it1 = min(it0 + S.per, S.items);
    for (uint32_t it = it0; it < it1; it++) {
        const uint32_t tr = it / S.col_tiles, tc = it - tr * S.col_tiles;
        const uint32_t r0 = tr * kDomTRows, w0 = tc * kDomTWords;
        __syncthreads();  // (every wave has left the tile before)
        const uint32_t w = w0 + wl;
        for (uint32_t r = ph; r < kDomTRows; r += kDomBlock / kDomTWords) {
            const uint32_t i = r0 + r;
            const bool in = i < n && w < stride;
            const uint32_t x = in ? dom_edge_word(matrix, svc_list, n_list, n, rw, i, w) : 0u;
            sh[r][wl] = x;
            if constexpr (WITH_A)
                if (in) A[(size_t)i * stride + w] = x;
        }
        __syncthreads();
        // words q and q + 1 of the tile: lanes 0..31 end with the columns of q, lanes 32..63 with those of q + 1
        for (uint32_t q = 2u * wave; q < kDomTWords; q += 2u * kDomBlockWaves) {
            uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
#pragma unroll
            for (uint32_t s = 0; s < 2; s++) {
                const uint32_t x0 = sh[lane][q + s], x1 = sh[64u + lane][q + s];
#pragma unroll
                for (uint32_t k = 0; k < 32; k++) {
                    const unsigned long long b0 = __ballot(dom_ballot_bit(x0, k)), b1 = __ballot(dom_ballot_bit(x1, k));
                    if (lane == 32u * s + k) v0 = (uint32_t)b0, v1 = (uint32_t)(b0 >> 32), v2 = (uint32_t)b1, v3 = (uint32_t)(b1 >> 32);
                }
            }
            // (a column at or past n has no cell: its words are zero. stride is a multiple of 4 and the tile's
            // rows are words 4 tr .. 4 tr + 3 of an ET row: inside it, 16-B aligned)
            const uint32_t c = 32u * (w0 + q) + lane;
            if (c < n) *reinterpret_cast<uint4*>(ET + (size_t)c * stride + 4u * tr) = make_uint4(v0, v1, v2, v3);
            if constexpr (WITH_TE) {
                // the OR of 16 adjacent ET rows: the tile word of the rounds
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    v0 |= (uint32_t)__shfl_xor((int)v0, d, 64), v1 |= (uint32_t)__shfl_xor((int)v1, d, 64);
                    v2 |= (uint32_t)__shfl_xor((int)v2, d, 64), v3 |= (uint32_t)__shfl_xor((int)v3, d, 64);
                }
                if ((lane & 15u) == 0 && c < n) *reinterpret_cast<uint4*>(TE + (c >> 4) * stride + 4u * tr) = make_uint4(v0, v1, v2, v3);
            }
        }
    }
}

}  // namespace pg
