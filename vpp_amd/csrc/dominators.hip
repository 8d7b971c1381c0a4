// gfx950 kernels of the reachability dominators (pg_reach_dominators; dominators.hpp has the
// definitions, the per-word code and the plan).
//
// One scratch block: ET (n x closure_stride(n): bit p of ET[v] says p -> v), TE (per 16-row tile of ET
// the OR of its rows, static for the call), Avoid, D and D' (n x dom_stride(n): the sets, this
// round's increments and the next round's, swapped by the host), and two bit vectors over the end
// points, live and live' (is the row's D non-empty).
//  k_edges_t      edge_tiles.hpp, shared with cut.hip: the edge matrix of the selected slices, transposed
//                 through LDS ballots into ET, and the OR of every 16 rows of ET into TE.
//  k_dom_init     a workgroup per entry: its Avoid and D rows (dom_entry_word), its live bit and its
//                 entry flag; duplicates store the same values.
//  k_dom_round    one round. A workgroup of 16 waves owns 16 rows x 64 * LW bit-words of Avoid; wave w
//                 holds the accumulators of row w, a lane LW adjacent words. p goes in chunks of 32:
//                 the chunk's TE word & its live word (scalars) say which D rows any row of the tile
//                 needs; zero = the chunk is skipped by every wave, no barrier; with no chunk needed
//                 the workgroup ends having written nothing. The chunks are looked through 64 at a time,
//                 a lane per chunk and one ballot, so an idle tile costs n / 2048 loads per lane, not
//                 n / 32 dependent ones. Else those rows' segments are staged in LDS
//                 (two buffers: one barrier per staged chunk; fetched into registers one staged chunk
//                 ahead) and every wave walks its own word ET[v] & live, a scalar, bit by bit: one
//                 conflict-free ds_read of LW words per set bit, four in flight while the word has four
//                 bits left. Then the owner of each output word updates Avoid (dom_new), stores D', the
//                 row's live' bit (an atomic OR where the column tiles of a row meet), and the workgroup
//                 adds its popcount once. A D' row is read next round only where live' is set, and then
//                 every column tile of its row tile has run and stored it: a skipped tile may hold
//                 stale words that nobody reads.
//  k_dom_rows     a workgroup per row: |Dom(v)| to scratch and, when asked for, Dom(v) expanded to the
//                 audits' 2-bit layout.
//  k_dom_cut      tiles of 64 rows x 32 bit-words of Dom without its diagonal, one run per workgroup: read
//                 along the rows into LDS, then a ballot per column of a word and a popcount give the
//                 tile's column sums, added by integer atomics where the row tiles meet.
//  k_dom_idom     a wave per row: the set bits k of Dom(v) \ {v} with |Dom(k)| = |Dom(v)| - 1; at most
//                 one matches.
//  k_dom_result   one workgroup: the result words from the sizes, the cuts and the entry flags.
// One launch per round; the host reads the running total back after each and stops when it stands
// still. No kernel waits on another workgroup.
//
// No kernel reads a table or touches a hit counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "audit_launch.hpp"
#include "dominators.hpp"
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
__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
#pragma unroll
    for (int d = 32; d; d >>= 1) x = min(x, (uint32_t)__shfl_xor(x, d, 64));
    return x;
}
__device__ __forceinline__ uint64_t wave_max64(uint64_t x) {
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)x, d, 64);
        x = o > x ? o : x;
    }
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
template <uint32_t LW>
__device__ __forceinline__ void store_words(uint32_t* p, const uint32_t (&v)[LW]) {
    if constexpr (LW == 4) *reinterpret_cast<uint4*>(p) = make_uint4(v[0], v[1], v[2], v[3]);
    else if constexpr (LW == 2) *reinterpret_cast<uint2*>(p) = make_uint2(v[0], v[1]);
    else *p = v[0];
}

using DomTiles = EdgeTiles;  // all tiles; those of one workgroup

__global__ __launch_bounds__(kDomBlock) void k_dom_init(const uint32_t* __restrict__ entry, uint32_t n, uint32_t stride_a,
                                                        uint32_t* __restrict__ avoid, uint32_t* __restrict__ D,
                                                        uint32_t* __restrict__ live, uint32_t* __restrict__ is_entry) {
    const uint32_t e = __builtin_amdgcn_readfirstlane(entry[blockIdx.x]);
    if (e >= n) return;  // (checked on the host)
    for (uint32_t w = threadIdx.x; w < stride_a; w += kDomBlock) {
        const uint32_t x = dom_entry_word(n, e, w);
        avoid[e * stride_a + w] = x, D[e * stride_a + w] = x;
    }
    if (threadIdx.x == 0) {
        atomicOr(&live[e >> 5], 1u << (e & 31u));
        is_entry[e] = 1u;  // (every writer stores the same value)
    }
}

template <uint32_t LW>
__global__ __launch_bounds__(kDomRoundBlock) void k_dom_round(const uint32_t* __restrict__ ET, const uint32_t* __restrict__ TE,
                                                              const uint32_t* __restrict__ D, const uint32_t* __restrict__ live,
                                                              uint32_t* __restrict__ avoid, uint32_t* __restrict__ Dn,
                                                              uint32_t* __restrict__ live_n,
                                                              unsigned long long* __restrict__ total, uint32_t n,
                                                              uint32_t stride_e, uint32_t stride_a) {
    constexpr uint32_t kTileWords = 64u * LW;
    // two buffers of 32 D-row segments; after the p loop the first words hold the waves' sums
    __shared__ __attribute__((aligned(16))) uint32_t lds[2][32][kTileWords];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t my_w = blockIdx.x * kTileWords + lane * LW;  // this lane's first bit-word of a row
    const bool in = my_w < stride_a;                            // (stride_a is a multiple of 4: all LW words or none)
    const uint32_t v = blockIdx.y * kDomTileRows + wave;        // this wave's row
    const bool row = v < n;

    const uint32_t* __restrict__ t_row = TE + blockIdx.y * stride_e;
    const uint32_t chunks = closure_bit_words(n);
    // The chunks are looked through 64 at a time: lane k of every wave holds the live word and the needed
    // rows of chunk cg + k, one ballot says which chunks are needed at all, and a chunk's two words come
    // out of the lanes as scalars. (blockIdx and c only: `need` is the same scalar in every wave, so they
    // skip or stage together)
    uint32_t cg = 0, g_live = 0, g_need = 0;
    unsigned long long g_mask = 0;
    auto group = [&](uint32_t g0) {
        cg = g0;
        g_live = g0 + lane < chunks ? live[g0 + lane] : 0u;
        g_need = g_live ? t_row[g0 + lane] & g_live : 0u;
        g_mask = __ballot(g_need != 0u);
    };
    // the first needed chunk at or behind `from` (cg <= from <= cg + 64), or `chunks`
    auto find = [&](uint32_t from, uint32_t& at, uint32_t& nd, uint32_t& lw) {
        for (;;) {
            const uint32_t skip = from - cg;
            const unsigned long long m = skip < 64u ? (g_mask >> skip) << skip : 0ull;
            if (m) {
                const uint32_t k = (uint32_t)__builtin_ctzll(m);
                at = cg + k, nd = __builtin_amdgcn_readlane(g_need, k), lw = __builtin_amdgcn_readlane(g_live, k);
                return;
            }
            if (cg + 64u >= chunks) {
                at = chunks, nd = 0, lw = 0;
                return;
            }
            group(cg + 64u);
            from = cg;
        }
    };
    group(0);
    uint32_t c, need, lv;
    find(0, c, need, lv);
    if (c == chunks) return;  // no live row has an edge into this tile: nothing grows, nothing is written

    uint32_t acc[LW];
#pragma unroll
    for (uint32_t q = 0; q < LW; q++) acc[q] = 0;
    // wave w stages the needed rows among its kStage of the chunk's 32; they are fetched one staged chunk
    // ahead, so the loads fly while the chunk before is walked
    constexpr uint32_t kStage = 32u / kDomWaves;
    uint32_t pre[kStage][LW];
    auto fetch = [&](uint32_t cc, uint32_t nd) {
        const uint32_t mine = nd >> (kStage * wave);
#pragma unroll
        for (uint32_t j = 0; j < kStage; j++)
            if ((mine >> j & 1u) && in) load_words<LW>(D + (32u * cc + kStage * wave + j) * stride_a + my_w, pre[j]);
    };
    fetch(c, need);
    uint32_t buf = 0;
    while (c < chunks) {
        const uint32_t mine = need >> (kStage * wave);
#pragma unroll
        for (uint32_t j = 0; j < kStage; j++)
            if ((mine >> j & 1u) && in) store_words<LW>(&lds[buf][kStage * wave + j][lane * LW], pre[j]);
        uint32_t cn, need_n, lv_n;
        find(c + 1u, cn, need_n, lv_n);
        if (cn < chunks) fetch(cn, need_n);
        __syncthreads();
        if (row) {  // (uniform in the wave; a lane outside the row reads LDS words nobody uses)
            // the word of (row, chunk) restricted to the live rows: wave-uniform, walked on the scalar side;
            // four reads in flight while it has four bits left
            uint32_t f = __builtin_amdgcn_readfirstlane(ET[v * stride_e + c]) & lv;
            while (__builtin_popcount(f) >= 4) {
                uint32_t x[4][LW];
#pragma unroll
                for (uint32_t u = 0; u < 4; u++) {
                    load_words<LW>(&lds[buf][__builtin_ctz(f)][lane * LW], x[u]);
                    f &= f - 1u;
                }
#pragma unroll
                for (uint32_t q = 0; q < LW; q++) acc[q] |= (x[0][q] | x[1][q]) | (x[2][q] | x[3][q]);
            }
            for (; f; f &= f - 1u) {
                uint32_t x[LW];
                load_words<LW>(&lds[buf][__builtin_ctz(f)][lane * LW], x);
#pragma unroll
                for (uint32_t q = 0; q < LW; q++) acc[q] |= x[q];
            }
        }
        buf ^= 1u;  // (the next staging writes the other buffer: a wave still reading this one is safe)
        c = cn, need = need_n, lv = lv_n;
    }

    uint32_t cnt = 0;
    if (row) {  // (uniform in the wave)
        uint32_t any_new = 0;
        if (in) {
            uint32_t nw[LW], any_acc = 0;
#pragma unroll
            for (uint32_t q = 0; q < LW; q++) nw[q] = 0, any_acc |= acc[q];
            uint32_t* ap = avoid + v * stride_a + my_w;
            if (any_acc) {
                uint32_t have[LW];
                load_words<LW>(ap, have);
#pragma unroll
                for (uint32_t q = 0; q < LW; q++) {
                    nw[q] = dom_new(acc[q], have[q], v, my_w + q);
                    have[q] |= nw[q];
                    any_new |= nw[q];
                    cnt += (uint32_t)__builtin_popcount(nw[q]);
                }
                if (any_new) store_words<LW>(ap, have);  // (this lane owns these words: no atomics)
            }
            store_words<LW>(Dn + v * stride_a + my_w, nw);
        }
        if (__any(any_new != 0) && lane == 0) atomicOr(&live_n[v >> 5], 1u << (v & 31u));
    }

    // the workgroup's popcount, through the staging buffer
    __syncthreads();  // (every wave has left the p loop)
    uint32_t* sh_c = &lds[0][0][0];  // [waves]
    const uint32_t ws = wave_sum(cnt);
    if (lane == 0) sh_c[wave] = ws;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t s = 0;
#pragma unroll
        for (uint32_t k = 0; k < kDomWaves; k++) s += sh_c[k];
        if (s) atomicAdd(total, (unsigned long long)s);
    }
}

template <bool PACK>
__global__ __launch_bounds__(kDomBlock) void k_dom_rows(const uint32_t* __restrict__ avoid, uint32_t n, uint32_t stride_a,
                                                        uint32_t* __restrict__ size, uint32_t* __restrict__ out_dom) {
    __shared__ uint32_t sh[kDomBlockWaves];
    const uint32_t v = blockIdx.x, rw = (n + 15u) / 16u;
    const uint32_t* __restrict__ row = avoid + v * stride_a;
    const bool reached = dom_reached(row, n);  // (the same in every lane)
    uint32_t cnt = 0;
    for (uint32_t jw = threadIdx.x; jw < rw; jw += kDomBlock) {
        const uint32_t w = jw >> 1;
        const uint32_t h = (dom_word(row[w], reached, n, w) >> (16u * (jw & 1u))) & 0xFFFFu;
        if constexpr (PACK) out_dom[v * rw + jw] = closure_expand(h);
        cnt += (uint32_t)__builtin_popcount(h);
    }
    const uint32_t ws = wave_sum(cnt);
    if ((threadIdx.x & 63u) == 0) sh[threadIdx.x >> 6] = ws;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t k = 0; k < kDomBlockWaves; k++) s += sh[k];
        size[v] = s;
    }
}

__global__ __launch_bounds__(kDomBlock) void k_dom_cut(const uint32_t* __restrict__ avoid, uint32_t n, uint32_t stride_a,
                                                       DomTiles S, uint32_t* __restrict__ cut) {
    __shared__ uint32_t sh[kDomCutRows][kDomCutPitch];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t wl = threadIdx.x % kDomCutWords, ph = threadIdx.x / kDomCutWords;
    const uint32_t bw = closure_bit_words(n);
    const uint32_t it0 = blockIdx.x * S.per, it1 = min(it0 + S.per, S.items);
    for (uint32_t it = it0; it < it1; it++) {
        const uint32_t tr = it / S.col_tiles, tc = it - tr * S.col_tiles;
        const uint32_t r0 = tr * kDomCutRows, w0 = tc * kDomCutWords;
        __syncthreads();  // (every wave has left the tile before)
        const uint32_t w = w0 + wl;
        for (uint32_t r = ph; r < kDomCutRows; r += kDomBlock / kDomCutWords) {
            const uint32_t i = r0 + r;
            uint32_t x = 0;
            if (i < n && w < bw) {
                const uint32_t* __restrict__ row = avoid + i * stride_a;
                x = dom_word(row[w], dom_reached(row, n), n, w) & ~dom_self(i, w);
            }
            sh[r][wl] = x;
        }
        __syncthreads();
        for (uint32_t q = wave; q < kDomCutWords; q += kDomBlockWaves) {
            const uint32_t x = sh[lane][q];
            if (!__any(x != 0u)) continue;  // (the same in every lane)
            uint32_t cnt = 0;
#pragma unroll
            for (uint32_t k = 0; k < 32; k++) {
                const unsigned long long b = __ballot(dom_ballot_bit(x, k));
                if (lane == k) cnt = (uint32_t)__popcll(b);
            }
            // (a column at or past n has no cell: its count is zero)
            if (cnt) atomicAdd(&cut[32u * (w0 + q) + lane], cnt);
        }
    }
}

__global__ __launch_bounds__(kDomBlock) void k_dom_idom(const uint32_t* __restrict__ avoid, const uint32_t* __restrict__ size,
                                                        uint32_t n, uint32_t stride_a, uint16_t* __restrict__ out_idom) {
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t bw = closure_bit_words(n);
    for (uint32_t v = blockIdx.x * kDomBlockWaves + wave; v < n; v += gridDim.x * kDomBlockWaves) {
        const uint32_t sv = size[v];
        uint32_t found = kDomNoIdom;
        if (sv > 1u) {  // (reached, and some k != v dominates it)
            const uint32_t* __restrict__ row = avoid + v * stride_a;
            for (uint32_t w = lane; w < bw; w += 64u)
                for (uint32_t d = dom_word(row[w], true, n, w) & ~dom_self(v, w); d; d &= d - 1u) {
                    const uint32_t k = 32u * w + (uint32_t)__builtin_ctz(d);
                    if (dom_is_idom(size[k], sv)) found = min(found, k);
                }
        }
        found = wave_min(found);
        if (lane == 0) out_idom[v] = (uint16_t)found;
    }
}

__global__ __launch_bounds__(kDomResultBlock) void k_dom_result(const uint32_t* __restrict__ size, const uint32_t* __restrict__ cut,
                                                                const uint32_t* __restrict__ is_entry, uint32_t n,
                                                                uint32_t* __restrict__ result) {
    constexpr uint32_t kWaves = kDomResultBlock / 64;
    __shared__ uint32_t sh_red[3][kWaves];
    __shared__ uint64_t sh_key[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t reached = 0, chokes = 0, largest = 0;
    uint64_t key = 0;
    for (uint32_t v = threadIdx.x; v < n; v += kDomResultBlock) {
        const uint32_t s = size[v], c = cut[v];
        reached += s != 0u, largest = max(largest, s);
        if (c && !is_entry[v]) {
            chokes++;
            const uint64_t k = dom_top_key(c, v);
            key = k > key ? k : key;
        }
    }
    reached = wave_sum(reached), chokes = wave_sum(chokes), largest = wave_max(largest), key = wave_max64(key);
    if (lane == 0) sh_red[0][wave] = reached, sh_red[1][wave] = chokes, sh_red[2][wave] = largest, sh_key[wave] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t r = 0, c = 0, l = 0;
        uint64_t k = 0;
        for (uint32_t w = 0; w < kWaves; w++) r += sh_red[0][w], c += sh_red[1][w], l = max(l, sh_red[2][w]), k = sh_key[w] > k ? sh_key[w] : k;
        result[0] = r, result[1] = c, result[2] = dom_top_of(k), result[3] = (uint32_t)(k >> 32), result[4] = l ? l - 1u : 0u;
    }
}

struct RoundArgs {
    const uint32_t *ET, *TE, *D, *live;
    uint32_t *avoid, *Dn, *live_n;
    unsigned long long* total;
    uint32_t n, stride_e, stride_a;
};
template <uint32_t LW>
void launch_round(const DomPlan& p, hipStream_t st, const RoundArgs& a) {
    hipLaunchKernelGGL((k_dom_round<LW>), dim3(p.col_tiles, p.row_tiles), dim3(kDomRoundBlock), 0, st, a.ET, a.TE, a.D, a.live,
                       a.avoid, a.Dn, a.live_n, a.total, a.n, a.stride_e, a.stride_a);
}

}  // namespace

int dev_reach_dominators(uint32_t blocks_per_cu, const DomSpecDev& spec, uint32_t* out_dom, uint16_t* out_idom,
                         uint32_t* out_cut, DomResult* res, void* stream, std::string* err) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n = spec.n, stride_e = closure_stride(n), stride_a = dom_stride(n), rw = (n + 15u) / 16u;
    const DomPlan p = dom_plan(n);
    // (before blk: a call that leaves early still outlives the copies out of it)
    uint32_t words[kDomResultWords] = {};
    uint64_t now = 0;
    std::vector<unsigned char> h;  // the host image of LIST and ENTRY
    Scratch blk;
    // TOTAL: the running popcount, a u64 cleared as 16 B. LIVE .. CUT are adjacent: one memset clears
    // them. DN / LIVE_N: the next round's D / live. LIST and ENTRY are adjacent: one copy fills them.
    enum { TOTAL, MAT_ET, TILE_TE, AVOID, MAT_D, MAT_DN, LIVE, LIVE_N, IS_ENTRY, CUT, SIZE, RESULT, LIST, ENTRY, END };
    const size_t mat_e = (size_t)n * stride_e * sizeof(uint32_t), tiles = (size_t)p.row_tiles * stride_e * sizeof(uint32_t);
    const size_t mat_a = (size_t)n * stride_a * sizeof(uint32_t), vec = (size_t)n * sizeof(uint32_t);
    const size_t flags = (size_t)stride_e * sizeof(uint32_t);  // (a bit per end point, cleared whole)
    const auto l = lay_out({16, mat_e, tiles, mat_a, mat_a, mat_a, flags, flags, vec, vec, vec, kDomResultWords * sizeof(uint32_t),
                            spec.n_list * sizeof(uint32_t), spec.n_entry * sizeof(uint32_t), 0});
    if (Scratch::make(&blk, l.total, err) != 0) {
        (void)hipGetLastError();
        return -2;
    }
    unsigned long long* total = l.at<unsigned long long>(blk, TOTAL);
    uint32_t *ET = l.at<uint32_t>(blk, MAT_ET), *TE = l.at<uint32_t>(blk, TILE_TE), *avoid = l.at<uint32_t>(blk, AVOID);
    uint32_t *D = l.at<uint32_t>(blk, MAT_D), *Dn = l.at<uint32_t>(blk, MAT_DN), *live = l.at<uint32_t>(blk, LIVE),
             *live_n = l.at<uint32_t>(blk, LIVE_N), *is_entry = l.at<uint32_t>(blk, IS_ENTRY), *size = l.at<uint32_t>(blk, SIZE),
             *d_res = l.at<uint32_t>(blk, RESULT), *list = l.at<uint32_t>(blk, LIST), *entry = l.at<uint32_t>(blk, ENTRY);
    uint32_t* cut = out_cut ? out_cut : l.at<uint32_t>(blk, CUT);
    h.resize(l.off[END] - l.off[LIST]);
    l.put(h, LIST, LIST, spec.svc_list, spec.n_list);
    l.put(h, LIST, ENTRY, spec.entry, spec.n_entry);
    HIPCHK(hipMemsetAsync(total, 0, 16, st));
    HIPCHK(hipMemsetAsync(avoid, 0, mat_a, st));
    HIPCHK(hipMemsetAsync(live, 0, l.off[SIZE] - l.off[LIVE], st));
    if (out_cut) HIPCHK(hipMemsetAsync(out_cut, 0, vec, st));
    if (!h.empty()) HIPCHK(hipMemcpyAsync(list, h.data(), h.size(), hipMemcpyHostToDevice, st));

    DomTiles S{p.t_col_tiles, p.t_grid, 0};
    Runs runs = run_grid(k_edges_t<false, true>, (int)kDomBlock, 0, S.items, blocks_per_cu);
    S.per = (uint32_t)runs.per;
    hipLaunchKernelGGL((k_edges_t<false, true>), dim3((uint32_t)runs.groups), dim3(kDomBlock), 0, st, spec.matrix, list, spec.n_list,
                       n, rw, stride_e, S, (uint32_t*)nullptr, ET, TE);
    HIPCHK(hipGetLastError());
    if (spec.n_entry) {
        hipLaunchKernelGGL(k_dom_init, dim3(spec.n_entry), dim3(kDomBlock), 0, st, entry, n, stride_a, avoid, D, live, is_entry);
        HIPCHK(hipGetLastError());
    }
    // (the copies above read `h`: they are done before it goes, whatever ends the call)
    HIPCHK(hipStreamSynchronize(st));

    // (a round that grows adds a bit to a set and there are n (n + 1) bits: the loop ends by itself)
    uint32_t rounds = 0;
    for (uint64_t grown = 0; spec.n_entry;) {
        HIPCHK(hipMemsetAsync(live_n, 0, flags, st));
        const RoundArgs a{ET, TE, D, live, avoid, Dn, live_n, total, n, stride_e, stride_a};
        if (p.lane_words == 1) launch_round<1>(p, st, a);
        else if (p.lane_words == 2) launch_round<2>(p, st, a);
        else launch_round<4>(p, st, a);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&now, total, sizeof now, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (now == grown) break;
        grown = now, rounds++;
        std::swap(D, Dn), std::swap(live, live_n);
    }

    if (out_dom) hipLaunchKernelGGL(k_dom_rows<true>, dim3(p.finish_grid), dim3(kDomBlock), 0, st, avoid, n, stride_a, size, out_dom);
    else hipLaunchKernelGGL(k_dom_rows<false>, dim3(p.finish_grid), dim3(kDomBlock), 0, st, avoid, n, stride_a, size, out_dom);
    HIPCHK(hipGetLastError());
    S = DomTiles{p.cut_col_tiles, p.cut_grid, 0};
    runs = run_grid(k_dom_cut, (int)kDomBlock, 0, S.items, blocks_per_cu);
    S.per = (uint32_t)runs.per;
    hipLaunchKernelGGL(k_dom_cut, dim3((uint32_t)runs.groups), dim3(kDomBlock), 0, st, avoid, n, stride_a, S, cut);
    HIPCHK(hipGetLastError());
    if (out_idom) {
        const uint32_t items = (p.finish_grid + kDomBlockWaves - 1u) / kDomBlockWaves;
        const int g = grid_resident(k_dom_idom, (int)kDomBlock, 0, (uint64_t)items * kDomBlock, blocks_per_cu);
        (void)hipGetLastError();
        hipLaunchKernelGGL(k_dom_idom, dim3(g), dim3(kDomBlock), 0, st, avoid, size, n, stride_a, out_idom);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_dom_result, dim3(1), dim3(kDomResultBlock), 0, st, size, cut, is_entry, n, d_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(words, d_res, sizeof(words), hipMemcpyDeviceToHost, st));
    if (blk.finish(st, "reach dominators", err) != 0) return -1;
    *res = DomResult{words[0], words[1], words[2], words[3], words[4], rounds};
    return 0;
}

}  // namespace pg
