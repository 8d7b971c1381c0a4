// gfx950 kernels of the reachability classes (pg_reach_classes; classes.hpp has the per-word code, the
// plan and the rounds).
//
//  k_classes_hash_dst   the work items (chunk, column tile) cut into one contiguous run per workgroup,
//                       the grid the resident workgroups. Per item a lane owns one column word and
//                       walks its rows of the chunk, adjacent lanes on adjacent words, eight loads in
//                       flight, the 16 column sums in registers (classes_dst_add). At the end of the
//                       item it adds them to the signatures, one u64 atomic per column that is not
//                       zero. The sums wrap, so the order of the adds does not show.
//  k_classes_hash_src   a wave per src end point: row i of every slice with coalesced loads, a term
//                       per word (classes_src_term), a wave sum, one store.
//  k_classes_check_src  a wave per (member, leader) pair: the two rows of every slice word for word,
//                       masked; one mark per pair, every mark written.
//  k_classes_check_dst  the items of k_classes_hash_dst. A lane holds the leaders of its 16 columns;
//                       per row it compares each cell with the leader's cell of the same row, read
//                       from the row it has just read a word of (L1 / L2). Words with nothing to check
//                       walk no row. A column that differed gets mark 1: every writer writes the same
//                       value, and the marks are cleared on the stream first.
//  k_classes_quotient   one lane per output word: its 16 cells gathered from the representatives' rows
//                       and columns (classes_quotient_word).
// No workgroup waits on another. The rounds (classes_resolve) run on the host between the launches:
// the signatures and the marks come back, the pairs and the leaders go in. The matrix stays here.
//
// No kernel reads a table or touches a hit counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "audit_launch.hpp"
#include "classes.hpp"

namespace pg {

namespace {

constexpr uint32_t kClassesLoads = 8;  // row loads a lane keeps in flight

struct ClassesShape {
    uint32_t n_rows, n_dst, row_words;  // n_rows = n_svc * n_src
    uint32_t tile_shift;                // tile_words = 1 << tile_shift
    uint32_t tiles, chunk_rows;
    uint64_t items, per;  // all work items; those of one workgroup
};

// the lane's place in item `it`: its column word, its first row and the end of the chunk
struct ClassesLane {
    uint32_t w, phases;
    uint64_t r, r1;  // (64 bits: r + 8 * phases may pass 2^32)
    bool on;
};
__device__ __forceinline__ ClassesLane classes_lane(const ClassesShape& S, uint64_t it) {
    const uint32_t tile_words = 1u << S.tile_shift;
    const uint32_t col = threadIdx.x & (tile_words - 1u), phase = threadIdx.x >> S.tile_shift;
    const uint32_t ch = (uint32_t)(it / S.tiles), tile = (uint32_t)(it - (uint64_t)ch * S.tiles);
    const uint64_t r0 = (uint64_t)ch * S.chunk_rows, r1 = r0 + S.chunk_rows < S.n_rows ? r0 + S.chunk_rows : S.n_rows;
    ClassesLane L;
    L.w = (tile << S.tile_shift) + col, L.r = r0 + phase, L.r1 = r1, L.phases = kClassesBlock >> S.tile_shift;
    L.on = L.w < S.row_words && L.r < L.r1;
    return L;
}

__global__ __launch_bounds__(kClassesBlock) void k_classes_hash_dst(const uint32_t* __restrict__ matrix, ClassesShape S,
                                                                    unsigned long long* __restrict__ sig) {
    const uint64_t it0 = (uint64_t)blockIdx.x * S.per, it1 = it0 + S.per < S.items ? it0 + S.per : S.items;
    for (uint64_t it = it0; it < it1; it++) {
        const ClassesLane L = classes_lane(S, it);
        if (!L.on) continue;
        const uint32_t mask = 3u * diff_valid(S.n_dst, L.w);
        const uint32_t* __restrict__ base = matrix + L.w;
        ClassesAcc a = {};
        uint64_t r = L.r;
        for (; r + (kClassesLoads - 1u) * L.phases < L.r1; r += kClassesLoads * L.phases) {
            uint32_t x[kClassesLoads];
#pragma unroll
            for (uint32_t u = 0; u < kClassesLoads; u++) x[u] = base[(r + u * L.phases) * S.row_words];
#pragma unroll
            for (uint32_t u = 0; u < kClassesLoads; u++) classes_dst_add(a, x[u] & mask, classes_row_key(r + u * L.phases));
        }
        for (; r < L.r1; r += L.phases) classes_dst_add(a, base[r * S.row_words] & mask, classes_row_key(r));
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            if (a.h[k]) atomicAdd(sig + 16u * (size_t)L.w + k, (unsigned long long)a.h[k]);  // (padding columns sum to 0)
    }
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t x) {
#pragma unroll
    for (int d = 32; d; d >>= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, d, 64);
    return x;
}

__global__ __launch_bounds__(kClassesBlock) void k_classes_hash_src(const uint32_t* __restrict__ matrix, uint32_t n_svc,
                                                                    uint32_t n_src, uint32_t n_dst, uint32_t row_words,
                                                                    unsigned long long* __restrict__ sig) {
    const uint32_t lane = threadIdx.x & (kClassesWave - 1u), waves = kClassesBlock / kClassesWave;
    for (uint64_t i = (uint64_t)blockIdx.x * waves + threadIdx.x / kClassesWave; i < n_src; i += (uint64_t)gridDim.x * waves) {
        uint64_t h = 0;
        for (uint32_t v = 0; v < n_svc; v++) {
            const uint32_t* __restrict__ row = matrix + ((uint64_t)v * n_src + i) * row_words;
            for (uint32_t w = lane; w < row_words; w += kClassesWave)
                h += classes_src_term(row[w] & 3u * diff_valid(n_dst, w), w, v);
        }
        h = wave_sum(h);
        if (lane == 0) sig[i] = h;
    }
}

__global__ __launch_bounds__(kClassesBlock) void k_classes_check_src(const uint32_t* __restrict__ matrix, uint32_t n_svc,
                                                                     uint32_t n_src, uint32_t n_dst, uint32_t row_words,
                                                                     const uint32_t* __restrict__ pairs, uint32_t n_pairs,
                                                                     uint32_t* __restrict__ marks) {
    const uint32_t lane = threadIdx.x & (kClassesWave - 1u), waves = kClassesBlock / kClassesWave;
    for (uint64_t p = (uint64_t)blockIdx.x * waves + threadIdx.x / kClassesWave; p < n_pairs; p += (uint64_t)gridDim.x * waves) {
        const uint32_t a = pairs[2u * p], b = pairs[2u * p + 1u];
        uint32_t bad = 0;
        for (uint32_t v = 0; v < n_svc; v++) {
            const uint32_t* __restrict__ ra = matrix + ((uint64_t)v * n_src + a) * row_words;
            const uint32_t* __restrict__ rb = matrix + ((uint64_t)v * n_src + b) * row_words;
            for (uint32_t w = lane; w < row_words; w += kClassesWave) bad |= (ra[w] ^ rb[w]) & 3u * diff_valid(n_dst, w);
        }
        const int any = __any(bad != 0);
        if (lane == 0) marks[p] = any ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kClassesBlock) void k_classes_check_dst(const uint32_t* __restrict__ matrix, ClassesShape S,
                                                                     const uint32_t* __restrict__ lead,
                                                                     uint32_t* __restrict__ marks) {
    const uint64_t it0 = (uint64_t)blockIdx.x * S.per, it1 = it0 + S.per < S.items ? it0 + S.per : S.items;
    for (uint64_t it = it0; it < it1; it++) {
        const ClassesLane L = classes_lane(S, it);
        if (!L.on) continue;
        const uint4* lp = reinterpret_cast<const uint4*>(lead + 16u * (size_t)L.w);  // (the scratch block is 16-B aligned)
        const uint4 l0 = lp[0], l1 = lp[1], l2 = lp[2], l3 = lp[3];
        const uint32_t ld[16] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w, l2.x, l2.y, l2.z, l2.w, l3.x, l3.y, l3.z, l3.w};
        if (!classes_dst_pending(ld, L.w)) continue;
        uint32_t bad = 0;
        for (uint64_t r = L.r; r < L.r1; r += L.phases) {
            const uint32_t* __restrict__ row = matrix + r * S.row_words;
            bad |= classes_dst_differs(row[L.w], ld, L.w, [&](uint32_t lw) { return row[lw]; });
        }
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
            if (bad >> k & 1u) marks[16u * (size_t)L.w + k] = 1u;
    }
}

__global__ __launch_bounds__(kClassesBlock) void k_classes_quotient(const uint32_t* __restrict__ matrix, uint32_t n_src,
                                                                    uint32_t row_words, const uint32_t* __restrict__ src_rep,
                                                                    uint32_t n_src_classes, const uint32_t* __restrict__ dst_rep,
                                                                    uint32_t n_dst_classes, uint64_t n_words,
                                                                    uint32_t* __restrict__ out) {
    const uint32_t rwq = (n_dst_classes + 15u) / 16u;
    for (uint64_t o = (uint64_t)blockIdx.x * kClassesBlock + threadIdx.x; o < n_words; o += (uint64_t)gridDim.x * kClassesBlock) {
        const uint64_t row = o / rwq;
        const uint32_t jw = (uint32_t)(o - row * rwq), v = (uint32_t)(row / n_src_classes);
        const uint32_t cs = (uint32_t)(row - (uint64_t)v * n_src_classes);
        // (the representatives' block is padded to whole words of 16 and 16-B aligned: four 16-B loads)
        const uint4* rp = reinterpret_cast<const uint4*>(dst_rep + 16u * (size_t)jw);
        const uint4 r0 = rp[0], r1 = rp[1], r2 = rp[2], r3 = rp[3];
        const uint32_t rep[16] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x, r3.y, r3.z, r3.w};
        const uint32_t left = n_dst_classes - 16u * jw;
        out[o] = classes_quotient_word(matrix + ((uint64_t)v * n_src + src_rep[cs]) * row_words, rep, left < 16u ? left : 16u);
    }
}

}  // namespace

int dev_reach_classes(uint32_t blocks_per_cu, const ClassesSpecDev& spec, const ClassesOutDev& out, ClassesResult* result,
                      void* stream, std::string* err) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_src = spec.n_src, n_dst = spec.n_dst, rw = (n_dst + 15u) / 16u, n_rows = spec.n_svc * n_src;
    const bool want_src = out.src_class != nullptr, want_dst = out.dst_class != nullptr;
    const ClassesPlan plan = classes_plan(n_dst);
    // S: the dst signatures' cut; C: the dst check's, the same tiles over shorter chunks
    ClassesShape S{n_rows, n_dst, rw, 0, 0, plan.chunk_rows, 0, 0};
    while ((1u << S.tile_shift) < plan.tile_words) S.tile_shift++;
    S.tiles = (rw + plan.tile_words - 1u) / plan.tile_words;
    S.items = (uint64_t)((n_rows + plan.chunk_rows - 1u) / plan.chunk_rows) * S.tiles;
    ClassesShape C = S;
    C.chunk_rows = plan.check_rows;
    C.items = (uint64_t)((n_rows + plan.check_rows - 1u) / plan.check_rows) * C.tiles;
    // (before blk: a call that leaves early still outlives the copies out of and into these)
    std::vector<uint64_t> sig(std::max(want_src ? n_src : 0u, want_dst ? 16u * rw : 0u));
    std::vector<uint32_t> aux, marks;
    ClassesSide src, dst;
    Scratch blk;
    // AUX: the src check's pairs or the dst check's leaders; SREP / DREP: the quotient's representatives or nothing
    enum { SIG, AUX, MARKS, SREP, DREP };
    const size_t n_aux = std::max<size_t>(want_src ? 2u * (size_t)n_src : 0u, want_dst ? 16u * (size_t)rw : 0u);
    const size_t n_marks = std::max<size_t>(want_src ? n_src : 0u, want_dst ? 16u * (size_t)rw : 0u);
    const auto l = lay_out({sig.size() * sizeof(uint64_t), n_aux * sizeof(uint32_t), n_marks * sizeof(uint32_t),
                            out.quotient ? n_src * sizeof(uint32_t) : 0u, out.quotient ? 16u * (size_t)rw * sizeof(uint32_t) : 0u});
    if (Scratch::make(&blk, l.total, err) != 0) {
        (void)hipGetLastError();
        return -2;
    }
    unsigned long long* d_sig = l.at<unsigned long long>(blk, SIG);
    uint32_t *d_aux = l.at<uint32_t>(blk, AUX), *d_marks = l.at<uint32_t>(blk, MARKS);
    uint32_t *d_srep = l.at<uint32_t>(blk, SREP), *d_drep = l.at<uint32_t>(blk, DREP);

    // the grid of a column kernel and the run of each of its workgroups
    auto column_grid = [&](auto kernel, ClassesShape& S) {
        const Runs runs = run_grid(kernel, (int)kClassesBlock, 0, S.items, blocks_per_cu);
        S.per = runs.per;
        return (uint32_t)runs.groups;
    };
    auto wave_grid = [&](auto kernel, uint64_t n) {
        const int grid = grid_resident(kernel, (int)kClassesBlock, 0, n * kClassesWave, blocks_per_cu);
        (void)hipGetLastError();
        return (uint32_t)grid;
    };

    if (want_src) {
        hipLaunchKernelGGL(k_classes_hash_src, dim3(wave_grid(k_classes_hash_src, n_src)), dim3(kClassesBlock), 0, st, spec.matrix,
                           spec.n_svc, n_src, n_dst, rw, d_sig);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(sig.data(), d_sig, n_src * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        auto check = [&](const std::vector<uint32_t>& pending, const std::vector<uint32_t>& leader, std::vector<uint8_t>& differs) {
            const uint32_t n = (uint32_t)pending.size();
            aux.resize(2u * (size_t)n), marks.resize(n);
            for (uint32_t k = 0; k < n; k++) aux[2u * k] = pending[k], aux[2u * k + 1u] = leader[pending[k]];
            HIPCHK(hipMemcpyAsync(d_aux, aux.data(), aux.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_classes_check_src, dim3(wave_grid(k_classes_check_src, n)), dim3(kClassesBlock), 0, st,
                               spec.matrix, spec.n_svc, n_src, n_dst, rw, d_aux, n, d_marks);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(marks.data(), d_marks, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (uint32_t k = 0; k < n; k++) differs[k] = marks[k] != 0;
            return 0;
        };
        if (classes_resolve(sig.data(), n_src, spec.hash_bits, check, &src) != 0) return -1;
    }
    if (want_dst) {
        HIPCHK(hipMemsetAsync(d_sig, 0, 16u * (size_t)rw * sizeof(uint64_t), st));
        hipLaunchKernelGGL(k_classes_hash_dst, dim3(column_grid(k_classes_hash_dst, S)), dim3(kClassesBlock), 0, st, spec.matrix, S,
                           d_sig);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(sig.data(), d_sig, n_dst * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        auto check = [&](const std::vector<uint32_t>& pending, const std::vector<uint32_t>& leader, std::vector<uint8_t>& differs) {
            aux.resize(16u * (size_t)rw), marks.resize(n_dst);
            for (uint32_t j = 0; j < 16u * rw; j++) aux[j] = j;
            for (uint32_t j : pending) aux[j] = leader[j];
            HIPCHK(hipMemcpyAsync(d_aux, aux.data(), aux.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemsetAsync(d_marks, 0, 16u * (size_t)rw * sizeof(uint32_t), st));
            const uint32_t grid = column_grid(k_classes_check_dst, C);
            hipLaunchKernelGGL(k_classes_check_dst, dim3(grid), dim3(kClassesBlock), 0, st, spec.matrix, C, d_aux, d_marks);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(marks.data(), d_marks, n_dst * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (size_t k = 0; k < pending.size(); k++) differs[k] = marks[pending[k]] != 0;
            return 0;
        };
        if (classes_resolve(sig.data(), n_dst, spec.hash_bits, check, &dst) != 0) return -1;
    }
    // ids and representatives out; the quotient from the representatives in the scratch block
    auto put = [&](uint32_t* to, const std::vector<uint32_t>& from) {
        if (to && !from.empty()) HIPCHK(hipMemcpyAsync(to, from.data(), from.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        return 0;
    };
    if (want_src && (put(out.src_class, src.cls) || put(out.src_rep, src.rep))) return -1;
    if (want_dst && (put(out.dst_class, dst.cls) || put(out.dst_rep, dst.rep))) return -1;
    if (out.quotient) {
        const uint32_t n_sc = (uint32_t)src.rep.size(), n_dc = (uint32_t)dst.rep.size();
        if (put(d_srep, src.rep) || put(d_drep, dst.rep)) return -1;
        const uint64_t n_words = (uint64_t)spec.n_svc * n_sc * ((n_dc + 15u) / 16u);
        const uint32_t g = (uint32_t)std::min<uint64_t>((n_words + kClassesBlock - 1) / kClassesBlock, 4096);
        hipLaunchKernelGGL(k_classes_quotient, dim3(g), dim3(kClassesBlock), 0, st, spec.matrix, n_src, rw, d_srep,
                           n_sc, d_drep, n_dc, n_words, out.quotient);
        HIPCHK(hipGetLastError());
    }
    *result = ClassesResult{(uint32_t)src.rep.size(), (uint32_t)dst.rep.size(), std::max(src.rounds, dst.rounds)};
    // (the kernels read the block, and the copies read the host vectors above: Scratch)
    return blk.finish(st, "reach classes", err) != 0 ? -1 : 0;
}

}  // namespace pg
