// Reachability classes (pg_reach_classes): the end points of a pg_reach_matrix result that the
// policy treats identically, written once for both sides like groups.hpp -- the gfx950 kernels
// (classes.hip) and the host twin (pg_debug_reach_classes_host, tests only) run the same per-word
// code, and both are driven by the one classes_resolve below, so they take the same rounds.
//
// Signatures are 64-bit sums that wrap, so their value does not depend on the order of the adds:
//   dst column j   h = sum over the rows r = v * n_src + i of code(r, j) * classes_row_key(r)
//   src row i      h = sum over the slices v and the words w of classes_src_term(masked word, w, v)
// Equal end points have equal signatures; the reverse is checked, never assumed: every member of a
// hash bucket is compared cell for cell with the bucket's leader (its least member), and those that
// differ go through another round under a new leader. Padding bits are masked, never trusted.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "diff.hpp"

namespace pg {

constexpr uint32_t kClassesMaxSide = 1u << 20, kClassesMaxSvc = 4096;
constexpr uint32_t kClassesBlock = 256, kClassesWave = 64;
// rows of one work item of the dst signatures: a lane ends an item with up to 16 u64 atomics, so the
// rows are many; an 8 x 4096 x 4096 matrix has 256 items
constexpr uint32_t kClassesChunkRows = 128;
// rows of one work item of the dst check: a lane ends an item with stores only where a column differed,
// so the items can be many (1024 for that matrix, four workgroups per CU)
constexpr uint32_t kClassesCheckRows = 32;
constexpr uint64_t kClassesGolden = 0x9E3779B97F4A7C15ull;

// splitmix64's finaliser
PG_HD uint64_t classes_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the multiplier of matrix row r in the dst signatures (odd: a single cell always moves the sum)
PG_HD uint64_t classes_row_key(uint64_t r) { return classes_mix((r + 1u) * kClassesGolden) | 1u; }

// a lane's 16 column sums
struct ClassesAcc {
    uint64_t h[16];
};
// one word of row r into them; x: the word masked with 3 * diff_valid
PG_HD void classes_dst_add(ClassesAcc& a, uint32_t x, uint64_t key) {
    PG_UNROLL
    for (uint32_t k = 0; k < 16; k++) a.h[k] += (uint64_t)((x >> (2u * k)) & 3u) * key;
}

// what word w of slice v adds to a src signature; x: the word masked with 3 * diff_valid
PG_HD uint64_t classes_src_term(uint32_t x, uint32_t w, uint32_t v) {
    return classes_mix(classes_mix((((uint64_t)v << 32) | w) + kClassesGolden) ^ x);
}

// The columns (bit k: column 16 w + k) of word x of one row that differ from their leaders' cells in
// that row. lead: the leader of each of the 16 columns, the column itself where there is nothing to
// check (a leader, a column already classed, padding); word(lw): word lw of the same row.
template <class WORD>
PG_HD uint32_t classes_dst_differs(uint32_t x, const uint32_t (&lead)[16], uint32_t w, WORD&& word) {
    uint32_t bad = 0;
    PG_UNROLL
    for (uint32_t k = 0; k < 16; k++) {
        const uint32_t l = lead[k];
        if (l != 16u * w + k) {
            const uint32_t y = word(l >> 4);
            bad |= ((((x >> (2u * k)) ^ (y >> (2u * (l & 15u)))) & 3u) ? 1u : 0u) << k;
        }
    }
    return bad;
}

// whether the 16 columns of word w have anything to check
PG_HD bool classes_dst_pending(const uint32_t (&lead)[16], uint32_t w) {
    bool any = false;
    PG_UNROLL
    for (uint32_t k = 0; k < 16; k++) any |= lead[k] != 16u * w + k;
    return any;
}

// A word of the quotient from row (v, src_rep[cs]) of the matrix: cell k is the row's cell rep[k], for
// the first n of the word's 16 cells, padding zero. Representatives that follow each other in one word
// of the row (always, where every end point is its own class) cost one load.
PG_HD uint32_t classes_quotient_word(const uint32_t* row, const uint32_t (&rep)[16], uint32_t n) {
    uint32_t out = 0, at = 0xFFFFFFFFu, y = 0;
    PG_UNROLL
    for (uint32_t k = 0; k < 16; k++) {
        if (k < n) {
            const uint32_t j = rep[k];
            if ((j >> 4) != at) at = j >> 4, y = row[at];
            out |= ((y >> (2u * (j & 15u))) & 3u) << (2u * k);
        }
    }
    return out;
}

// ---- the plan and the rounds (host only) ---------------------------------------------------------
// How the column kernels (the dst signatures and the dst check) cut the matrix: a work item is (chunk,
// column tile). A chunk is chunk_rows consecutive rows of the n_svc * n_src; a tile is tile_words
// column words, a power of two <= 256 that covers a narrow row at once, and the 256 / tile_words lane
// rows of a workgroup then take every 256 / tile_words-th row of the chunk. The one function the
// launch, the host twin and pg_debug_reach_classes_plan use.
struct ClassesPlan {
    uint32_t tile_words, chunk_rows, check_rows;  // chunk_rows: the signatures' chunk; check_rows: the check's
};
inline ClassesPlan classes_plan(uint32_t n_dst) {
    const uint32_t rw = (n_dst + 15u) / 16u;
    uint32_t t = 1;
    while (t < kClassesBlock && t < rw) t <<= 1;
    return ClassesPlan{t, kClassesChunkRows, kClassesCheckRows};
}

// the low `bits` bits of a signature ("classes_hash_bits": 64 keeps all, 0 makes every one equal)
inline uint64_t classes_keep(uint64_t h, uint32_t bits) { return bits >= 64u ? h : bits ? h & ((1ull << bits) - 1u) : 0u; }

struct ClassesSide {
    std::vector<uint32_t> cls, rep;  // the class of every end point; the least member of every class
    uint32_t rounds = 0;
};

// The classes of one side from its n signatures. Candidates: the end points of one signature are a
// bucket, and its least index is the bucket's leader. A round hands
//   check(pending, leader, differs)
// the members still to be compared (ascending) and every end point's leader, and gets differs[k] != 0
// for the pending[k] that is not equal to leader[pending[k]]; nonzero return: an error, passed on.
// The least member of a bucket that differed leads the others that differed into the next round. So
// every member is compared with every earlier leader of its bucket until it equals one: the classes
// are exact whatever the signatures are. rounds: 1 + the rounds in which a member differed, which is
// the most signatures (classes) any bucket holds. Ids by first appearance.
template <class CHECK>
int classes_resolve(const uint64_t* sig, uint32_t n, uint32_t hash_bits, CHECK&& check, ClassesSide* out) {
    constexpr uint32_t kNone = 0xFFFFFFFFu;
    out->cls.assign(n, 0), out->rep.clear(), out->rounds = 0;
    if (!n) return 0;
    std::vector<uint64_t> h(n);
    for (uint32_t i = 0; i < n; i++) h[i] = classes_keep(sig[i], hash_bits);
    // the first end point with a signature leads its bucket: an open-addressing table over the end
    // points in ascending order (what sorting (signature, index) gives, without the sort)
    std::vector<uint32_t> leader(n), pending, next(n, kNone);
    size_t cap = 16;
    while (cap < 2u * (size_t)n) cap <<= 1;
    std::vector<uint32_t> slot(cap, kNone);
    for (uint32_t i = 0; i < n; i++) {
        size_t at = (size_t)classes_mix(h[i] + kClassesGolden) & (cap - 1u);
        while (slot[at] != kNone && h[slot[at]] != h[i]) at = (at + 1u) & (cap - 1u);
        if (slot[at] == kNone) slot[at] = i;
        leader[i] = slot[at];
    }
    for (uint32_t i = 0; i < n; i++)
        if (leader[i] != i) pending.push_back(i);
    std::vector<uint8_t> differs;
    std::vector<uint32_t> again, keys;
    out->rounds = 1;
    while (!pending.empty()) {
        differs.assign(pending.size(), 0);
        if (int rc = check(pending, leader, differs)) return rc;
        again.clear(), keys.clear();
        for (size_t k = 0; k < pending.size(); k++) {
            if (!differs[k]) continue;
            const uint32_t m = pending[k], old = leader[m];
            if (next[old] == kNone) next[old] = m, keys.push_back(old);  // (ascending: the least that differed)
            again.push_back(m);
        }
        if (again.empty()) break;
        out->rounds++;
        pending.clear();
        for (uint32_t m : again) {
            leader[m] = next[leader[m]];  // (the old leaders are no members of `again`: they stay keys)
            if (leader[m] != m) pending.push_back(m);
        }
        for (uint32_t old : keys) next[old] = kNone;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (leader[i] == i) {
            out->cls[i] = (uint32_t)out->rep.size();
            out->rep.push_back(i);
        } else {
            out->cls[i] = out->cls[leader[i]];  // (a leader is its class's least member: already numbered)
        }
    }
    return 0;
}

// device.hpp-style API of classes.hip
struct ClassesSpecDev {
    const uint32_t* matrix;  // device
    uint32_t n_svc, n_src, n_dst;
    uint32_t hash_bits;  // "classes_hash_bits"
};
struct ClassesOutDev {  // device, each null or as include/policygpu.h says; a side is computed when its class is given
    uint32_t *src_class, *dst_class, *src_rep, *dst_rep, *quotient;
};
struct ClassesResult {  // pg_reach_classes_result
    uint32_t n_src_classes, n_dst_classes, rounds;
};
// 0, -1 (a HIP error) or -2 (the scratch allocation failed); synchronises the stream
int dev_reach_classes(uint32_t blocks_per_cu, const ClassesSpecDev& spec, const ClassesOutDev& out, ClassesResult* result,
                      void* stream, std::string* err);

}  // namespace pg
