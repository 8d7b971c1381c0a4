// Rule coverage (pg_reach_rules): per-rule histograms of a reach product, without the product.
// Written once for both sides like reach.hpp -- the gfx950 kernel (reach.hip k_rules_pairs) and the
// host twin (pg_debug_reach_rules_host, tests only) instantiate the same per-word code, sink and
// plan.
//
// The product, its end points, the form A / form B partition of the services and the hoisted
// prologues are the matrix's (reach.hpp). What differs is where a word's results go: nothing is
// stored per cell; instead
//   evals  every evalACL of testConnection adds the service's weight at the slot that decided it --
//          the sink the conn_* templates count into (COUNT = true), so exactly the counts of
//          pg_classify(PG_MODE_CONN, counters) over the product's tuples
//   cells  the final word c << 30 | s of every pair that is not deferred adds the weight at 4 * s + c
// Both histograms are a window of u32 cells per workgroup (LDS on the device) in front of the u64
// output arrays; rules_plan decides the windows and after how many words a workgroup has to flush
// them so that no cell can wrap.
#pragma once
#include <string>
#include <vector>

#include "reach.hpp"

namespace pg {

constexpr uint32_t kRulesBlock = 256;            // threads of a k_rules_pairs workgroup
constexpr uint32_t kRulesMaxWeight = 65536;      // a service's weight at most
constexpr uint32_t kRulesMaxCells = 16384;       // u32 cells of both windows together (64 KiB: two workgroups per CU)
constexpr uint32_t kRulesHostGrid = 2;           // workgroups the host twin walks

// A windowed histogram: index x of [0, n) has window cell (x - base) mod n when that is below
// `cells`, else it goes to the u64 array at once. A window that starts before the end of the index
// space and wraps to its start holds the slots past the rules (the tables' default denies, "no
// ACL", "unresolved") and the first rules.
struct RulesWindow {
    uint32_t base, cells;
};

// How a call counts: the workgroup, the two windows and the words a workgroup processes between
// two flushes at most. One word adds up to 16 pairs x 4 evaluations x max_weight to one cell, so
// flush_words * 64 * max_weight < 2^32 (at the largest weight 1023 words, three rounds of a
// workgroup). The one function the launch, the host twin and pg_debug_reach_rules_plan use.
//   n_slots     counter slots; n_tail: the slots past the rules, the last of [0, n_slots)
//   hist_cells  "rules_hist_cells": cap of the cells of both windows together (0: none)
struct RulesPlan {
    uint32_t block;
    RulesWindow evals, cells;  // (cells: in units of one 4 * s + c index)
    uint32_t flush_words, lds_bytes;
};
inline RulesPlan rules_plan(uint32_t n_slots, uint32_t n_tail, bool evals, bool cells, uint32_t hist_cells,
                            uint32_t max_weight) {
    RulesPlan p{};
    p.block = kRulesBlock;
    const uint32_t budget = hist_cells < kRulesMaxCells ? hist_cells : kRulesMaxCells;
    // an evaluation histogram takes up to four increments a pair and the cells one: the evaluations
    // get up to three quarters of the budget first, the cells what is left (whole slots: four cells each)
    const uint32_t want_e = evals ? n_slots : 0u;
    const uint64_t want_c = cells ? 4ull * n_slots : 0ull;
    uint32_t ne = want_e;
    if (want_e + want_c > budget) ne = cells ? (want_e < budget / 4u * 3u ? want_e : budget / 4u * 3u) : (want_e < budget ? want_e : budget);
    uint32_t nc = (uint32_t)(want_c < (uint64_t)(budget - ne) ? want_c : (uint64_t)(budget - ne)) & ~3u;
    // a window that does not hold everything starts so that it holds the tail, up to half of it
    auto base = [&](uint32_t win_slots) {
        if (win_slots >= n_slots) return 0u;
        const uint32_t tail = n_tail < win_slots / 2u ? n_tail : win_slots / 2u;
        return tail ? n_slots - tail : 0u;
    };
    p.evals = RulesWindow{base(ne), ne};
    p.cells = RulesWindow{4u * base(nc / 4u), nc};
    const uint32_t w = max_weight ? max_weight : 1u;
    p.flush_words = (uint32_t)(0xFFFFFFFFull / (64ull * w));
    p.lds_bytes = 4u * (ne + nc);
    return p;
}

// One histogram as the per-word code sees it: the sink of the conn_* templates (inc, inc_t, inc_w,
// inc_cold: every increment adds the current service's weight) and add() for the cells.
//   win     the workgroup's window cells (LDS on the device; null: none)
//   glob    the u64 output array
//   n       the index space
// AGG (device): the lanes of the wave that share the first active lane's index add their weights
// with one atomic; the others one each. On the host every add is a plain one, and one that would
// wrap a cell sets *wrapped (the plan's flush bound makes that impossible; the twin checks it).
template <bool AGG>
struct RulesSink {
    uint32_t* win;
    unsigned long long* glob;
    RulesWindow w;
    uint32_t n, weight;
    bool* wrapped;

    PG_HD uint32_t cell(uint32_t x) const { return x >= w.base ? x - w.base : x + (n - w.base); }
    PG_HD void put(uint32_t x, uint32_t amount) const {
        const uint32_t c = cell(x);
#if defined(__HIP_DEVICE_COMPILE__)
        if (c < w.cells) {
            atomicAdd(&win[c], amount);
            return;
        }
        // past the window: one global atomic per distinct (index, amount) over the wave's lanes (one
        // amount per index unless the wave straddles two services)
        for (;;) {
            const uint32_t lead = __builtin_amdgcn_readfirstlane(x), al = __builtin_amdgcn_readfirstlane(amount);
            const unsigned long long m = __ballot(x == lead && amount == al);
            if (x == lead && amount == al) {
                if (__lane_id() == (unsigned)(__ffsll((long long)m) - 1))
                    atomicAdd(&glob[lead], (unsigned long long)al * (unsigned long long)__popcll(m));
                break;
            }
        }
#else
        if (c < w.cells) {
            if (win[c] + amount < win[c]) *wrapped = true;
            win[c] += amount;
        } else {
            glob[x] += amount;
        }
#endif
    }
    // n counts of index x (n * weight: at most 16 pairs of a word, 2^20, times a wave's 64 lanes)
    PG_HD void add_n(uint32_t x, uint32_t n) const {
        const uint32_t amount = n * weight;
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (AGG) {
            const uint32_t lead = __builtin_amdgcn_readfirstlane(x), al = __builtin_amdgcn_readfirstlane(amount);
            const unsigned long long m = __ballot(x == lead && amount == al);
            if (x == lead && amount == al) {
                if (__lane_id() == (unsigned)(__ffsll((long long)m) - 1)) put(lead, al * (uint32_t)__popcll(m));
                return;
            }
        }
#endif
        put(x, amount);
    }
    PG_HD void add(uint32_t x) const { add_n(x, 1u); }
    PG_HD void inc(uint32_t slot) const { add(slot); }
    PG_HD void inc_t(uint32_t slot, int32_t) const { add(slot); }
    PG_HD void inc_w(uint32_t word) const { add(word & kSlotMask); }
    PG_HD void inc_cold(uint32_t slot) const { add(slot); }
};

// the cells index of a final verdict word c << 30 | s
PG_HD uint32_t rules_cell_index(uint32_t word) { return (word & kSlotMask) << 2 | word >> 30; }

// The cells of one word, run-length coded in registers: consecutive dst of one src often end at the
// same rule (the src's own table decided), and a run is one add. end() after the word's last pair.
template <class SC>
struct RulesRun {
    const SC& sc;
    uint32_t idx = 0xFFFFFFFFu, n = 0;
    PG_HD void add(uint32_t word) {
        const uint32_t x = rules_cell_index(word);
        if (x != idx) {
            end();
            idx = x;
        }
        n++;
    }
    PG_HD void end() {
        if (n) sc.add_n(idx, n);
        n = 0;
    }
};

// ---- one word: dst j0 .. j0 + 15 (those below n_dst) of one (service, src), as reach_word_* runs
// it. A pair past n_dst is deferred: conn_* neither evaluates nor counts it, and its word stays out
// of the cells. EVALS / CELLS: the histograms asked for (se / sc are not touched otherwise).
template <bool WIDE, bool EVALS, bool CELLS, class L, class SE, class SC>
PG_HD void rules_word_uni(const DevTableSet& T, const DevNode& N, const L& img, const W4& rs1, uint32_t cs1, const W4* rec_d,
                          const uint32_t* cls_d, uint32_t j0, uint32_t n_dst, const W2& g, const SE& se, const SC& sc) {
    RulesRun<SC> run{sc};
    PG_UNROLL
    for (uint32_t r = 0; r < kReachWordPairs / kReachQ; r++) {
        const uint32_t jb = j0 + r * kReachQ;
        if (jb >= n_dst) break;
        W4 rs[kReachQ], rd[kReachQ];
        uint32_t cs[kReachQ], cd[kReachQ], gs[kReachQ], ga[kReachQ], o[kReachQ] = {};
        bool dfr[kReachQ];
        PG_UNROLL
        for (uint32_t q = 0; q < kReachQ; q++) {
            const uint32_t j = jb + q;
            dfr[q] = j >= n_dst;
            const uint32_t jj = dfr[q] ? n_dst - 1u : j;
            const DevLoader R{reinterpret_cast<const uint32_t*>(rec_d)};
            rd[q] = R.u4(4u * jj);
            cd[q] = cls_d[jj];
            rs[q] = rs1, cs[q] = cs1, gs[q] = g.x, ga[q] = g.y;
        }
        conn_uni_q<(int)kReachQ, EVALS, false, WIDE>(T, N, img, rs, rd, cs, cd, gs, ga, dfr, se, o);
        if (CELLS) {
            PG_UNROLL
            for (uint32_t q = 0; q < kReachQ; q++)
                if (!dfr[q]) run.add(o[q]);
        }
    }
    if (CELLS) run.end();
}

template <bool EVALS, bool CELLS, class SE, class SC>
PG_HD void rules_word_tab(const DevTableSet& T, const W4& es1, const W4* end_d, uint32_t j0, uint32_t n_dst, const W2& k,
                          const SE& se, const SC& sc) {
    RulesRun<SC> run{sc};
    for (uint32_t r = 0; r < kReachWordPairs / kReachQ; r++) {
        const uint32_t jb = j0 + r * kReachQ;
        if (jb >= n_dst) break;
        End es[kReachQ], ed[kReachQ];
        uint32_t src[kReachQ], dst[kReachQ], ks[kReachQ], ka[kReachQ], o[kReachQ] = {};
        bool dfr[kReachQ];
        PG_UNROLL
        for (uint32_t q = 0; q < kReachQ; q++) {
            const uint32_t j = jb + q;
            dfr[q] = j >= n_dst;
            const uint32_t jj = dfr[q] ? n_dst - 1u : j;
            const DevLoader R{reinterpret_cast<const uint32_t*>(end_d)};
            const W4 d = R.u4(4u * jj);
            es[q] = End{(int32_t)es1.x, (int32_t)es1.y, (int32_t)es1.z};
            ed[q] = End{(int32_t)d.x, (int32_t)d.y, (int32_t)d.z};
            src[q] = es1.w, dst[q] = d.w, ks[q] = k.x, ka[q] = k.y;
        }
        const TabEval<(int)kReachQ> ev{T, src, dst, ks, ka};
        conn_q<(int)kReachQ, EVALS>(T, ev, es, ed, se, o, dfr);
        if (CELLS) {
            PG_UNROLL
            for (uint32_t q = 0; q < kReachQ; q++)
                if (!dfr[q]) run.add(o[q]);
        }
    }
    if (CELLS) run.end();
}

// the (service, src, first dst) of word w of a pass, numbered as k_reach_pairs numbers them: lanes
// run over the src of one (service, 16 dst), w = (k * row_words + jw) * n_src + i
struct RulesWord {
    uint32_t k, i, jw;
};
PG_HD RulesWord rules_word_of(uint64_t w, uint64_t n_words, uint32_t row_words, uint32_t n_src) {
    const uint64_t per_svc = (uint64_t)row_words * n_src;
    RulesWord r;
    if (n_words >> 32) {  // (uniform) 64-bit word indices; 32-bit divisions otherwise
        r.k = (uint32_t)(w / per_svc);
        const uint64_t rem = w - (uint64_t)r.k * per_svc;
        r.jw = (uint32_t)(rem / n_src), r.i = (uint32_t)(rem - (uint64_t)r.jw * n_src);
    } else {
        const uint32_t w32 = (uint32_t)w, ps = (uint32_t)per_svc;
        r.k = w32 / ps;
        const uint32_t rem = w32 - r.k * ps;
        r.jw = rem / n_src, r.i = rem - r.jw * n_src;
    }
    return r;
}

// What the pair kernel and the host twin work on beside the pass: the weights, the windows and the
// outputs. A workgroup's window cells are [evals cells | cells cells].
struct RulesArgs {
    const uint32_t* weight;        // per service (all n_svc)
    unsigned long long* out_evals; // null: not asked for
    unsigned long long* out_cells;
    RulesWindow evals, cells;
    uint32_t n_slots, flush_words;
};

// a workgroup's flush of one window cell: its count to the output array, the cell cleared
PG_HD uint32_t rules_index_of_cell(const RulesWindow& w, uint32_t n, uint32_t c) {
    const uint32_t x = c + w.base;
    return x >= n ? x - n : x;
}

// device.hpp-style API of the rules driver in reach.hip
struct RulesSpecDev {
    ReachSpecDev reach;
    const uint32_t* weight;       // host, n_svc (never null here)
    uint32_t n_slots, n_tail, max_weight;
};
// out_evals / out_cells: device, either may be null. evals_host (with out_evals): the n_slots counts
// as the call left them. Clears the outputs on the stream first and synchronises it at the end.
int dev_reach_rules(const DevTableSet& T, const Tuning& tu, const RulesSpecDev& spec, unsigned long long* out_evals,
                    unsigned long long* out_cells, std::vector<uint64_t>* evals_host, void* stream, std::string* err);
// workgroups of k_rules_pairs the device holds at once with lds_bytes of window and blocks_per_cu
int dev_rules_resident(const Tuning& tu, uint32_t lds_bytes);

}  // namespace pg
