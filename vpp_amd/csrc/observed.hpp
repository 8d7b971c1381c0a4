// Observed reachability (pg_reach_observed): a flow log folded into the audits' packed matrix over
// the caller's end-point lists and services, written once for both sides like zones.hpp -- the gfx950
// kernels (observed.hip) and the host twin (pg_debug_reach_observed_host, tests only) run the same
// per-flow code over the same tables.
//
// The output is pg_reach_matrix's layout: n_svc * n_src rows of reach_row_words(n_dst) words, 2 bits
// per cell; a marked cell holds PG_CONN_ALLOW (bit 2 * (j & 15) + 1 of its word), every other cell
// PG_CONN_DENY_SYN (0), padding zero. Marking is an OR of one bit, so the order of the flows, of the
// lanes and of the launches never shows in the result.
//
//   address table  one per side, open addressing over the *distinct* addresses of the list. A cell is
//                  three words {address, first, count}: the run idx[first .. first + count) of the
//                  side's index array, which lists 0 .. n - 1 sorted by (address, index). count == 0
//                  marks an empty cell -- no address does, 0.0.0.0 and 255.255.255.255 are end points
//                  like any other. The cells are a power of two, at least twice the list's length
//                  (obs_cap: from the length alone, so a plan needs no list), the start cell is
//                  obs_hash, a probe walks upwards and wraps; at most half the cells are taken, so it
//                  ends at an empty cell, and it is bounded by the cell count on any memory.
//   service table  the distinct keys of the services ascending (obs_key: protocol, dst port and -- with
//                  PG_OBSERVED_MATCH_SRC_PORT -- src port, the ports of TCP and UDP only), key k with
//                  the run sidx[sstart[k] .. sstart[k + 1]) of the services sorted by (key, index). A
//                  flow's key is found by binary search (obs_svc_find).
//   per flow       obs_flow: the status, and for a matched flow every cell of V x S x D handed to a
//                  `mark(word, bit)` of the caller's -- an atomic OR on the device, a plain one here.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "blobwalk.hpp"

namespace pg {

constexpr uint32_t kObsMatched = 0, kObsNoSrc = 1, kObsNoDst = 2, kObsNoSvc = 3;   // PG_OBS_*
constexpr uint32_t kObsAccumulate = 1u, kObsMatchSrcPort = 2u, kObsFlagsAll = 3u;  // PG_OBSERVED_*
constexpr size_t kObsMaxSide = (size_t)1 << 20, kObsMaxSvc = 4096;
// a workgroup of 256 lanes; on the vector path a lane takes 8 consecutive flows per step (16-B loads
// of the ports, two of each address array, 8 B of protocols), on the scalar path one
constexpr uint32_t kObsBlock = 256, kObsVecFlows = 8;
constexpr uint32_t kObsCellWords = 3;  // {address, first, count}
// the dynamic LDS of a workgroup up to which address tables are staged beside the service table and
// the counters: two workgroups and more per CU
constexpr uint32_t kObsLdsMax = 64u << 10;
// the most flows of one launch (32-bit flow indices in the kernel); pieces are multiples of 64
constexpr uint64_t kObsMaxLaunchFlows = ((uint64_t)1 << 30) - 64;
// the counters of a call in scratch, u64 each: the four statuses, the ALLOW cells, then one per service
constexpr uint32_t kObsCntCells = 4, kObsCntSvc = 5;

// cells of the address table of a list of n addresses: a power of two, >= 2 n and >= 4
PG_HD uint32_t obs_cap(uint32_t n) {
    uint32_t c = 4;
    while (c < 2u * n) c <<= 1;
    return c;
}
// the cell a probe of `ip` starts at (mask = cells - 1): a multiplicative hash, its high bits folded into the low ones
PG_HD uint32_t obs_hash(uint32_t ip, uint32_t mask) {
    const uint32_t h = ip * 0x9E3779B1u;
    return (h ^ (h >> 15)) & mask;
}
// The run of `ip` in a table of mask + 1 cells: true and (*first, *count), or false at an empty cell.
// *steps (optional): the cells read.
template <class TAB>
PG_HD bool obs_find(TAB tab, uint32_t mask, uint32_t ip, uint32_t* first, uint32_t* count, uint32_t* steps = nullptr) {
    uint32_t c = obs_hash(ip, mask);
    for (uint32_t k = 0; k <= mask; k++, c = (c + 1u) & mask) {
        const uint32_t cnt = tab[kObsCellWords * c + 2u];
        if (steps) *steps = k + 1u;
        if (!cnt) return false;
        if (tab[kObsCellWords * c] == ip) {
            *first = tab[kObsCellWords * c + 1u], *count = cnt;
            return true;
        }
    }
    return false;
}

// protocol codes above 3 are read as 3, as pg_classify does
PG_HD uint32_t obs_proto(uint32_t p) { return p > 3u ? 3u : p; }
// the key of a service or of a flow: only TCP (0) and UDP (1) have ports
PG_HD uint64_t obs_key(uint32_t proto, uint32_t src_port, uint32_t dst_port, bool match_src_port) {
    const uint32_t p = obs_proto(proto);
    if (p > 1u) return (uint64_t)p << 32;
    return (uint64_t)p << 32 | (uint64_t)(dst_port & 0xFFFFu) << 16 | (match_src_port ? src_port & 0xFFFFu : 0u);
}
// the index of `key` among the nk ascending keys (two words each: low, high), or nk
template <class KEYS>
PG_HD uint32_t obs_svc_find(KEYS keys, uint32_t nk, uint64_t key) {
    uint32_t lo = 0, hi = nk;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint64_t k = (uint64_t)keys[2u * mid + 1u] << 32 | keys[2u * mid];
        if (k < key) lo = mid + 1u;
        else hi = mid;
    }
    if (lo < nk && ((uint64_t)keys[2u * lo + 1u] << 32 | keys[2u * lo]) == key) return lo;
    return nk;
}

// the tables of a call as the per-flow code reads them: on the device the address tables and the
// service arrays point into LDS or HBM, on the host into ObservedTables
template <class P>
struct ObsView {
    P src_tab, dst_tab;            // cells
    P src_idx, dst_idx;            // index arrays (always HBM on the device)
    P skeys, sstart, sidx;         // service table
    uint32_t src_mask, dst_mask, nk;
    uint32_t n_src, row_words;     // of the output
    bool match_src_port;
};

// One flow: its status, *key_at = the index of its key where it matched (else unchanged); mark(word,
// bit) for every cell of V x S x D
template <class P, class MARK>
PG_HD uint32_t obs_flow(const ObsView<P>& T, uint32_t src, uint32_t dst, uint32_t src_port, uint32_t dst_port, uint32_t proto,
                        uint32_t* key_at, MARK mark) {
    uint32_t sf = 0, sc = 0, df = 0, dc = 0;
    if (!obs_find(T.src_tab, T.src_mask, src, &sf, &sc)) return kObsNoSrc;
    if (!obs_find(T.dst_tab, T.dst_mask, dst, &df, &dc)) return kObsNoDst;
    const uint32_t k = obs_svc_find(T.skeys, T.nk, obs_key(proto, src_port, dst_port, T.match_src_port));
    if (k == T.nk) return kObsNoSvc;
    *key_at = k;
    const uint32_t v0 = T.sstart[k], v1 = T.sstart[k + 1u];
    for (uint32_t b = 0; b < dc; b++) {
        const uint32_t j = T.dst_idx[df + b];
        const uint32_t jw = j >> 4, bit = 2u << (2u * (j & 15u));  // PG_CONN_ALLOW
        for (uint32_t a = 0; a < sc; a++) {
            const uint32_t i = T.src_idx[sf + a];
            for (uint32_t q = v0; q < v1; q++) mark((T.sidx[q] * T.n_src + i) * T.row_words + jw, bit);
        }
    }
    return kObsMatched;
}

// the ALLOW cells of a word
PG_HD uint32_t obs_allow_cells(uint32_t w) { return (uint32_t)__builtin_popcount((w >> 1) & ~w & 0x55555555u); }

// ---- host side: the tables, the plan --------------------------------------------------------------
struct ObservedSide {
    std::vector<uint32_t> tab, idx;  // kObsCellWords * cap words; n indices
    uint32_t cap = 0;
};
inline ObservedSide observed_side(const uint32_t* ip, uint32_t n) {
    ObservedSide s;
    s.cap = obs_cap(n);
    s.tab.assign((size_t)kObsCellWords * s.cap, 0u);
    s.idx.resize(n);
    for (uint32_t i = 0; i < n; i++) s.idx[i] = i;
    std::sort(s.idx.begin(), s.idx.end(), [&](uint32_t a, uint32_t b) { return ip[a] != ip[b] ? ip[a] < ip[b] : a < b; });
    const uint32_t mask = s.cap - 1u;
    for (uint32_t f = 0; f < n;) {
        uint32_t e = f + 1u;
        while (e < n && ip[s.idx[e]] == ip[s.idx[f]]) e++;
        uint32_t c = obs_hash(ip[s.idx[f]], mask);
        while (s.tab[kObsCellWords * c + 2u]) c = (c + 1u) & mask;
        uint32_t* cell = &s.tab[(size_t)kObsCellWords * c];
        cell[0] = ip[s.idx[f]], cell[1] = f, cell[2] = e - f;
        f = e;
    }
    return s;
}

struct ObservedSvc {
    std::vector<uint32_t> keys, start, idx;  // 2 nk; nk + 1; n_svc
    uint32_t nk = 0;
};
// proto / src_port / dst_port of service v through `get(v, &proto, &sport, &dport)`
template <class GET>
inline ObservedSvc observed_svc(uint32_t n_svc, bool match_src_port, GET get) {
    ObservedSvc s;
    std::vector<uint64_t> key(n_svc);
    for (uint32_t v = 0; v < n_svc; v++) {
        uint32_t p, sp, dp;
        get(v, &p, &sp, &dp);
        key[v] = obs_key(p, sp, dp, match_src_port);
    }
    s.idx.resize(n_svc);
    for (uint32_t v = 0; v < n_svc; v++) s.idx[v] = v;
    std::sort(s.idx.begin(), s.idx.end(), [&](uint32_t a, uint32_t b) { return key[a] != key[b] ? key[a] < key[b] : a < b; });
    for (uint32_t f = 0; f < n_svc; f++) {
        if (f && key[s.idx[f]] == key[s.idx[f - 1]]) continue;
        s.keys.push_back((uint32_t)key[s.idx[f]]), s.keys.push_back((uint32_t)(key[s.idx[f]] >> 32));
        s.start.push_back(f);
    }
    s.nk = (uint32_t)s.start.size();
    s.start.push_back(n_svc);
    return s;
}

// How a launch is laid out, from the lengths alone: the cells of both address tables, which of them a
// workgroup stages in LDS (the src table if it fits under the budget beside the service part, then the
// dst table if it fits in what is left; the others are probed in HBM), the dynamic LDS, the
// workgroup and -- filled in by dev_observed_plan -- the most workgroups of a launch. lds_budget:
// "observed_lds_bytes". The one function the launch and pg_debug_reach_observed_plan use. Host only.
struct ObservedPlan {
    uint32_t src_cap, dst_cap;
    uint32_t src_in_lds, dst_in_lds;
    uint32_t svc_bytes, lds_bytes;  // the service table with its counters; all dynamic LDS
    uint32_t block, vec_flows;      // lanes; flows of a lane per step on the vector path
    uint32_t grid;
};
// LDS words of the service part: keys (2 per service at most), starts, indices, a counter per key and
// the four status counters, rounded up to 16 B
PG_HD uint32_t obs_svc_words(uint32_t n_svc) { return (2u * n_svc + (n_svc + 1u) + n_svc + n_svc + 4u + 3u) & ~3u; }
inline ObservedPlan observed_plan(uint32_t n_src, uint32_t n_dst, uint32_t n_svc, uint32_t lds_budget) {
    ObservedPlan p{obs_cap(n_src), obs_cap(n_dst), 0, 0, 4u * obs_svc_words(n_svc), 0, kObsBlock, kObsVecFlows, 0};
    // (4096 services take 80 KiB on their own: then no address table is staged)
    const uint64_t room = p.svc_bytes < kObsLdsMax ? kObsLdsMax - p.svc_bytes : 0;
    uint64_t left = std::min<uint64_t>(lds_budget, room);
    const uint64_t sb = 4ull * kObsCellWords * p.src_cap, db = 4ull * kObsCellWords * p.dst_cap;
    if (sb <= left) p.src_in_lds = 1, left -= sb;
    if (db <= left) p.dst_in_lds = 1, left -= db;
    p.lds_bytes = p.svc_bytes + (p.src_in_lds ? (uint32_t)sb : 0u) + (p.dst_in_lds ? (uint32_t)db : 0u);
    return p;
}

// device.hpp-style API of observed.hip
struct ObservedSpecDev {
    const ObservedSide *src, *dst;  // host
    const ObservedSvc* svc;
    uint32_t n_src, n_dst, n_svc, flags;
    // the flow arrays, device; src_port only with kObsMatchSrcPort
    const uint32_t *f_src, *f_dst;
    const uint16_t *f_sport, *f_dport;
    const uint8_t* f_proto;
    uint64_t n;
};
struct ObservedKnobs {
    uint32_t blocks_per_cu, lds_bytes, test_first, launch_max;  // launch_max: "launch_max_tuples"
};
struct ObservedResult {  // pg_reach_observed_result
    uint64_t n_matched, n_no_src, n_no_dst, n_no_svc, n_cells;
};
// the plan with its grid under blocks_per_cu on the current device
ObservedPlan dev_observed_plan(uint32_t n_src, uint32_t n_dst, uint32_t n_svc, uint32_t lds_budget, uint32_t blocks_per_cu);
// out_packed device; out_flow / out_svc_flows device or null. 0, -1 (a HIP error) or -2 (the scratch
// allocation failed); synchronises the stream once, at its end
int dev_reach_observed(const ObservedKnobs& knobs, const ObservedSpecDev& spec, uint32_t* out_packed, uint8_t* out_flow,
                       uint64_t* out_svc_flows, ObservedResult* result, void* stream, std::string* err);

}  // namespace pg
