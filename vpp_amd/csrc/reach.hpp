// Reachability matrix (pg_reach_matrix): testConnection over src x dst x service, written once for
// both sides like classify.hpp -- the gfx950 kernels (reach.hip) and the host twin
// (pg_debug_reach_matrix_host, tests only) instantiate the same per-end-point, per-service and
// per-pair code.
//
// A matrix repeats every end point n_dst (or n_src) * n_svc times and every service n_src * n_dst
// times, so whatever pg_classify(CONN) derives from one address or one (protocol, port) alone is
// computed once per end point / service by a prologue, and a pair costs only testConnection's
// up-to-four evaluations on those values:
//   form A (a uniform node, services of protocol <= 2): per end point its node IP class and class
//          record, per service the node key classes of its SYN and SYN-ACK keys; a pair is
//          conn_uni_q over them -- cross-array entries only, no trie walk
//   form B (everything else): per end point its End by the iphash (probe_q), per service its two
//          L4 keys; a pair is conn_q over TabEval, as k_conn_queries runs it
// Both give the verdict words of pg_classify(PG_MODE_CONN) on the tuple (src, dst, sport, dport,
// proto). Nothing here counts: every evaluation is instantiated with COUNT = false.
//
// Output: 2 bits per pair, 16 pairs per word (reach_word_*: the unit of work is one output word,
// 16 consecutive dst of one (service, src), four rounds of Q = 4), and optionally the full words.
#pragma once
#include <algorithm>
#include <vector>

#include "classify.hpp"

namespace pg {

constexpr uint32_t kReachQ = 4, kReachWordPairs = 16;
constexpr size_t kReachMaxSide = (size_t)1 << 20, kReachMaxSvc = 4096;

PG_HD uint64_t reach_row_words(uint64_t n_dst) { return (n_dst + kReachWordPairs - 1) / kReachWordPairs; }

// a service as the kernels read it: {protocol clamped to 0..3, src port, dst port, 0}
PG_HD W4 reach_service(int32_t protocol, uint32_t sport, uint32_t dport) {
    return W4{protocol < 0 || protocol > 3 ? 3u : (uint32_t)protocol, sport, dport, 0u};
}

// ---- form A prologue: one end point -> {class record, class}, one service -> {gs, ga} ----------
template <class L>
PG_HD void reach_end_uni(const DevNode& N, const L& img, uint32_t ip, W4* rec, uint32_t* cls) {
    const uint32_t a[1] = {ip};
    uint32_t r[1];
    node_trie_q<false, true>(img, 0u, N.ip_s1, 32u, N.ip_depth, a, r);
    *rec = img.u4_at_byte(r[0]);
    *cls = (r[0] >> node_ip_rec_shift<true>()) - N.ipself;
}
// the node key classes of the service's SYN key (dst port) and SYN-ACK key (src port), the keys
// formed as classify_node_q's KEYS18 branch forms them (protocol <= 2)
template <class L>
PG_HD W2 reach_svc_uni(const DevNode& N, const L& img, const W4& s) {
    const uint32_t prm = (s.x & 3u) << 16, pm = s.x < 2u ? 0xFFFFu : 0u;
    const uint32_t k[2] = {prm | (s.z & pm), prm | (s.y & pm)};
    uint32_t r[2];
    node_trie_q<false, true>(img, N.key_root, N.key_k1, 18u, N.key_depth, k, r);
    return W2{(r[0] >> node_key_rec_shift<true>()) - N.kself, (r[1] >> node_key_rec_shift<true>()) - N.kself};
}

// ---- form B prologue: one end point -> {interface | kind, tin, tout, address}, one service ->
// {SYN key, SYN-ACK key} ---------------------------------------------------------------------------
PG_HD W4 reach_end_tab(const DevTableSet& T, uint32_t ip) {
    const uint32_t a[1] = {ip};
    End e[1];
    probe_q(T, a, e);
    return W4{(uint32_t)e[0].ifc, (uint32_t)e[0].tin, (uint32_t)e[0].tout, ip};
}
PG_HD W2 reach_svc_tab(const W4& s) { return W2{pkt_key(s.x, s.z), pkt_key(s.x, s.y)}; }

// ---- one output word: dst j0 .. j0 + 15 (those below n_dst) of one (service, src) ----------------
// A pair past n_dst reads dst n_dst - 1's values and is deferred (no evaluation); its bits stay 0.
// emit(round, words of the round's four pairs, pairs of the round below n_dst): the caller's store
// of the full verdict words (a no-op when they are not asked for).
template <bool WIDE, class L, class E>
PG_HD uint32_t reach_word_uni(const DevTableSet& T, const DevNode& N, const L& img, const W4& rs1, uint32_t cs1,
                              const W4* rec_d, const uint32_t* cls_d, uint32_t j0, uint32_t n_dst, const W2& g,
                              const E& emit) {
    uint32_t packed = 0;
    PG_UNROLL
    for (uint32_t r = 0; r < kReachWordPairs / kReachQ; r++) {
        const uint32_t jb = j0 + r * kReachQ;
        if (jb >= n_dst) break;
        W4 rs[kReachQ], rd[kReachQ];
        uint32_t cs[kReachQ], cd[kReachQ], gs[kReachQ], ga[kReachQ], o[kReachQ];
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
        conn_uni_q<(int)kReachQ, false, false, WIDE>(T, N, img, rs, rd, cs, cd, gs, ga, dfr, Hist{nullptr, nullptr}, o);
        uint32_t valid = 0;
        PG_UNROLL
        for (uint32_t q = 0; q < kReachQ; q++) {
            if (dfr[q]) continue;
            packed |= (o[q] >> 30) << (2u * (r * kReachQ + q));
            valid++;
        }
        emit(r, o, valid);
    }
    return packed;
}

template <class E>
PG_HD uint32_t reach_word_tab(const DevTableSet& T, const W4& es1, const W4* end_d, uint32_t j0, uint32_t n_dst,
                              const W2& k, const E& emit) {
    uint32_t packed = 0;
    for (uint32_t r = 0; r < kReachWordPairs / kReachQ; r++) {
        const uint32_t jb = j0 + r * kReachQ;
        if (jb >= n_dst) break;
        End es[kReachQ], ed[kReachQ];
        uint32_t src[kReachQ], dst[kReachQ], ks[kReachQ], ka[kReachQ], o[kReachQ];
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
        conn_q<(int)kReachQ, false>(T, ev, es, ed, Hist{nullptr, nullptr}, o, dfr);
        uint32_t valid = 0;
        PG_UNROLL
        for (uint32_t q = 0; q < kReachQ; q++) {
            if (dfr[q]) continue;
            packed |= (o[q] >> 30) << (2u * (r * kReachQ + q));
            valid++;
        }
        emit(r, o, valid);
    }
    return packed;
}

// The hoisted end-point arrays of one form, src and dst (the matrix's and the port sweep's).
struct ReachEnds {
    const W4* rec_s;          // form A: class records; form B: ends {interface, tin, tout, address}
    const W4* rec_d;
    const uint32_t* cls_s;    // form A: classes
    const uint32_t* cls_d;
    uint32_t n_src, n_dst;
};

// What a pair pass works on: the end points and the services it covers. A pass has
// n_list * n_src * row_words words: word jw of src i of service v = svc_list[k] lands at
// out_packed[(v * n_src + i) * row_words + jw], its full words at out_words[(v * n_src + i) * n_dst +
// 16 * jw ...] (the kernel numbers them with i fastest, reach.hip).
struct ReachPass : ReachEnds {
    const W2* svc;            // per service (all n_svc): form A {gs, ga}, form B {SYN key, SYN-ACK key}
    const uint32_t* svc_list; // the services of this pass
    uint32_t n_list;
    uint32_t* out_packed;
    uint32_t* out_words;      // null: not asked for
};

// device.hpp-style API of reach.hip
struct ReachSpecDev {         // host arrays
    const uint32_t* src_ip;
    const uint32_t* dst_ip;
    const W4* services;       // reach_service
    uint32_t n_src, n_dst, n_svc;
};
int dev_reach_matrix(const DevTableSet& T, const Tuning& tu, const ReachSpecDev& spec, uint32_t* out_packed,
                     uint32_t* out_words, void* stream, std::string* err);
// whether a call takes form A for the services of protocol <= 2 (the launch's and the host twin's
// one decision)
inline bool reach_form_a(const DevNode& nd, const Tuning& tu) { return nd.img && tu.node_path && nd.uniform; }
// The services of each form: *list = [form A ..., form B ...] -> how many are form A's. With weights
// (rule coverage), those that weigh nothing are left out.
inline uint32_t reach_form_split(bool form_a, const W4* svc, uint32_t n, const uint32_t* weight, std::vector<uint32_t>* list) {
    list->clear();
    for (uint32_t v = 0; v < n; v++)
        if (!weight || weight[v]) list->push_back(v);
    const auto mid = std::stable_partition(list->begin(), list->end(), [&](uint32_t v) { return form_a && svc[v].x <= 2u; });
    return (uint32_t)(mid - list->begin());
}

}  // namespace pg
