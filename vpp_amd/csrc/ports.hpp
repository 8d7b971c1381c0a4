// Port sweep (pg_reach_ports): the open dst ports of every src x dst pair, written once for both
// sides like reach.hpp -- the gfx950 pair kernel (reach.hip) and the host twin
// (pg_debug_reach_ports_host, tests only) instantiate the same per-pair code.
//
// For a fixed protocol (TCP or UDP) and src port, evalACL looks at a packet's dst port only through
// the rules' dst-port ranges, so the verdict word of (src, dst, proto, sport, dport) is constant
// inside every elementary interval of the partition of 0..65535 by all rules' dst-port bounds
// (pg_port_intervals, capi_reach.cpp). A sweep over all 65,536 ports is K evaluations per pair, on the
// K representatives (proto, sport, lo[k]). The prologues are reach.hpp's: per end point
// reach_end_uni / reach_end_tab, per interval reach_svc_uni / reach_svc_tab on the representative.
//
// The interval loop is innermost: a pair's src and dst values are loaded once and stay in
// registers for all K intervals, which run in rounds of Q = 4 through conn_uni_q (form A) or
// conn_q over TabEval (form B), COUNT = false. The per-interval values ({gs, ga} or the key pair,
// and the interval's length) are indexed by the loop counter alone -- the same address in every
// lane. Output per pair: 2 bits per interval, 16 intervals per word, the words of a pair next to
// each other; the number of open (ALLOW) ports; optionally the K full words.
#pragma once
#include "reach.hpp"

namespace pg {

constexpr uint32_t kPortsAllow = 2;  // PG_CONN_ALLOW

// One pair over intervals 0 .. K - 1. eval(kk, dfr, o): the round's four evaluations on intervals
// kk[q] (an interval past K reads K - 1's values and is deferred: no evaluation, its bits stay 0).
// emit_code(w, word): code word w of the pair is complete; emit_words(k0, words of the round, how
// many of them are below K). -> the pair's open ports: the lengths of its ALLOW intervals.
template <class EV, class EC, class EW>
PG_HD uint32_t ports_pair(uint32_t K, const uint32_t* len, const EV& eval, const EC& emit_code, const EW& emit_words) {
    uint32_t open = 0, packed = 0;
    for (uint32_t k0 = 0; k0 < K; k0 += kReachQ) {
        uint32_t kk[kReachQ], o[kReachQ];
        bool dfr[kReachQ];
        PG_UNROLL
        for (uint32_t q = 0; q < kReachQ; q++) {
            dfr[q] = k0 + q >= K;
            kk[q] = dfr[q] ? K - 1u : k0 + q;
        }
        eval(kk, dfr, o);
        uint32_t valid = 0;
        PG_UNROLL
        for (uint32_t q = 0; q < kReachQ; q++) {
            if (dfr[q]) continue;
            const uint32_t code = o[q] >> 30;
            packed |= code << (2u * ((k0 + q) & (kReachWordPairs - 1u)));
            open += code == kPortsAllow ? len[kk[q]] : 0u;
            valid++;
        }
        emit_words(k0, o, valid);
        const uint32_t k1 = k0 + kReachQ;
        if ((k1 & (kReachWordPairs - 1u)) == 0u || k1 >= K) {
            emit_code(k0 / kReachWordPairs, packed);
            packed = 0;
        }
    }
    return open;
}

// form A: the pair's class records and classes, iv[k] = {gs, ga} of interval k's representative
template <bool WIDE, class L, class EC, class EW>
PG_HD uint32_t ports_pair_uni(const DevTableSet& T, const DevNode& N, const L& img, const W4& rs1, uint32_t cs1,
                              const W4& rd1, uint32_t cd1, const W2* iv, const uint32_t* len, uint32_t K,
                              const EC& emit_code, const EW& emit_words) {
    auto eval = [&](const uint32_t(&kk)[kReachQ], const bool(&dfr)[kReachQ], uint32_t(&o)[kReachQ]) {
        W4 rs[kReachQ], rd[kReachQ];
        uint32_t cs[kReachQ], cd[kReachQ], gs[kReachQ], ga[kReachQ];
        PG_UNROLL
        for (uint32_t q = 0; q < kReachQ; q++) {
            const W2 g = iv[kk[q]];
            rs[q] = rs1, rd[q] = rd1, cs[q] = cs1, cd[q] = cd1, gs[q] = g.x, ga[q] = g.y;
        }
        conn_uni_q<(int)kReachQ, false, false, WIDE>(T, N, img, rs, rd, cs, cd, gs, ga, dfr, Hist{nullptr, nullptr}, o);
    };
    return ports_pair(K, len, eval, emit_code, emit_words);
}

// form B: the pair's ends {interface | kind, tin, tout, address}, iv[k] = {SYN key, SYN-ACK key}
template <class EC, class EW>
PG_HD uint32_t ports_pair_tab(const DevTableSet& T, const W4& es1, const W4& ed1, const W2* iv, const uint32_t* len,
                              uint32_t K, const EC& emit_code, const EW& emit_words) {
    auto eval = [&](const uint32_t(&kk)[kReachQ], const bool(&dfr)[kReachQ], uint32_t(&o)[kReachQ]) {
        End es[kReachQ], ed[kReachQ];
        uint32_t src[kReachQ], dst[kReachQ], ks[kReachQ], ka[kReachQ];
        PG_UNROLL
        for (uint32_t q = 0; q < kReachQ; q++) {
            const W2 k = iv[kk[q]];
            es[q] = End{(int32_t)es1.x, (int32_t)es1.y, (int32_t)es1.z};
            ed[q] = End{(int32_t)ed1.x, (int32_t)ed1.y, (int32_t)ed1.z};
            src[q] = es1.w, dst[q] = ed1.w, ks[q] = k.x, ka[q] = k.y;
        }
        const TabEval<(int)kReachQ> ev{T, src, dst, ks, ka};
        conn_q<(int)kReachQ, false>(T, ev, es, ed, Hist{nullptr, nullptr}, o, dfr);
    };
    return ports_pair(K, len, eval, emit_code, emit_words);
}

// device.hpp-style API of the sweep (reach.hip)
struct PortsSpecDev {         // host arrays
    const uint32_t* src_ip;
    const uint32_t* dst_ip;
    const uint32_t* lo;       // the K interval bounds (pg_port_intervals)
    uint32_t n_src, n_dst, K, protocol, src_port;
};
int dev_reach_ports(const DevTableSet& T, const Tuning& tu, const PortsSpecDev& spec, uint32_t* out_codes,
                    uint32_t* out_open, uint32_t* out_words, void* stream, std::string* err);
// the length of interval k of K bounds
inline uint32_t ports_len(const uint32_t* lo, uint32_t K, uint32_t k) { return (k + 1u < K ? lo[k + 1u] : 65536u) - lo[k]; }

}  // namespace pg
