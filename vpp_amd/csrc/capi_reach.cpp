// extern "C" boundary of the reachability audits (include/policygpu.h): the matrix, the rule
// coverage, the port sweep, the diff, the closure, the groups, the paths, the classes, the zones, the
// dominators, the cut, the cost and the observed matrix, each with the host twin the tests compare its kernels to.
#include <algorithm>
#include <numeric>

#include "capi_internal.hpp"
#include "classes.hpp"
#include "closure.hpp"
#include "cost.hpp"
#include "cut.hpp"
#include "diff.hpp"
#include "dominators.hpp"
#include "groups.hpp"
#include "observed.hpp"
#include "paths.hpp"
#include "ports.hpp"
#include "rules.hpp"
#include "zones.hpp"

using namespace pg;

// ---- reachability matrix (reach.hpp) -------------------------------------------------------------
namespace {
// argument checks shared by pg_reach_matrix and its host twin: PG_OK with *empty set when there
// is nothing to do
int reach_args(pg_ctx* ctx, const pg_reach_spec* spec, const uint32_t* out_packed, bool* empty) {
    if (!ctx || !spec || !out_packed) return PG_EINVAL;
    if (spec->n_src > kReachMaxSide || spec->n_dst > kReachMaxSide) return fail(ctx, PG_EINVAL, "a side longer than 2^20");
    if (spec->n_svc > kReachMaxSvc) return fail(ctx, PG_EINVAL, "more than 4096 services");
    *empty = !spec->n_src || !spec->n_dst || !spec->n_svc;
    if (!*empty && (!spec->src_ip || !spec->dst_ip || !spec->services)) return fail(ctx, PG_EINVAL, "null spec array");
    return PG_OK;
}
std::vector<W4> reach_services(const pg_reach_spec* spec) {
    std::vector<W4> v(spec->n_svc);
    for (size_t k = 0; k < spec->n_svc; k++)
        v[k] = reach_service(spec->services[k].protocol, spec->services[k].src_port, spec->services[k].dst_port);
    return v;
}

// The hoisted arrays of the host twins, and one form's prologue over them as k_reach_ends and
// k_reach_svcs run it: rec (and cls, form A) of the end points src ++ dst, g[v] of the services in
// `list`.
struct HostHoist {
    std::vector<W4> rec;
    std::vector<uint32_t> cls;
    std::vector<W2> g;
    // spec: src_ip, dst_ip, n_src, n_dst. -> the form's end-point arrays
    template <class SPEC>
    ReachEnds run(bool uni, const DevTableSet& T, const SPEC& spec, const std::vector<W4>& svc, const uint32_t* list,
                  uint32_t n_list) {
        const uint32_t ns = (uint32_t)spec.n_src, nd = (uint32_t)spec.n_dst;
        const DevLoader img{T.node.img};
        rec.resize(ns + nd), cls.resize(ns + nd), g.resize(svc.size());
        for (uint32_t e = 0; e < ns + nd; e++) {
            const uint32_t ip = e < ns ? spec.src_ip[e] : spec.dst_ip[e - ns];
            if (uni) reach_end_uni(T.node, img, ip, &rec[e], &cls[e]);
            else rec[e] = reach_end_tab(T, ip);
        }
        for (uint32_t k = 0; k < n_list; k++) g[list[k]] = uni ? reach_svc_uni(T.node, img, svc[list[k]]) : reach_svc_tab(svc[list[k]]);
        const uint32_t* c = uni ? cls.data() : nullptr;
        return ReachEnds{rec.data(), rec.data() + ns, c, uni ? c + ns : nullptr, ns, nd};
    }
};

// every word of the services `list` (one form's), as k_reach_pairs runs them
template <bool UNI, bool WIDE>
void host_reach_pairs(const DevTableSet& T, const ReachPass& P) {
    const uint64_t rw = reach_row_words(P.n_dst);
    const DevLoader img{T.node.img};
    for (uint32_t k = 0; k < P.n_list; k++) {
        const uint32_t v = P.svc_list[k];
        for (uint32_t i = 0; i < P.n_src; i++) {
            const uint64_t row = (uint64_t)v * P.n_src + i;
            for (uint64_t jw = 0; jw < rw; jw++) {
                const uint32_t j0 = (uint32_t)jw * kReachWordPairs;
                uint32_t* ow = P.out_words ? P.out_words + row * P.n_dst + j0 : nullptr;
                auto emit = [&](uint32_t r, const uint32_t(&o)[kReachQ], uint32_t valid) {
                    for (uint32_t q = 0; ow && q < valid; q++) ow[r * kReachQ + q] = o[q];
                };
                uint32_t packed;
                if constexpr (UNI)
                    packed = reach_word_uni<WIDE>(T, T.node, img, P.rec_s[i], P.cls_s[i], P.rec_d, P.cls_d, j0, P.n_dst,
                                                  P.svc[v], emit);
                else
                    packed = reach_word_tab(T, P.rec_s[i], P.rec_d, j0, P.n_dst, P.svc[v], emit);
                P.out_packed[row * rw + jw] = packed;
            }
        }
    }
}
}  // namespace

extern "C" {

size_t pg_reach_row_words(size_t n_dst) { return (size_t)reach_row_words(n_dst); }

int pg_reach_matrix(pg_ctx* ctx, const pg_reach_spec* spec, uint32_t* out_packed, uint32_t* out_words,
                    void* stream) {
    bool empty = false;
    if (int rc = reach_args(ctx, spec, out_packed, &empty)) return rc;
    if (empty) return PG_OK;
    DEVICE_GUARD(ctx);
    GUARD_BEGIN
    int rc = ctx->eng.sync();
    if (rc) return rc;
    const DevTableSet& T = *ctx->eng.view();
    const std::vector<W4> svc = reach_services(spec);
    const ReachSpecDev sd{spec->src_ip, spec->dst_ip, svc.data(), (uint32_t)spec->n_src, (uint32_t)spec->n_dst,
                          (uint32_t)spec->n_svc};
    std::string err;
    if (dev_reach_matrix(T, ctx->eng.tune, sd, out_packed, out_words, stream, &err) != 0 ||
        dev_mark_use(ctx->eng.cur, stream, false, &err) != 0)
        return fail(ctx, PG_EIO, err);
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_matrix_host(pg_ctx* ctx, const pg_reach_spec* spec, uint32_t* out_packed, uint32_t* out_words,
                               int flags) {
    bool empty = false;
    if (int rc = reach_args(ctx, spec, out_packed, &empty)) return rc;
    GUARD_BEGIN
    if (empty) return PG_OK;
    Engine& E = ctx->eng;
    if (!E.compiled) E.compile();
    const DevTableSet T = host_view(E.host);
    const uint32_t nv = (uint32_t)spec->n_svc;
    const std::vector<W4> svc = reach_services(spec);
    const bool form_a = (flags & 1) && reach_form_a(T.node, E.tune);
    std::vector<uint32_t> list;
    const uint32_t na = reach_form_split(form_a, svc.data(), nv, nullptr, &list), nb = nv - na;
    const uint32_t *la = list.data(), *lb = la + na;
    HostHoist H;
    if (na) {
        const ReachEnds ends = H.run(true, T, *spec, svc, la, na);
        const ReachPass P{ends, H.g.data(), la, na, out_packed, out_words};
        if (T.node.wide) host_reach_pairs<true, true>(T, P);
        else host_reach_pairs<true, false>(T, P);
    }
    if (nb) {
        const ReachEnds ends = H.run(false, T, *spec, svc, lb, nb);
        const ReachPass P{ends, H.g.data(), lb, nb, out_packed, out_words};
        host_reach_pairs<false, false>(T, P);
    }
    return PG_OK;
    GUARD_END(ctx)
}

}  // extern "C"

// ---- rule coverage (rules.hpp) -------------------------------------------------------------------
namespace {
static_assert(sizeof(pg_reach_rules_plan) == 7 * sizeof(uint32_t), "pg_reach_rules_plan is seven words");

// what pg_reach_rules and its host twin work on once the arguments are checked
struct RulesCall {
    pg_reach_spec reach;           // the spec's pg_reach_spec fields
    std::vector<W4> svc;
    std::vector<uint32_t> weight;  // per service (1 where svc_weight is null)
    uint32_t n_slots = 0, n_rule_slots = 0, max_weight = 0;
    bool empty = false;
};

// Argument checks shared by pg_reach_rules and its host twin (inside a GUARD: the compile may
// throw). PG_OK: *c filled, *result = {layout_gen, n_cells, 0, n_slots, n_rule_slots, 0} (zeroed
// apart from n_slots and layout_gen when c->empty)
int rules_args(pg_ctx* ctx, const pg_reach_rules_spec* spec, const uint64_t* out_evals, const uint64_t* out_cells,
               pg_reach_rules_result* result, RulesCall* c) {
    if (!ctx) return PG_EINVAL;
    if (!spec || !result) return fail(ctx, PG_EINVAL, "null spec or result");
    if (!out_evals && !out_cells) return fail(ctx, PG_EINVAL, "out_evals and out_cells are both null");
    if (spec->n_src > kReachMaxSide || spec->n_dst > kReachMaxSide) return fail(ctx, PG_EINVAL, "a side longer than 2^20");
    if (spec->n_svc > kReachMaxSvc) return fail(ctx, PG_EINVAL, "more than 4096 services");
    c->empty = !spec->n_src || !spec->n_dst || !spec->n_svc;
    if (!c->empty && (!spec->src_ip || !spec->dst_ip || !spec->services)) return fail(ctx, PG_EINVAL, "null spec array");
    c->reach = pg_reach_spec{spec->src_ip, spec->n_src, spec->dst_ip, spec->n_dst, spec->services, spec->n_svc};
    uint64_t sum = 0;
    c->weight.assign(spec->n_svc, 1u);
    for (size_t v = 0; v < spec->n_svc; v++) {
        if (spec->svc_weight) c->weight[v] = spec->svc_weight[v];
        if (c->weight[v] > kRulesMaxWeight)
            return fail(ctx, PG_EINVAL, "svc_weight[" + std::to_string(v) + "] = " + std::to_string(c->weight[v]) + " is above 65536");
        sum += c->weight[v];
        c->max_weight = std::max(c->max_weight, c->weight[v]);
    }
    Engine& E = ctx->eng;
    if (!E.compiled) E.compile();
    c->n_slots = (uint32_t)E.slot_table.size();
    if (spec->n_slots != c->n_slots)
        return fail(ctx, PG_EINVAL, "n_slots is " + std::to_string(spec->n_slots) + " but the installed ACLs give " +
                                        std::to_string(c->n_slots) + " counter slots: they changed since pg_num_counter_slots");
    // (both sides <= 2^20 and the weights add to at most 2^28: the product fits 64 bits only after this check)
    const uint64_t pairs = (uint64_t)spec->n_src * spec->n_dst;
    if (sum && pairs > (((uint64_t)1 << 61) - 1u) / sum) return fail(ctx, PG_EINVAL, "n_src * n_dst * sum of weights * 4 reaches 2^63");
    *result = pg_reach_rules_result{E.layout_gen, 0, 0, c->n_slots, 0, 0};
    if (c->empty) return PG_OK;
    c->n_rule_slots = (uint32_t)std::count_if(E.slot_rule.begin(), E.slot_rule.end(), [](int32_t r) { return r >= 0; });
    result->n_cells = pairs * sum, result->n_rule_slots = c->n_rule_slots;
    c->svc = reach_services(&c->reach);
    return PG_OK;
}

// n_evals and n_dead_rules of a finished call from its evaluation counts
void rules_result(const Engine& E, const uint64_t* evals, pg_reach_rules_result* result) {
    for (uint32_t s = 0; s < result->n_slots; s++) {
        result->n_evals += evals[s];
        if (E.slot_rule[s] >= 0 && !evals[s]) result->n_dead_rules++;
    }
}

void host_rules_flush(uint32_t* win, const RulesWindow& w, uint32_t n, unsigned long long* out) {
    for (uint32_t c = 0; c < w.cells; c++) {
        if (win[c]) out[rules_index_of_cell(w, n, c)] += win[c];
        win[c] = 0;
    }
}

// every word of the services of one form, workgroup by workgroup and round by round as k_rules_pairs
// runs them, the window cells flushed where the kernel flushes them. -> a cell wrapped
template <bool UNI, bool WIDE, bool EVALS, bool CELLS>
bool host_rules_pairs(const DevTableSet& T, const ReachPass& P, const RulesArgs& A) {
    const uint32_t rw = (uint32_t)reach_row_words(P.n_dst);
    const uint64_t n_words = (uint64_t)P.n_list * P.n_src * rw, step = (uint64_t)kRulesHostGrid * kRulesBlock;
    const DevLoader img{T.node.img};
    std::vector<uint32_t> win((size_t)A.evals.cells + A.cells.cells + 1u);
    uint32_t *we = win.data(), *wc = win.data() + A.evals.cells;
    bool wrapped = false;
    auto flush = [&]() {
        if (EVALS) host_rules_flush(we, A.evals, A.n_slots, A.out_evals);
        if (CELLS) host_rules_flush(wc, A.cells, 4u * A.n_slots, A.out_cells);
    };
    for (uint32_t b = 0; b < kRulesHostGrid; b++) {
        uint32_t since = 0;
        for (uint64_t w0 = (uint64_t)b * kRulesBlock; w0 < n_words; w0 += step) {
            if (since + kRulesBlock > A.flush_words) flush(), since = 0;
            since += kRulesBlock;
            for (uint64_t w = w0; w < std::min<uint64_t>(w0 + kRulesBlock, n_words); w++) {
                const RulesWord x = rules_word_of(w, n_words, rw, P.n_src);
                const uint32_t v = P.svc_list[x.k], j0 = x.jw * kReachWordPairs, wgt = A.weight[v];
                const RulesSink<false> se{we, A.out_evals, A.evals, A.n_slots, wgt, &wrapped};
                const RulesSink<false> sc{wc, A.out_cells, A.cells, 4u * A.n_slots, wgt, &wrapped};
                if constexpr (UNI)
                    rules_word_uni<WIDE, EVALS, CELLS>(T, T.node, img, P.rec_s[x.i], P.cls_s[x.i], P.rec_d, P.cls_d, j0, P.n_dst,
                                                       P.svc[v], se, sc);
                else
                    rules_word_tab<EVALS, CELLS>(T, P.rec_s[x.i], P.rec_d, j0, P.n_dst, P.svc[v], se, sc);
            }
        }
        flush();
    }
    return wrapped;
}
template <bool UNI, bool WIDE>
bool host_rules_form(const DevTableSet& T, const ReachPass& P, const RulesArgs& A) {
    if (A.out_evals && A.out_cells) return host_rules_pairs<UNI, WIDE, true, true>(T, P, A);
    if (A.out_evals) return host_rules_pairs<UNI, WIDE, true, false>(T, P, A);
    return host_rules_pairs<UNI, WIDE, false, true>(T, P, A);
}
}  // namespace

extern "C" {

int pg_reach_rules(pg_ctx* ctx, const pg_reach_rules_spec* spec, uint64_t* out_evals, uint64_t* out_cells,
                   pg_reach_rules_result* result, void* stream) {
    GUARD_BEGIN
    RulesCall c;
    if (int rc = rules_args(ctx, spec, out_evals, out_cells, result, &c)) return rc;
    DEVICE_GUARD(ctx);
    int rc = ctx->eng.sync();
    if (rc) return rc;
    Engine& E = ctx->eng;
    const DevTableSet& T = *E.view();
    const ReachSpecDev rd{spec->src_ip, spec->dst_ip, c.svc.data(), (uint32_t)spec->n_src, (uint32_t)spec->n_dst,
                          (uint32_t)spec->n_svc};
    const RulesSpecDev sd{rd, c.weight.data(), c.n_slots, c.n_slots - c.n_rule_slots, c.max_weight};
    std::string err;
    std::vector<uint64_t> evals;
    if (dev_reach_rules(T, E.tune, sd, reinterpret_cast<unsigned long long*>(out_evals),
                        reinterpret_cast<unsigned long long*>(out_cells), &evals, stream, &err) != 0 ||
        dev_mark_use(E.cur, stream, false, &err) != 0)
        return fail(ctx, PG_EIO, err);
    if (out_evals && !c.empty) rules_result(E, evals.data(), result);
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_rules_host(pg_ctx* ctx, const pg_reach_rules_spec* spec, uint64_t* out_evals, uint64_t* out_cells,
                              pg_reach_rules_result* result, int flags) {
    GUARD_BEGIN
    RulesCall c;
    if (int rc = rules_args(ctx, spec, out_evals, out_cells, result, &c)) return rc;
    if (out_evals) std::fill(out_evals, out_evals + c.n_slots, (uint64_t)0);
    if (out_cells) std::fill(out_cells, out_cells + 4u * (size_t)c.n_slots, (uint64_t)0);
    if (c.empty) return PG_OK;
    Engine& E = ctx->eng;
    const DevTableSet T = host_view(E.host);
    const uint32_t nv = (uint32_t)spec->n_svc;
    const bool form_a = (flags & 1) && reach_form_a(T.node, E.tune);
    std::vector<uint32_t> list;  // (the services that weigh anything)
    const uint32_t na = reach_form_split(form_a, c.svc.data(), nv, c.weight.data(), &list), nb = (uint32_t)list.size() - na;
    const uint32_t *la = list.data(), *lb = la + na;
    const RulesPlan plan = rules_plan(c.n_slots, c.n_slots - c.n_rule_slots, out_evals != nullptr, out_cells != nullptr,
                                      E.tune.rules_hist_cells, c.max_weight);
    const RulesArgs A{c.weight.data(), reinterpret_cast<unsigned long long*>(out_evals),
                      reinterpret_cast<unsigned long long*>(out_cells), plan.evals, plan.cells, c.n_slots, plan.flush_words};
    HostHoist H;
    bool wrapped = false;
    if (na) {
        const ReachEnds ends = H.run(true, T, c.reach, c.svc, la, na);
        const ReachPass P{ends, H.g.data(), la, na, nullptr, nullptr};
        wrapped |= T.node.wide ? host_rules_form<true, true>(T, P, A) : host_rules_form<true, false>(T, P, A);
    }
    if (nb) {
        const ReachEnds ends = H.run(false, T, c.reach, c.svc, lb, nb);
        const ReachPass P{ends, H.g.data(), lb, nb, nullptr, nullptr};
        wrapped |= host_rules_form<false, false>(T, P, A);
    }
    if (wrapped) return fail(ctx, PG_EFAULT, "a 32-bit window cell wrapped between two flushes");
    if (out_evals) rules_result(E, out_evals, result);
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_rules_plan(pg_ctx* ctx, uint32_t n_slots, uint32_t n_tail, int evals, int cells, uint32_t max_weight,
                              pg_reach_rules_plan* plan, uint32_t* resident) {
    if (!ctx || !plan) return PG_EINVAL;
    GUARD_BEGIN
    if ((!evals && !cells) || n_tail > n_slots || max_weight > kRulesMaxWeight)
        return fail(ctx, PG_EINVAL, "no histogram, n_tail above n_slots or max_weight above 65536");
    const RulesPlan p = rules_plan(n_slots, n_tail, evals != 0, cells != 0, ctx->eng.tune.rules_hist_cells, max_weight);
    *plan = pg_reach_rules_plan{p.block, p.evals.cells, p.evals.base, p.cells.cells, p.cells.base, p.flush_words, p.lds_bytes};
    if (resident) {
        DEVICE_GUARD(ctx);
        *resident = (uint32_t)dev_rules_resident(ctx->eng.tune, p.lds_bytes);
    }
    return PG_OK;
    GUARD_END(ctx)
}

}  // extern "C"

// ---- port sweep (ports.hpp) ----------------------------------------------------------------------
namespace {
// The elementary dst-port intervals of a protocol: 0 and, of every installed rule whose L4 section
// of that protocol carries a dst range, the two bounds as evalACL compares them (after its uint16
// truncation, aclengine_mock.go:589): lower & 0xFFFF and (upper & 0xFFFF) + 1. Rules that never
// reach the comparison (a structural FAILURE before it, an empty range) only add cuts. Both
// protocols' bounds are kept with the engine until the next ACL change (Engine::touch).
const std::vector<uint32_t>& port_bounds(Engine& E, int protocol) {
    if (!E.port_lo_valid) {
        for (int p : {PG_PROTO_TCP, PG_PROTO_UDP}) {
            std::vector<uint32_t>& lo = E.port_lo[p];
            lo.assign(1, 0u);
            for (const auto& kv : E.by_name)
                for (const AclRule& r : kv.second->rules) {
                    const L4Section& s = p == PG_PROTO_TCP ? r.tcp : r.udp;
                    if (!s.present || !s.has_dst) continue;
                    lo.push_back(s.dst.lower & 0xFFFFu);
                    lo.push_back((s.dst.upper & 0xFFFFu) + 1u);
                }
            std::sort(lo.begin(), lo.end());
            lo.erase(std::unique(lo.begin(), lo.end()), lo.end());
            if (lo.back() == 65536u) lo.pop_back();
        }
        E.port_lo_valid = true;
    }
    return E.port_lo[protocol];
}

// argument checks shared by pg_reach_ports and its host twin: PG_OK with *empty set when there is
// nothing to do, else *lo = the partition the call runs on
int ports_args(pg_ctx* ctx, const pg_port_sweep_spec* spec, const uint32_t* out_codes, bool* empty,
               std::vector<uint32_t>* lo) {
    if (!ctx || !spec || !out_codes) return PG_EINVAL;
    if (spec->protocol != PG_PROTO_TCP && spec->protocol != PG_PROTO_UDP)
        return fail(ctx, PG_EINVAL, "a port sweep takes PG_PROTO_TCP or PG_PROTO_UDP");
    if (spec->n_src > kReachMaxSide || spec->n_dst > kReachMaxSide) return fail(ctx, PG_EINVAL, "a side longer than 2^20");
    *lo = port_bounds(ctx->eng, spec->protocol);
    if (spec->n_intervals != lo->size())
        return fail(ctx, PG_EINVAL, "n_intervals is " + std::to_string(spec->n_intervals) + " but the installed ACLs give " +
                                        std::to_string(lo->size()) + " intervals: they changed since pg_port_intervals");
    // (both sides <= 2^20 and row words <= 4097: the product fits 64 bits)
    if ((uint64_t)spec->n_src * spec->n_dst * reach_row_words(lo->size()) >> 32)
        return fail(ctx, PG_EINVAL, "n_src * n_dst * row_words(K) reaches 2^32");
    *empty = !spec->n_src || !spec->n_dst;
    if (!*empty && (!spec->src_ip || !spec->dst_ip)) return fail(ctx, PG_EINVAL, "null spec array");
    return PG_OK;
}

// every pair, as k_ports_pairs runs it
template <bool UNI, bool WIDE>
void host_ports_pairs(const DevTableSet& T, const ReachEnds& E, const W2* iv, const uint32_t* len, uint32_t K,
                      uint32_t* codes, uint32_t* open_ports, uint32_t* words) {
    const uint64_t rw = reach_row_words(K);
    const DevLoader img{T.node.img};
    for (uint32_t i = 0; i < E.n_src; i++)
        for (uint32_t j = 0; j < E.n_dst; j++) {
            const uint64_t p = (uint64_t)i * E.n_dst + j;
            auto emit_code = [&](uint32_t w, uint32_t word) { codes[p * rw + w] = word; };
            auto emit_words = [&](uint32_t k0, const uint32_t(&o)[kReachQ], uint32_t valid) {
                for (uint32_t q = 0; words && q < valid; q++) words[p * K + k0 + q] = o[q];
            };
            uint32_t open;
            if constexpr (UNI)
                open = ports_pair_uni<WIDE>(T, T.node, img, E.rec_s[i], E.cls_s[i], E.rec_d[j], E.cls_d[j], iv, len, K,
                                            emit_code, emit_words);
            else
                open = ports_pair_tab(T, E.rec_s[i], E.rec_d[j], iv, len, K, emit_code, emit_words);
            if (open_ports) open_ports[p] = open;
        }
}
}  // namespace

extern "C" {

int pg_port_intervals(pg_ctx* ctx, int protocol, uint32_t* lo, size_t cap) {
    if (!ctx) return PG_EINVAL;
    GUARD_BEGIN
    if (protocol != PG_PROTO_TCP && protocol != PG_PROTO_UDP)
        return fail(ctx, PG_EINVAL, "port intervals exist for PG_PROTO_TCP and PG_PROTO_UDP");
    const std::vector<uint32_t>& b = port_bounds(ctx->eng, protocol);
    if (lo) std::copy(b.begin(), b.begin() + std::min(cap, b.size()), lo);
    return (int)b.size();
    GUARD_END(ctx)
}

int pg_reach_ports(pg_ctx* ctx, const pg_port_sweep_spec* spec, uint32_t* out_codes, uint32_t* out_open,
                   uint32_t* out_words, void* stream) {
    GUARD_BEGIN
    bool empty = false;
    std::vector<uint32_t> lo;
    if (int rc = ports_args(ctx, spec, out_codes, &empty, &lo)) return rc;
    if (empty) return PG_OK;
    DEVICE_GUARD(ctx);
    int rc = ctx->eng.sync();
    if (rc) return rc;
    const DevTableSet& T = *ctx->eng.view();
    const PortsSpecDev sd{spec->src_ip, spec->dst_ip, lo.data(), (uint32_t)spec->n_src, (uint32_t)spec->n_dst,
                          (uint32_t)lo.size(), (uint32_t)spec->protocol, spec->src_port};
    std::string err;
    if (dev_reach_ports(T, ctx->eng.tune, sd, out_codes, out_open, out_words, stream, &err) != 0 ||
        dev_mark_use(ctx->eng.cur, stream, false, &err) != 0)
        return fail(ctx, PG_EIO, err);
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_ports_host(pg_ctx* ctx, const pg_port_sweep_spec* spec, uint32_t* out_codes, uint32_t* out_open,
                              uint32_t* out_words, int flags) {
    GUARD_BEGIN
    bool empty = false;
    std::vector<uint32_t> lo;
    if (int rc = ports_args(ctx, spec, out_codes, &empty, &lo)) return rc;
    if (empty) return PG_OK;
    Engine& E = ctx->eng;
    if (!E.compiled) E.compile();
    const DevTableSet T = host_view(E.host);
    const uint32_t K = (uint32_t)lo.size();
    const bool form_a = (flags & 1) && reach_form_a(T.node, E.tune);
    // the K representatives as services, all of one form
    std::vector<W4> svc(K);
    std::vector<uint32_t> list(K), len(K);
    std::iota(list.begin(), list.end(), 0u);
    for (uint32_t k = 0; k < K; k++) {
        svc[k] = reach_service(spec->protocol, spec->src_port, lo[k]);
        len[k] = ports_len(lo.data(), K, k);
    }
    HostHoist H;
    const ReachEnds ends = H.run(form_a, T, *spec, svc, list.data(), K);
    if (!form_a) host_ports_pairs<false, false>(T, ends, H.g.data(), len.data(), K, out_codes, out_open, out_words);
    else if (T.node.wide) host_ports_pairs<true, true>(T, ends, H.g.data(), len.data(), K, out_codes, out_open, out_words);
    else host_ports_pairs<true, false>(T, ends, H.g.data(), len.data(), K, out_codes, out_open, out_words);
    return PG_OK;
    GUARD_END(ctx)
}

}  // extern "C"

// ---- reachability diff (diff.hpp) ----------------------------------------------------------------
namespace {
static_assert(sizeof(pg_reach_change) == sizeof(DiffEntry), "pg_reach_change is diff.hpp's DiffEntry");

// argument checks shared by pg_reach_diff and its host twin: PG_OK with *empty set when there is no
// row (then *n_changes and trans are zeroed here)
int diff_args(pg_ctx* ctx, const pg_reach_diff_spec* spec, uint64_t* n_changes, uint64_t* trans, bool* empty) {
    if (!ctx) return PG_EINVAL;
    if (!spec || !spec->before || !spec->after || !n_changes)
        return fail(ctx, PG_EINVAL, "null spec, before, after or n_changes");
    if (!spec->n_cols || spec->n_cols > kDiffMaxCols) return fail(ctx, PG_EINVAL, "n_cols is 0 or above 2^20");
    if (spec->n_rows >> 32) return fail(ctx, PG_EINVAL, "n_rows reaches 2^32");
    // (n_rows < 2^32 and row_words <= 2^16: the product fits 64 bits)
    if (spec->n_rows * reach_row_words(spec->n_cols) >> 32) return fail(ctx, PG_EINVAL, "n_rows * row_words reaches 2^32");
    *empty = !spec->n_rows;
    if (*empty) {
        *n_changes = 0;
        if (trans) std::fill(trans, trans + 16, (uint64_t)0);
    }
    return PG_OK;
}
}  // namespace

extern "C" {

int pg_reach_diff(pg_ctx* ctx, const pg_reach_diff_spec* spec, pg_reach_change* changes, uint32_t* row_changes,
                  uint64_t* n_changes, uint64_t* trans, void* stream) {
    GUARD_BEGIN
    bool empty = false;
    if (int rc = diff_args(ctx, spec, n_changes, trans, &empty)) return rc;
    if (empty) return PG_OK;
    DEVICE_GUARD(ctx);
    const DiffSpecDev sd{spec->before, spec->after, (uint32_t)spec->n_rows, spec->n_cols, spec->transitions, spec->cap};
    std::string err;
    if (dev_reach_diff(ctx->eng.tune.blocks_per_cu, sd, reinterpret_cast<DiffEntry*>(changes), row_changes, n_changes, trans,
                       stream, &err) != 0)
        return fail(ctx, PG_EIO, err);
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_diff_host(pg_ctx* ctx, const pg_reach_diff_spec* spec, pg_reach_change* changes,
                             uint32_t* row_changes, uint64_t* n_changes, uint64_t* trans) {
    GUARD_BEGIN
    bool empty = false;
    if (int rc = diff_args(ctx, spec, n_changes, trans, &empty)) return rc;
    if (empty) return PG_OK;
    const uint32_t rw = (uint32_t)reach_row_words(spec->n_cols), n_rows = (uint32_t)spec->n_rows;
    const uint64_t cap = changes ? spec->cap : 0;
    uint64_t n = 0, hist[16] = {0};
    // every word in order, as the kernels' lanes run it
    for (uint32_t row = 0; row < n_rows; row++) {
        uint32_t in_row = 0;
        for (uint32_t jw = 0; jw < rw; jw++) {
            const uint32_t b = spec->before[(uint64_t)row * rw + jw], a = spec->after[(uint64_t)row * rw + jw];
            const uint32_t valid = diff_valid(spec->n_cols, jw);
            const DiffEq eb = diff_eq(b), ea = diff_eq(a);
            uint32_t h[16] = {0};
            if (b == a) diff_hist_same(eb, valid, h);
            else diff_hist(eb, ea, valid, h);
            for (int k = 0; k < 16; k++) hist[k] += h[k];
            for (uint32_t m = diff_selected(eb, ea, b ^ a, valid, spec->transitions); m; m &= m - 1u) {
                if (n < cap) changes[n] = pg_reach_change{row, diff_cell(jw, (uint32_t)__builtin_ctz(m), b, a)};
                n++, in_row++;
            }
        }
        if (row_changes) row_changes[row] = in_row;
    }
    *n_changes = n;
    if (trans) std::copy(hist, hist + 16, trans);
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_diff_plan(pg_ctx* ctx, uint64_t n_words, uint32_t* tile_words, uint32_t* grid, uint64_t* chunk_words) {
    if (!ctx || !tile_words || !grid || !chunk_words) return PG_EINVAL;
    GUARD_BEGIN
    DEVICE_GUARD(ctx);
    const DiffPlan p = dev_diff_plan(n_words, ctx->eng.tune.blocks_per_cu);
    *tile_words = p.tile_words, *grid = p.grid, *chunk_words = p.chunk_words;
    return PG_OK;
    GUARD_END(ctx)
}

}  // extern "C"

// ---- reachability closure (closure.hpp) ----------------------------------------------------------
namespace {
static_assert(sizeof(pg_reach_closure_result) == sizeof(ClosureResult), "pg_reach_closure_result is closure.hpp's ClosureResult");

// argument checks shared by pg_reach_closure and its host twin: PG_OK with *empty set when there is
// no end point (then *result is zeroed here), else *list = the selected slices
int closure_args(pg_ctx* ctx, const pg_reach_closure_spec* spec, const uint32_t* out_packed, pg_reach_closure_result* result,
                 bool* empty, std::vector<uint32_t>* list) {
    if (!ctx) return PG_EINVAL;
    if (!spec || !spec->matrix || !out_packed || !result)
        return fail(ctx, PG_EINVAL, "null spec, matrix, out_packed or result");
    if (spec->n > kClosureMaxN) return fail(ctx, PG_EINVAL, "more than 2^15 end points");
    if (!spec->n_svc || spec->n_svc > kClosureMaxSvc) return fail(ctx, PG_EINVAL, "n_svc is 0 or above 4096");
    *empty = !spec->n;
    if (*empty) *result = pg_reach_closure_result{0, 0, 0};
    for (uint32_t v = 0; v < spec->n_svc; v++)
        if (!spec->svc_select || spec->svc_select[v]) list->push_back(v);
    return PG_OK;
}
}  // namespace

extern "C" {

int pg_reach_closure(pg_ctx* ctx, const pg_reach_closure_spec* spec, uint32_t* out_packed, uint16_t* out_hops,
                     uint32_t* out_count, pg_reach_closure_result* result, void* stream) {
    GUARD_BEGIN
    bool empty = false;
    std::vector<uint32_t> list;
    if (int rc = closure_args(ctx, spec, out_packed, result, &empty, &list)) return rc;
    if (empty) return PG_OK;
    DEVICE_GUARD(ctx);
    const ClosureSpecDev sd{spec->matrix, spec->n, spec->n_svc, list.data(), (uint32_t)list.size(), spec->max_hops};
    std::string err;
    ClosureResult r{0, 0, 0};
    const int rc = dev_reach_closure(sd, out_packed, out_hops, out_count, &r, stream, &err);
    if (rc != 0) return fail(ctx, rc == -2 ? PG_ENOMEM : PG_EIO, err);
    *result = pg_reach_closure_result{r.levels, r.n_edges, r.n_reachable};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_closure_host(pg_ctx* ctx, const pg_reach_closure_spec* spec, uint32_t* out_packed, uint16_t* out_hops,
                                uint32_t* out_count, pg_reach_closure_result* result) {
    GUARD_BEGIN
    bool empty = false;
    std::vector<uint32_t> list;
    if (int rc = closure_args(ctx, spec, out_packed, result, &empty, &list)) return rc;
    if (empty) return PG_OK;
    const uint32_t n = spec->n, stride = closure_stride(n), chunks = closure_bit_words(n), rw = (uint32_t)reach_row_words(n);
    const size_t mat = (size_t)n * stride;
    std::vector<uint32_t> A(mat), R(mat), F(mat), Fn(mat), acc(stride);
    std::vector<uint8_t> live(n, 0), live_n(n);
    if (out_hops) std::fill(out_hops, out_hops + (size_t)n * n, (uint16_t)0);
    auto hops = [&](uint32_t i, uint32_t w, uint32_t bits, uint32_t level) {
        for (; out_hops && bits; bits &= bits - 1u) out_hops[(size_t)i * n + 32u * w + (uint32_t)__builtin_ctz(bits)] = (uint16_t)level;
    };
    // the edges, as k_closure_edges' lanes run them
    uint64_t reached = 0;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t w = 0; w < stride; w++) {
            const uint32_t valid = closure_valid(n, w);
            uint32_t a = 0;
            if (valid) {
                const size_t off = (size_t)i * rw + 2u * w;
                for (uint32_t v : list) {
                    const uint32_t* base = spec->matrix + (uint64_t)v * n * rw;
                    a |= closure_bits(base[off], 2u * w + 1u < rw ? base[off + 1] : 0u);
                }
                a &= valid;
            }
            A[(size_t)i * stride + w] = R[(size_t)i * stride + w] = F[(size_t)i * stride + w] = a;
            if (a) live[i] = 1;
            reached += (uint32_t)__builtin_popcount(a);
            hops(i, w, a, 1u);
        }
    result->n_edges = reached;
    uint32_t level = reached ? 1u : 0u;
    // one level per pass, as k_closure_step runs it: only live rows, only non-zero frontier words
    for (uint64_t fresh = reached; fresh && (!spec->max_hops || level < spec->max_hops);) {
        fresh = 0;
        for (uint32_t i = 0; i < n; i++) {
            uint32_t* fn = &Fn[(size_t)i * stride];
            live_n[i] = 0;
            std::fill(acc.begin(), acc.end(), 0u);
            if (live[i])
                for (uint32_t c = 0; c < chunks; c++)
                    for (uint32_t f = F[(size_t)i * stride + c]; f; f &= f - 1u) {
                        const uint32_t* a = &A[(size_t)(32u * c + (uint32_t)__builtin_ctz(f)) * stride];
                        for (uint32_t w = 0; w < stride; w++) acc[w] |= a[w];
                    }
            for (uint32_t w = 0; w < stride; w++) {
                uint32_t& r = R[(size_t)i * stride + w];
                const uint32_t nw = closure_new(acc[w], r);
                r |= nw, fn[w] = nw;
                if (nw) live_n[i] = 1;
                fresh += (uint32_t)__builtin_popcount(nw);
                hops(i, w, nw, level + 1u);
            }
        }
        reached += fresh;
        if (fresh) level++;
        F.swap(Fn), live.swap(live_n);
    }
    // as k_closure_pack
    for (uint32_t i = 0; i < n; i++) {
        uint32_t cnt = 0;
        for (uint32_t jw = 0; jw < rw; jw++) {
            const uint32_t h = (R[(size_t)i * stride + (jw >> 1)] >> (16u * (jw & 1u))) & 0xFFFFu;
            out_packed[(size_t)i * rw + jw] = closure_expand(h);
            cnt += (uint32_t)__builtin_popcount(h);
        }
        if (out_count) out_count[i] = cnt;
    }
    *result = pg_reach_closure_result{level, result->n_edges, reached};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_closure_plan(pg_ctx* ctx, uint32_t n, uint32_t* tile_rows, uint32_t* tile_cols, uint32_t* grid) {
    if (!ctx || !tile_rows || !tile_cols || !grid) return PG_EINVAL;
    const ClosurePlan p = closure_plan(n);
    *tile_rows = p.tile_rows, *tile_cols = p.tile_cols, *grid = p.grid;
    return PG_OK;
}

}  // extern "C"

// ---- reachability groups (groups.hpp) ------------------------------------------------------------
namespace {
static_assert(PG_GROUP_SKIP == kGroupsSkip && (int)PG_GROUPS_ALL == (int)PG_CONN_ALLOW, "groups.hpp's constants are the header's");

// argument checks shared by pg_reach_groups and its host twin: PG_OK with *nothing set when no
// output has an entry (no service, or an empty side with a group count of zero)
int groups_args(pg_ctx* ctx, const pg_reach_groups_spec* spec, const uint64_t* out_counts, bool* nothing) {
    if (!ctx) return PG_EINVAL;
    if (!spec || !out_counts) return fail(ctx, PG_EINVAL, "null spec or out_counts");
    if (spec->n_src > kGroupsMaxSide || spec->n_dst > kGroupsMaxSide) return fail(ctx, PG_EINVAL, "a side longer than 2^20");
    if (spec->n_svc > kGroupsMaxSvc) return fail(ctx, PG_EINVAL, "more than 4096 services");
    if (spec->n_src_groups > kGroupsMaxGroups || spec->n_dst_groups > kGroupsMaxGroups)
        return fail(ctx, PG_EINVAL, "n_src_groups or n_dst_groups above 4096");
    const bool empty = !spec->n_svc || !spec->n_src || !spec->n_dst;
    if (!spec->n_src_groups || !spec->n_dst_groups) {
        if (!empty) return fail(ctx, PG_EINVAL, "n_src_groups or n_dst_groups is 0");
        *nothing = true;
        return PG_OK;
    }
    if ((uint64_t)spec->n_svc * spec->n_src_groups * spec->n_dst_groups >> 30)
        return fail(ctx, PG_EINVAL, "n_svc * n_src_groups * n_dst_groups reaches 2^30");
    if (!spec->matrix && !empty) return fail(ctx, PG_EINVAL, "null matrix");
    if ((spec->n_src && !spec->src_group) || (spec->n_dst && !spec->dst_group))
        return fail(ctx, PG_EINVAL, "null src_group or dst_group");
    auto ids = [&](const char* what, const uint32_t* g, uint32_t n, uint32_t count) {
        for (uint32_t i = 0; i < n; i++)
            if (g[i] >= count && g[i] != kGroupsSkip)
                return fail(ctx, PG_EINVAL, std::string(what) + "[" + std::to_string(i) + "] = " + std::to_string(g[i]) +
                                                " is neither below its group count nor PG_GROUP_SKIP");
        return (int)PG_OK;
    };
    if (int rc = ids("src_group", spec->src_group, spec->n_src, spec->n_src_groups)) return rc;
    if (int rc = ids("dst_group", spec->dst_group, spec->n_dst, spec->n_dst_groups)) return rc;
    *nothing = !spec->n_svc;
    return PG_OK;
}
}  // namespace

extern "C" {

int pg_reach_groups(pg_ctx* ctx, const pg_reach_groups_spec* spec, uint64_t* out_counts, uint32_t* out_packed, void* stream) {
    GUARD_BEGIN
    bool nothing = false;
    if (int rc = groups_args(ctx, spec, out_counts, &nothing)) return rc;
    if (nothing) return PG_OK;
    DEVICE_GUARD(ctx);
    const GroupsPartition part = groups_partition(spec->src_group, spec->n_src, spec->n_src_groups, spec->dst_group,
                                                  spec->n_dst, groups_plan(spec->n_dst).chunk_rows);
    const GroupsSpecDev sd{spec->matrix, spec->n_svc, spec->n_src, spec->n_dst, spec->n_src_groups, spec->n_dst_groups, &part};
    std::string err;
    const int rc = dev_reach_groups(ctx->eng.tune.blocks_per_cu, sd, out_counts, out_packed, stream, &err);
    if (rc != 0) return fail(ctx, rc == -2 ? PG_ENOMEM : PG_EIO, err);
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_groups_host(pg_ctx* ctx, const pg_reach_groups_spec* spec, uint64_t* out_counts, uint32_t* out_packed) {
    GUARD_BEGIN
    bool nothing = false;
    if (int rc = groups_args(ctx, spec, out_counts, &nothing)) return rc;
    if (nothing) return PG_OK;
    const uint32_t n_dg = spec->n_dst_groups, rw = (uint32_t)reach_row_words(spec->n_dst), cells = 4u * n_dg;
    const uint32_t n_pair_rows = spec->n_svc * spec->n_src_groups;
    std::fill(out_counts, out_counts + (size_t)n_pair_rows * cells, (uint64_t)0);
    const GroupsPlan plan = groups_plan(spec->n_dst);
    const GroupsPartition P = groups_partition(spec->src_group, spec->n_src, spec->n_src_groups, spec->dst_group, spec->n_dst,
                                               plan.chunk_rows);
    const uint32_t tiles = (rw + plan.tile_words - 1u) / plan.tile_words, phases = kGroupsBlock / plan.tile_words;
    std::vector<uint32_t> acc(cells);
    // every work item in order, its lanes as k_groups_count runs them; the accumulators go to
    // out_counts after every item
    for (uint32_t v = 0; v < spec->n_svc && spec->n_dst; v++)
        for (const GroupsChunk& c : P.chunks)
            for (uint32_t tile = 0; tile < tiles; tile++) {
                std::fill(acc.begin(), acc.end(), 0u);
                for (uint32_t lane = 0; lane < kGroupsBlock; lane++) {
                    const uint32_t w = tile * plan.tile_words + lane % plan.tile_words, phase = lane / plan.tile_words;
                    if (w >= rw || c.r0 + phase >= c.r1) continue;
                    const uint32_t valid = diff_valid(spec->n_dst, w);
                    const uint32_t* base = spec->matrix + (uint64_t)v * spec->n_src * rw + w;
                    GroupsAcc a = {};
                    uint32_t n = 0;
                    for (uint32_t r = c.r0 + phase; r < c.r1; r += phases, n++) groups_add(a, base[(uint64_t)P.rows[r] * rw], valid);
                    uint32_t gw[8];
                    for (uint32_t k = 0; k < 8; k++) gw[k] = P.dgrp[16u * w + 2u * k] | (uint32_t)P.dgrp[16u * w + 2u * k + 1u] << 16;
                    groups_flush(a, n, gw, [&](uint32_t g, uint32_t code, uint32_t cnt) { acc[4u * g + code] += cnt; });
                }
                uint64_t* out = out_counts + ((size_t)v * spec->n_src_groups + c.gs) * cells;
                for (uint32_t i = 0; i < cells; i++) out[i] += acc[i];
            }
    // as k_groups_pack
    const uint32_t rwo = (uint32_t)reach_row_words(n_dg);
    for (uint32_t row = 0; out_packed && row < n_pair_rows; row++)
        for (uint32_t jw = 0; jw < rwo; jw++)
            out_packed[(size_t)row * rwo + jw] = groups_pack_word(out_counts + (size_t)row * cells, n_dg, jw);
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_groups_plan(pg_ctx* ctx, uint32_t n_dst, uint32_t* tile_words, uint32_t* chunk_rows) {
    if (!ctx || !tile_words || !chunk_rows) return PG_EINVAL;
    const GroupsPlan p = groups_plan(n_dst);
    *tile_words = p.tile_words, *chunk_rows = p.chunk_rows;
    return PG_OK;
}

}  // extern "C"

// ---- reachability paths (paths.hpp) --------------------------------------------------------------
namespace {
static_assert(sizeof(pg_reach_paths_result) == sizeof(PathsResult), "pg_reach_paths_result is paths.hpp's PathsResult");

// argument checks shared by pg_reach_paths and its host twin: PG_OK with *result zeroed
int paths_args(pg_ctx* ctx, const pg_reach_paths_spec* spec, const uint16_t* out_len, const uint16_t* out_nodes,
               pg_reach_paths_result* result) {
    if (!ctx) return PG_EINVAL;
    if (!spec || !spec->hops || !out_len || !result) return fail(ctx, PG_EINVAL, "null spec, hops, out_len or result");
    if (spec->n > kPathsMaxN) return fail(ctx, PG_EINVAL, "more than 2^15 end points");
    if (spec->n_queries > kPathsMaxQueries) return fail(ctx, PG_EINVAL, "n_queries above 2^24");
    if (spec->n_queries && (!spec->src || !spec->dst)) return fail(ctx, PG_EINVAL, "null src or dst");
    if (out_nodes) {
        if (!spec->max_len || spec->max_len > kPathsMaxLen) return fail(ctx, PG_EINVAL, "max_len is 0 or above 2^15");
        if (spec->n_queries * ((uint64_t)spec->max_len + 1u) >> 32)
            return fail(ctx, PG_EINVAL, "n_queries * (max_len + 1) reaches 2^32");
    }
    auto ids = [&](const char* what, const uint32_t* a) {
        for (uint64_t q = 0; q < spec->n_queries; q++)
            if (a[q] >= spec->n)
                return fail(ctx, PG_EINVAL, std::string(what) + "[" + std::to_string(q) + "] = " + std::to_string(a[q]) +
                                                " is not below n = " + std::to_string(spec->n));
        return (int)PG_OK;
    };
    if (int rc = ids("src", spec->src)) return rc;
    if (int rc = ids("dst", spec->dst)) return rc;
    *result = pg_reach_paths_result{0, 0, 0, 0, 0, 0};
    return PG_OK;
}
}  // namespace

extern "C" {

int pg_reach_paths(pg_ctx* ctx, const pg_reach_paths_spec* spec, uint16_t* out_len, uint16_t* out_nodes, uint32_t* out_via,
                   pg_reach_paths_result* result, void* stream) {
    GUARD_BEGIN
    if (int rc = paths_args(ctx, spec, out_len, out_nodes, result)) return rc;
    if (!spec->n) return PG_OK;  // (then there is no query either)
    if (!spec->n_queries && !out_via) return PG_OK;
    DEVICE_GUARD(ctx);
    PathsPartition part;
    if (spec->n_queries) part = paths_partition(spec->src, spec->dst, spec->n_queries, spec->n, paths_plan(spec->n).chunk_queries);
    const PathsSpecDev sd{spec->hops, spec->n, spec->max_len, spec->n_queries, spec->n_queries ? &part : nullptr};
    std::string err;
    PathsResult r{0, 0, 0, 0, 0, 0};
    const int rc = dev_reach_paths(ctx->eng.tune.blocks_per_cu, sd, out_len, out_nodes, out_via, &r, stream, &err);
    if (rc != 0) return fail(ctx, rc == -2 ? PG_ENOMEM : PG_EIO, err);
    *result = pg_reach_paths_result{r.n_found, r.n_unreachable, r.n_too_long, r.n_broken, r.n_via, r.longest};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_paths_host(pg_ctx* ctx, const pg_reach_paths_spec* spec, uint16_t* out_len, uint16_t* out_nodes,
                              uint32_t* out_via, pg_reach_paths_result* result) {
    GUARD_BEGIN
    if (int rc = paths_args(ctx, spec, out_len, out_nodes, result)) return rc;
    const uint32_t n = spec->n, stride = closure_stride(n), bw = closure_bit_words(n);
    if (out_via) std::fill(out_via, out_via + n, 0u);
    if (!spec->n_queries) return PG_OK;
    const uint32_t max_len = out_nodes ? spec->max_len : 0u;
    // the transposed edge bits, as k_paths_edges_t's lanes build them
    std::vector<uint32_t> ET((size_t)n * stride, 0u);
    for (uint32_t c = 0; c < n; c++)
        for (uint32_t w = 0; w < stride; w++) ET[(size_t)c * stride + w] = paths_edge_word(spec->hops, n, c, w);
    const PathsPartition P = paths_partition(spec->src, spec->dst, spec->n_queries, n, paths_plan(n).chunk_queries);
    pg_reach_paths_result r{0, 0, 0, 0, 0, 0};
    // every work item in order, its queries as k_paths_walk's waves run them: passes of 64 lanes, the
    // lowest lane with a match
    for (const PathsItem& item : P.items) {
        const uint16_t* row = spec->hops + (size_t)item.src * n;
        for (uint32_t q = item.q0; q < item.q1; q++) {
            const uint32_t j = P.dst[q], o = P.pos[q], d = row[j];
            const bool fits = d <= max_len;
            uint16_t* nrow = out_nodes ? out_nodes + (size_t)o * (max_len + 1u) : nullptr;
            bool broken = false;
            uint32_t cur = j;
            for (uint32_t t = d; t >= 2u && !broken; t--) {
                const uint32_t* et = &ET[(size_t)cur * stride];
                uint32_t k = kPathsNoPred;
                for (uint32_t wp = 0; wp < bw && k == kPathsNoPred; wp += kPathsPassWords)
                    for (uint32_t lane = 0; lane < 64u && k == kPathsNoPred; lane++) {
                        const uint32_t w = wp + lane;
                        k = paths_word_pred(w < bw ? et[w] : 0u, w, row, t - 1u);
                    }
                if (k == kPathsNoPred) {
                    broken = true;
                    break;
                }
                if (nrow && fits) paths_store(nrow, t - 1u, k);
                if (out_via) out_via[k]++;
                cur = k;
            }
            const bool found = d != 0u && !broken;
            out_len[o] = (uint16_t)(found ? d : 0u);
            if (nrow) {
                const bool written = found && fits;
                if (written) paths_store(nrow, 0u, item.src), paths_store(nrow, d, j);
                paths_fill(nrow, written ? d + 1u : 0u, max_len + 1u, 0u, 1u);
            }
            if (found) {
                r.n_found++, r.n_via += d - 1u, r.longest = std::max(r.longest, d);
                if (nrow && !fits) r.n_too_long++;
            } else if (broken) {
                r.n_broken++;
            } else {
                r.n_unreachable++;
            }
        }
    }
    *result = r;
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_paths_plan(pg_ctx* ctx, uint32_t n, uint32_t* chunk_queries, uint32_t* lds_bytes) {
    if (!ctx || !chunk_queries || !lds_bytes) return PG_EINVAL;
    const PathsPlan p = paths_plan(n);
    *chunk_queries = p.chunk_queries, *lds_bytes = p.lds_bytes;
    return PG_OK;
}

}  // extern "C"

// ---- reachability classes (classes.hpp) ----------------------------------------------------------
namespace {
static_assert(sizeof(pg_reach_classes_result) == sizeof(ClassesResult), "pg_reach_classes_result is classes.hpp's ClassesResult");

// argument checks shared by pg_reach_classes and its host twin: PG_OK with *result zeroed, and *empty
// set when there is nothing to do
int classes_args(pg_ctx* ctx, const pg_reach_classes_spec* spec, const uint32_t* out_src_class, const uint32_t* out_dst_class,
                 const uint32_t* out_quotient, pg_reach_classes_result* result, bool* empty) {
    if (!ctx) return PG_EINVAL;
    if (!spec || !result) return fail(ctx, PG_EINVAL, "null spec or result");
    if (!out_src_class && !out_dst_class) return fail(ctx, PG_EINVAL, "out_src_class and out_dst_class are both null");
    if (out_quotient && (!out_src_class || !out_dst_class))
        return fail(ctx, PG_EINVAL, "out_quotient needs out_src_class and out_dst_class");
    if (spec->n_src > kClassesMaxSide || spec->n_dst > kClassesMaxSide) return fail(ctx, PG_EINVAL, "a side longer than 2^20");
    if (spec->n_svc > kClassesMaxSvc) return fail(ctx, PG_EINVAL, "more than 4096 services");
    *empty = !spec->n_svc || !spec->n_src || !spec->n_dst;
    if (!*empty) {
        if (!spec->matrix) return fail(ctx, PG_EINVAL, "null matrix");
        if ((uint64_t)spec->n_svc * spec->n_src * reach_row_words(spec->n_dst) >> 32)
            return fail(ctx, PG_EINVAL, "n_svc * n_src * row_words reaches 2^32");
    }
    *result = pg_reach_classes_result{0, 0, 0};
    return PG_OK;
}
}  // namespace

extern "C" {

int pg_reach_classes(pg_ctx* ctx, const pg_reach_classes_spec* spec, uint32_t* out_src_class, uint32_t* out_dst_class,
                     uint32_t* out_src_rep, uint32_t* out_dst_rep, uint32_t* out_quotient, pg_reach_classes_result* result,
                     void* stream) {
    GUARD_BEGIN
    bool empty = false;
    if (int rc = classes_args(ctx, spec, out_src_class, out_dst_class, out_quotient, result, &empty)) return rc;
    if (empty) return PG_OK;
    DEVICE_GUARD(ctx);
    const ClassesSpecDev sd{spec->matrix, spec->n_svc, spec->n_src, spec->n_dst, ctx->eng.tune.classes_hash_bits};
    const ClassesOutDev od{out_src_class, out_dst_class, out_src_rep, out_dst_rep, out_quotient};
    std::string err;
    ClassesResult r{0, 0, 0};
    const int rc = dev_reach_classes(ctx->eng.tune.blocks_per_cu, sd, od, &r, stream, &err);
    if (rc != 0) return fail(ctx, rc == -2 ? PG_ENOMEM : PG_EIO, err);
    *result = pg_reach_classes_result{r.n_src_classes, r.n_dst_classes, r.rounds};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_classes_host(pg_ctx* ctx, const pg_reach_classes_spec* spec, uint32_t* out_src_class,
                                uint32_t* out_dst_class, uint32_t* out_src_rep, uint32_t* out_dst_rep, uint32_t* out_quotient,
                                pg_reach_classes_result* result) {
    GUARD_BEGIN
    bool empty = false;
    if (int rc = classes_args(ctx, spec, out_src_class, out_dst_class, out_quotient, result, &empty)) return rc;
    if (empty) return PG_OK;
    const uint32_t n_svc = spec->n_svc, n_src = spec->n_src, n_dst = spec->n_dst, rw = (uint32_t)reach_row_words(n_dst);
    const uint32_t n_rows = n_svc * n_src, bits = ctx->eng.tune.classes_hash_bits;
    const uint32_t* m = spec->matrix;
    const ClassesPlan plan = classes_plan(n_dst);
    const uint32_t tiles = (rw + plan.tile_words - 1u) / plan.tile_words, phases = kClassesBlock / plan.tile_words;
    // every work item (chunk of chunk_rows rows, tile) of a column kernel in order, its lanes as they
    // run: lane(w, first row, end of the chunk)
    auto column_items = [&](uint32_t chunk_rows, auto&& lane) {
        const uint32_t n_chunks = (n_rows + chunk_rows - 1u) / chunk_rows;
        for (uint32_t ch = 0; ch < n_chunks; ch++)
            for (uint32_t tile = 0; tile < tiles; tile++)
                for (uint32_t t = 0; t < kClassesBlock; t++) {
                    const uint32_t w = tile * plan.tile_words + t % plan.tile_words;
                    const uint64_t r0 = (uint64_t)ch * chunk_rows + t / plan.tile_words;
                    const uint64_t r1 = std::min<uint64_t>((uint64_t)(ch + 1u) * chunk_rows, n_rows);
                    if (w < rw && r0 < r1) lane(w, r0, r1);
                }
    };
    ClassesSide src, dst;
    std::vector<uint64_t> sig;
    if (out_src_class) {
        // as k_classes_hash_src: a wave per end point, its lanes' terms summed
        sig.assign(n_src, 0);
        for (uint32_t i = 0; i < n_src; i++)
            for (uint32_t lane = 0; lane < kClassesWave; lane++)
                for (uint32_t v = 0; v < n_svc; v++)
                    for (uint32_t w = lane; w < rw; w += kClassesWave)
                        sig[i] += classes_src_term(m[((uint64_t)v * n_src + i) * rw + w] & 3u * diff_valid(n_dst, w), w, v);
        // as k_classes_check_src: a wave per pair
        auto check = [&](const std::vector<uint32_t>& pending, const std::vector<uint32_t>& leader, std::vector<uint8_t>& differs) {
            for (size_t k = 0; k < pending.size(); k++) {
                const uint32_t a = pending[k], b = leader[a];
                uint32_t bad = 0;
                for (uint32_t v = 0; v < n_svc; v++)
                    for (uint32_t w = 0; w < rw; w++)
                        bad |= (m[((uint64_t)v * n_src + a) * rw + w] ^ m[((uint64_t)v * n_src + b) * rw + w]) & 3u * diff_valid(n_dst, w);
                differs[k] = bad != 0;
            }
            return 0;
        };
        classes_resolve(sig.data(), n_src, bits, check, &src);
    }
    if (out_dst_class) {
        // as k_classes_hash_dst
        sig.assign(16u * (size_t)rw, 0);
        column_items(plan.chunk_rows, [&](uint32_t w, uint64_t r0, uint64_t r1) {
            const uint32_t mask = 3u * diff_valid(n_dst, w);
            ClassesAcc a = {};
            for (uint64_t r = r0; r < r1; r += phases) classes_dst_add(a, m[r * rw + w] & mask, classes_row_key(r));
            for (uint32_t k = 0; k < 16; k++) sig[16u * (size_t)w + k] += a.h[k];
        });
        // as k_classes_check_dst
        std::vector<uint32_t> lead(16u * (size_t)rw), marks(16u * (size_t)rw);
        auto check = [&](const std::vector<uint32_t>& pending, const std::vector<uint32_t>& leader, std::vector<uint8_t>& differs) {
            for (uint32_t j = 0; j < 16u * rw; j++) lead[j] = j, marks[j] = 0;
            for (uint32_t j : pending) lead[j] = leader[j];
            column_items(plan.check_rows, [&](uint32_t w, uint64_t r0, uint64_t r1) {
                uint32_t ld[16];
                for (uint32_t k = 0; k < 16; k++) ld[k] = lead[16u * (size_t)w + k];
                if (!classes_dst_pending(ld, w)) return;
                uint32_t bad = 0;
                for (uint64_t r = r0; r < r1; r += phases) {
                    const uint32_t* row = m + r * rw;
                    bad |= classes_dst_differs(row[w], ld, w, [&](uint32_t lw) { return row[lw]; });
                }
                for (uint32_t k = 0; k < 16; k++)
                    if (bad >> k & 1u) marks[16u * (size_t)w + k] = 1u;
            });
            for (size_t k = 0; k < pending.size(); k++) differs[k] = marks[pending[k]] != 0;
            return 0;
        };
        classes_resolve(sig.data(), n_dst, bits, check, &dst);
    }
    if (out_src_class) std::copy(src.cls.begin(), src.cls.end(), out_src_class);
    if (out_src_class && out_src_rep) std::copy(src.rep.begin(), src.rep.end(), out_src_rep);
    if (out_dst_class) std::copy(dst.cls.begin(), dst.cls.end(), out_dst_class);
    if (out_dst_class && out_dst_rep) std::copy(dst.rep.begin(), dst.rep.end(), out_dst_rep);
    const uint32_t n_sc = (uint32_t)src.rep.size(), n_dc = (uint32_t)dst.rep.size();
    if (out_quotient) {  // as k_classes_quotient
        const uint32_t rwq = (uint32_t)reach_row_words(n_dc);
        for (uint32_t v = 0; v < n_svc; v++)
            for (uint32_t cs = 0; cs < n_sc; cs++)
                for (uint32_t jw = 0; jw < rwq; jw++) {
                    const uint32_t left = std::min(16u, n_dc - 16u * jw);
                    uint32_t rep[16] = {};
                    std::copy_n(dst.rep.begin() + 16u * jw, left, rep);
                    out_quotient[((size_t)v * n_sc + cs) * rwq + jw] =
                        classes_quotient_word(m + ((uint64_t)v * n_src + src.rep[cs]) * rw, rep, left);
                }
    }
    *result = pg_reach_classes_result{n_sc, n_dc, std::max(src.rounds, dst.rounds)};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_classes_plan(pg_ctx* ctx, uint32_t n_dst, uint32_t* tile_words, uint32_t* chunk_rows,
                                uint32_t* check_rows) {
    if (!ctx || !tile_words || !chunk_rows || !check_rows) return PG_EINVAL;
    const ClassesPlan p = classes_plan(n_dst);
    *tile_words = p.tile_words, *chunk_rows = p.chunk_rows, *check_rows = p.check_rows;
    return PG_OK;
}

}  // extern "C"

// ---- reachability zones (zones.hpp) --------------------------------------------------------------
namespace {
static_assert(sizeof(pg_reach_zones_result) == sizeof(ZonesResult), "pg_reach_zones_result is zones.hpp's ZonesResult");
static_assert(sizeof(pg_reach_zones_plan) == sizeof(ZonesPlan), "pg_reach_zones_plan is zones.hpp's ZonesPlan");

// argument checks shared by pg_reach_zones and its host twin: PG_OK with *empty set when there is no
// end point (then *result is zeroed here)
int zones_args(pg_ctx* ctx, const pg_reach_zones_spec* spec, const uint32_t* out_zone, const uint32_t* out_rep,
               const uint32_t* out_dag, pg_reach_zones_result* result, bool* empty) {
    if (!ctx) return PG_EINVAL;
    if (!spec || !out_zone || !result) return fail(ctx, PG_EINVAL, "null spec, out_zone or result");
    if (out_dag && !out_rep) return fail(ctx, PG_EINVAL, "out_dag needs out_rep");
    if (spec->n > kClosureMaxN) return fail(ctx, PG_EINVAL, "more than 2^15 end points");
    *empty = !spec->n;
    if (!*empty && !spec->matrix) return fail(ctx, PG_EINVAL, "null matrix");
    if (*empty) *result = pg_reach_zones_result{0, 0, 0, 0, 0};
    return PG_OK;
}
}  // namespace

extern "C" {

int pg_reach_zones(pg_ctx* ctx, const pg_reach_zones_spec* spec, uint32_t* out_zone, uint32_t* out_rep, uint32_t* out_size,
                   uint32_t* out_reaches, uint32_t* out_reached_by, uint32_t* out_dag, pg_reach_zones_result* result,
                   void* stream) {
    GUARD_BEGIN
    bool empty = false;
    if (int rc = zones_args(ctx, spec, out_zone, out_rep, out_dag, result, &empty)) return rc;
    if (empty) return PG_OK;
    DEVICE_GUARD(ctx);
    const ZonesOutDev od{out_zone, out_rep, out_size, out_reaches, out_reached_by, out_dag};
    std::string err;
    ZonesResult r{0, 0, 0, 0, 0};
    const int rc = dev_reach_zones(ctx->eng.tune.blocks_per_cu, spec->matrix, spec->n, od, &r, stream, &err);
    if (rc != 0) return fail(ctx, rc == -2 ? PG_ENOMEM : PG_EIO, err);
    *result = pg_reach_zones_result{r.n_zones, r.n_cyclic, r.n_multi, r.largest, r.n_broken};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_zones_host(pg_ctx* ctx, const pg_reach_zones_spec* spec, uint32_t* out_zone, uint32_t* out_rep,
                              uint32_t* out_size, uint32_t* out_reaches, uint32_t* out_reached_by, uint32_t* out_dag,
                              pg_reach_zones_result* result) {
    GUARD_BEGIN
    bool empty = false;
    if (int rc = zones_args(ctx, spec, out_zone, out_rep, out_dag, result, &empty)) return rc;
    if (empty) return PG_OK;
    const uint32_t n = spec->n, stride = closure_stride(n), bw = closure_bit_words(n), rw = (uint32_t)reach_row_words(n);
    const ZonesPlan plan = zones_plan(n);
    const bool counts = out_reaches || out_reached_by;
    std::vector<uint32_t> B((size_t)n * stride, 0xA5A5A5A5u), BT((size_t)n * stride, 0xA5A5A5A5u);  // (every word is written below)
    // every tile in order, as k_zones_bits_t runs it: the tile's words into `sh`, then per pair of word
    // columns the ballots of the two 64-row halves, lane by lane
    std::vector<uint32_t> sh((size_t)kZonesTileRows * kZonesTilePitch);
    for (uint32_t it = 0; it < plan.bits_grid; it++) {
        const uint32_t tr = it / plan.col_tiles, tc = it % plan.col_tiles, r0 = tr * kZonesTileRows, w0 = tc * kZonesTileWords;
        for (uint32_t r = 0; r < kZonesTileRows; r++)
            for (uint32_t wl = 0; wl < kZonesTileWords; wl++) {
                const uint32_t i = r0 + r, w = w0 + wl;
                uint32_t x = 0;
                if (i < n && w < stride) {
                    x = zones_bit_word(spec->matrix + (size_t)i * rw, rw, n, w);
                    B[(size_t)i * stride + w] = x;
                }
                sh[(size_t)r * kZonesTilePitch + wl] = x;
            }
        for (uint32_t q = 0; q < kZonesTileWords; q++)
            for (uint32_t k = 0; k < 32; k++) {
                uint64_t b[2] = {0, 0};
                for (uint32_t half = 0; half < 2; half++)
                    for (uint32_t lane = 0; lane < 64; lane++)
                        b[half] |= (uint64_t)zones_ballot_bit(sh[(size_t)(64u * half + lane) * kZonesTilePitch + q], k) << lane;
                const uint32_t c = 32u * (w0 + q) + k;
                if (c >= n) continue;
                uint32_t* bt = &BT[(size_t)c * stride + 4u * tr];
                bt[0] = (uint32_t)b[0], bt[1] = (uint32_t)(b[0] >> 32), bt[2] = (uint32_t)b[1], bt[3] = (uint32_t)(b[1] >> 32);
            }
    }
    // every row, as k_zones_label's waves run it: passes of 64 words, the lowest lane with a bit
    std::vector<uint32_t> label(n), mark(n, 0u), cnt_b(n, 0u), cnt_bt(n, 0u);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t *rb = &B[(size_t)i * stride], *rt = &BT[(size_t)i * stride];
        const uint32_t last = i >> 5, end = counts ? bw : last + 1u;
        uint32_t lab = i;
        bool found = false;
        for (uint32_t w0 = 0; w0 < end && !(found && !counts); w0 += 64u)
            for (uint32_t lane = 0; lane < 64u; lane++) {
                const uint32_t w = w0 + lane;
                if (w >= end) break;
                if (counts) cnt_b[i] += (uint32_t)__builtin_popcount(rb[w]), cnt_bt[i] += (uint32_t)__builtin_popcount(rt[w]);
                if (!found && w <= last && (rb[w] & rt[w])) lab = zones_label(i, w, rb[w] & rt[w]), found = true;
            }
        label[i] = lab, mark[lab] = 1u;
    }
    // as k_zones_number: the scan of the marks, then the ids, the sizes and the result
    std::vector<uint32_t> zid(n, 0u), rep, size;
    uint32_t cyclic = 0, broken = 0, multi = 0, largest = 0;
    for (uint32_t j = 0; j < n; j++) {
        if (!mark[j]) continue;
        const uint32_t at = (uint32_t)rep.size();
        zid[j] = at, rep.push_back(j);
        if (out_rep) out_rep[at] = j;
        if (out_reaches) out_reaches[at] = cnt_b[j];
        if (out_reached_by) out_reached_by[at] = cnt_bt[j];
        cyclic += zones_bit(&B[(size_t)j * stride], j);
    }
    const uint32_t n_zones = (uint32_t)rep.size();
    size.assign(n_zones, 0u);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t l = label[i], z = zid[l];
        out_zone[i] = z, size[z]++;
        broken += label[l] != l;
    }
    for (uint32_t z = 0; z < n_zones; z++) {
        if (out_size) out_size[z] = size[z];
        multi += size[z] > 1u, largest = std::max(largest, size[z]);
    }
    // as k_zones_dag: a zone per workgroup, a lane per output word
    const uint32_t rwz = (uint32_t)reach_row_words(n_zones);
    for (uint32_t a = 0; out_dag && a < n_zones; a++)
        for (uint32_t ow = 0; ow < rwz; ow++)
            out_dag[(size_t)a * rwz + ow] = zones_dag_word(&B[(size_t)rep[a] * stride], out_rep + 16u * ow, std::min(16u, n_zones - 16u * ow));
    *result = pg_reach_zones_result{n_zones, cyclic, multi, largest, broken};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_zones_plan(pg_ctx* ctx, uint32_t n, pg_reach_zones_plan* plan) {
    if (!ctx || !plan) return PG_EINVAL;
    if (n > kClosureMaxN) return fail(ctx, PG_EINVAL, "more than 2^15 end points");
    const ZonesPlan p = zones_plan(n);
    *plan = pg_reach_zones_plan{p.tile_rows, p.tile_cols, p.row_tiles, p.col_tiles, p.bits_grid, p.label_rows, p.label_grid, p.dag_grid};
    return PG_OK;
}

}  // extern "C"

// ---- reachability dominators (dominators.hpp) ----------------------------------------------------
namespace {
static_assert(sizeof(pg_reach_dominators_result) == sizeof(DomResult), "pg_reach_dominators_result is dominators.hpp's DomResult");
static_assert(sizeof(pg_reach_dominators_plan) == sizeof(DomPlan), "pg_reach_dominators_plan is dominators.hpp's DomPlan");

// argument checks shared by pg_reach_dominators and its host twin: PG_OK with *empty set when there
// is no end point (then *result is zeroed here), else *list = the selected slices
int dominators_args(pg_ctx* ctx, const pg_reach_dominators_spec* spec, pg_reach_dominators_result* result, bool* empty,
                    std::vector<uint32_t>* list) {
    if (!ctx) return PG_EINVAL;
    if (!spec || !result) return fail(ctx, PG_EINVAL, "null spec or result");
    if (spec->n > kDomMaxN) return fail(ctx, PG_EINVAL, "n: more than 2^15 end points");
    if (spec->n_entry > kDomMaxEntry) return fail(ctx, PG_EINVAL, "n_entry: more than 2^15 entries");
    if (!spec->n_svc || spec->n_svc > kDomMaxSvc) return fail(ctx, PG_EINVAL, "n_svc is 0 or above 4096");
    if (spec->n_entry && !spec->entry) return fail(ctx, PG_EINVAL, "null entry with n_entry > 0");
    *empty = !spec->n;
    if (!*empty && !spec->matrix) return fail(ctx, PG_EINVAL, "null matrix");
    for (uint32_t k = 0; k < spec->n_entry; k++)
        if (spec->entry[k] >= spec->n)
            return fail(ctx, PG_EINVAL, "entry[" + std::to_string(k) + "] = " + std::to_string(spec->entry[k]) + " is not below n");
    if (*empty) *result = pg_reach_dominators_result{0, 0, 0, 0, 0, 0};
    for (uint32_t v = 0; v < spec->n_svc; v++)
        if (!spec->svc_select || spec->svc_select[v]) list->push_back(v);
    return PG_OK;
}
}  // namespace

extern "C" {

int pg_reach_dominators(pg_ctx* ctx, const pg_reach_dominators_spec* spec, uint32_t* out_dom, uint16_t* out_idom,
                        uint32_t* out_cut, pg_reach_dominators_result* result, void* stream) {
    GUARD_BEGIN
    bool empty = false;
    std::vector<uint32_t> list;
    if (int rc = dominators_args(ctx, spec, result, &empty, &list)) return rc;
    if (empty) return PG_OK;
    DEVICE_GUARD(ctx);
    const DomSpecDev sd{spec->matrix, spec->n, spec->n_svc, list.data(), (uint32_t)list.size(), spec->entry, spec->n_entry};
    std::string err;
    DomResult r{0, 0, kDomNone, 0, 0, 0};
    const int rc = dev_reach_dominators(ctx->eng.tune.blocks_per_cu, sd, out_dom, out_idom, out_cut, &r, stream, &err);
    if (rc != 0) return fail(ctx, rc == -2 ? PG_ENOMEM : PG_EIO, err);
    *result = pg_reach_dominators_result{r.n_reached, r.n_chokes, r.top, r.top_cut, r.depth, r.rounds};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_dominators_host(pg_ctx* ctx, const pg_reach_dominators_spec* spec, uint32_t* out_dom, uint16_t* out_idom,
                                   uint32_t* out_cut, pg_reach_dominators_result* result) {
    GUARD_BEGIN
    bool empty = false;
    std::vector<uint32_t> list;
    if (int rc = dominators_args(ctx, spec, result, &empty, &list)) return rc;
    if (empty) return PG_OK;
    const uint32_t n = spec->n, se = closure_stride(n), sa = dom_stride(n), bw = closure_bit_words(n), rw = (uint32_t)reach_row_words(n);
    const DomPlan plan = dom_plan(n);
    // every tile in order, as k_edges_t (edge_tiles.hpp) runs it: the tile's words into `sh`, then per word column
    // the ballots of the two 64-row halves, lane by lane; the OR of 16 adjacent ET rows is the tile word
    std::vector<uint32_t> ET((size_t)n * se, 0xA5A5A5A5u), TE((size_t)plan.row_tiles * se, 0u);  // (every word of ET is written below)
    std::vector<uint32_t> sh((size_t)kDomTRows * kDomTPitch);
    for (uint32_t it = 0; it < plan.t_grid; it++) {
        const uint32_t tr = it / plan.t_col_tiles, tc = it % plan.t_col_tiles, r0 = tr * kDomTRows, w0 = tc * kDomTWords;
        for (uint32_t r = 0; r < kDomTRows; r++)
            for (uint32_t wl = 0; wl < kDomTWords; wl++) {
                const uint32_t i = r0 + r, w = w0 + wl;
                sh[(size_t)r * kDomTPitch + wl] =
                    i < n && w < se ? dom_edge_word(spec->matrix, list.data(), (uint32_t)list.size(), n, rw, i, w) : 0u;
            }
        for (uint32_t q = 0; q < kDomTWords; q++)
            for (uint32_t k = 0; k < 32; k++) {
                uint64_t b[2] = {0, 0};
                for (uint32_t half = 0; half < 2; half++)
                    for (uint32_t lane = 0; lane < 64; lane++)
                        b[half] |= (uint64_t)dom_ballot_bit(sh[(size_t)(64u * half + lane) * kDomTPitch + q], k) << lane;
                const uint32_t c = 32u * (w0 + q) + k;
                if (c >= n) continue;
                const uint32_t x[4] = {(uint32_t)b[0], (uint32_t)(b[0] >> 32), (uint32_t)b[1], (uint32_t)(b[1] >> 32)};
                for (uint32_t u = 0; u < 4; u++) ET[(size_t)c * se + 4u * tr + u] = x[u], TE[(size_t)(c >> 4) * se + 4u * tr + u] |= x[u];
            }
    }
    // as k_dom_init: the entries' rows, live bits and flags
    const size_t mat = (size_t)n * sa;
    std::vector<uint32_t> avoid(mat, 0u), D(mat, 0u), Dn(mat, 0u), live(se, 0u), live_n(se), acc(sa);
    std::vector<uint8_t> is_entry(n, 0);
    for (uint32_t k = 0; k < spec->n_entry; k++) {
        const uint32_t e = spec->entry[k];
        for (uint32_t w = 0; w < sa; w++) avoid[(size_t)e * sa + w] = D[(size_t)e * sa + w] = dom_entry_word(n, e, w);
        live[e >> 5] |= 1u << (e & 31u), is_entry[e] = 1;
    }
    // one round per pass, as k_dom_round runs it: a tile only where a live row has an edge into it, a
    // row over the live bits of its ET words
    uint32_t rounds = 0;
    for (bool go = spec->n_entry != 0; go;) {
        uint64_t grown = 0;
        std::fill(live_n.begin(), live_n.end(), 0u);
        for (uint32_t t = 0; t < plan.row_tiles; t++) {
            bool need = false;
            for (uint32_t c = 0; c < bw && !need; c++) need = (TE[(size_t)t * se + c] & live[c]) != 0;
            if (!need) continue;  // (the workgroup ends having written nothing)
            for (uint32_t v = t * kDomTileRows; v < std::min(n, (t + 1u) * kDomTileRows); v++) {
                std::fill(acc.begin(), acc.end(), 0u);
                for (uint32_t c = 0; c < bw; c++)
                    for (uint32_t f = ET[(size_t)v * se + c] & live[c]; f; f &= f - 1u) {
                        const uint32_t* d = &D[(size_t)(32u * c + (uint32_t)__builtin_ctz(f)) * sa];
                        for (uint32_t w = 0; w < sa; w++) acc[w] |= d[w];
                    }
                for (uint32_t w = 0; w < sa; w++) {
                    uint32_t& a = avoid[(size_t)v * sa + w];
                    const uint32_t nw = dom_new(acc[w], a, v, w);
                    a |= nw, Dn[(size_t)v * sa + w] = nw;
                    if (nw) live_n[v >> 5] |= 1u << (v & 31u);
                    grown += (uint32_t)__builtin_popcount(nw);
                }
            }
        }
        go = grown != 0;
        if (go) rounds++;
        D.swap(Dn), live.swap(live_n);
    }
    // as k_dom_rows: the sizes and the packed rows
    std::vector<uint32_t> size(n, 0u), cut(n, 0u);
    for (uint32_t v = 0; v < n; v++) {
        const uint32_t* row = &avoid[(size_t)v * sa];
        const bool reached = dom_reached(row, n);
        for (uint32_t jw = 0; jw < rw; jw++) {
            const uint32_t w = jw >> 1, h = (dom_word(row[w], reached, n, w) >> (16u * (jw & 1u))) & 0xFFFFu;
            if (out_dom) out_dom[(size_t)v * rw + jw] = closure_expand(h);
            size[v] += (uint32_t)__builtin_popcount(h);
        }
    }
    // as k_dom_cut: the column sums of Dom without its diagonal
    for (uint32_t v = 0; v < n; v++) {
        const uint32_t* row = &avoid[(size_t)v * sa];
        for (uint32_t w = 0; w < bw; w++)
            for (uint32_t d = dom_word(row[w], dom_reached(row, n), n, w) & ~dom_self(v, w); d; d &= d - 1u)
                cut[32u * w + (uint32_t)__builtin_ctz(d)]++;
    }
    if (out_cut) std::copy(cut.begin(), cut.end(), out_cut);
    // as k_dom_idom
    for (uint32_t v = 0; out_idom && v < n; v++) {
        uint32_t found = kDomNoIdom;
        const uint32_t* row = &avoid[(size_t)v * sa];
        if (size[v] > 1u)
            for (uint32_t w = 0; w < bw; w++)
                for (uint32_t d = dom_word(row[w], true, n, w) & ~dom_self(v, w); d; d &= d - 1u) {
                    const uint32_t k = 32u * w + (uint32_t)__builtin_ctz(d);
                    if (dom_is_idom(size[k], size[v])) found = std::min(found, k);
                }
        out_idom[v] = (uint16_t)found;
    }
    // as k_dom_result
    uint32_t reached = 0, chokes = 0, largest = 0;
    uint64_t key = 0;
    for (uint32_t v = 0; v < n; v++) {
        reached += size[v] != 0u, largest = std::max(largest, size[v]);
        if (cut[v] && !is_entry[v]) chokes++, key = std::max(key, dom_top_key(cut[v], v));
    }
    *result = pg_reach_dominators_result{reached, chokes, dom_top_of(key), (uint32_t)(key >> 32), largest ? largest - 1u : 0u, rounds};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_dominators_plan(pg_ctx* ctx, uint32_t n, pg_reach_dominators_plan* plan) {
    if (!ctx || !plan) return PG_EINVAL;
    if (n > kDomMaxN) return fail(ctx, PG_EINVAL, "n: more than 2^15 end points");
    const DomPlan p = dom_plan(n);
    *plan = pg_reach_dominators_plan{p.lane_words, p.tile_rows, p.tile_cols, p.row_tiles, p.col_tiles, p.round_grid,
                                     p.t_rows, p.t_cols, p.t_row_tiles, p.t_col_tiles, p.t_grid,
                                     p.cut_rows, p.cut_cols, p.cut_row_tiles, p.cut_col_tiles, p.cut_grid, p.finish_grid};
    return PG_OK;
}

}  // extern "C"

// ---- reachability cut (cut.hpp) ------------------------------------------------------------------
namespace {
static_assert(sizeof(pg_reach_cut_result) == sizeof(CutResult), "pg_reach_cut_result is cut.hpp's CutResult");
static_assert(sizeof(pg_reach_cut_plan) == sizeof(CutPlan), "pg_reach_cut_plan is cut.hpp's CutPlan");
static_assert(PG_CUT_NEAR == kCutNear && PG_CUT_FAR == kCutFar && PG_CUT_NEAR_REACH == kCutNearReach && PG_CUT_FAR_REACH == kCutFarReach,
              "out_cut's flags are cut.hpp's");

// what both sides work on: the selected slices, the distinct entries ascending, and E and T as bit vectors
struct CutArgs {
    bool empty = false;
    std::vector<uint32_t> list, entry, e_bits, t_bits;
};

int cut_ids(pg_ctx* ctx, const char* name, const uint32_t* ids, uint32_t count, uint32_t n, std::vector<uint32_t>* bits) {
    for (uint32_t k = 0; k < count; k++) {
        if (ids[k] >= n)
            return fail(ctx, PG_EINVAL, std::string(name) + "[" + std::to_string(k) + "] = " + std::to_string(ids[k]) + " is not below n");
        (*bits)[ids[k] >> 5] |= 1u << (ids[k] & 31u);
    }
    return PG_OK;
}

// argument checks shared by pg_reach_cut and its host twin: PG_OK with a->empty set when there is no
// end point (then *result is zeroed here)
int cut_args(pg_ctx* ctx, const pg_reach_cut_spec* spec, pg_reach_cut_result* result, CutArgs* a) {
    if (!ctx) return PG_EINVAL;
    if (!spec || !result) return fail(ctx, PG_EINVAL, "null spec or result");
    if (spec->n > kCutMaxN) return fail(ctx, PG_EINVAL, "n: more than 2^15 end points");
    if (spec->n_entry > kCutMaxList) return fail(ctx, PG_EINVAL, "n_entry: more than 2^15 entries");
    if (spec->n_target > kCutMaxList) return fail(ctx, PG_EINVAL, "n_target: more than 2^15 targets");
    if (spec->max_cut > kCutMaxCut) return fail(ctx, PG_EINVAL, "max_cut is above 2^15");
    if (!spec->n_svc || spec->n_svc > kCutMaxSvc) return fail(ctx, PG_EINVAL, "n_svc is 0 or above 4096");
    if (spec->n_entry && !spec->entry) return fail(ctx, PG_EINVAL, "null entry with n_entry > 0");
    if (spec->n_target && !spec->target) return fail(ctx, PG_EINVAL, "null target with n_target > 0");
    a->empty = !spec->n;
    if (!a->empty && !spec->matrix) return fail(ctx, PG_EINVAL, "null matrix");
    const uint32_t stride = closure_stride(spec->n);
    a->e_bits.assign(stride, 0u), a->t_bits.assign(stride, 0u);
    if (int rc = cut_ids(ctx, "entry", spec->entry, spec->n_entry, spec->n, &a->e_bits)) return rc;
    if (int rc = cut_ids(ctx, "target", spec->target, spec->n_target, spec->n, &a->t_bits)) return rc;
    if (a->empty) *result = pg_reach_cut_result{0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t v = 0; v < spec->n; v++)
        if (cut_bit(a->e_bits.data(), v)) a->entry.push_back(v);
    for (uint32_t v = 0; v < spec->n_svc; v++)
        if (!spec->svc_select || spec->svc_select[v]) a->list.push_back(v);
    return PG_OK;
}

// the host's search state: cut.hip's head and tail
struct CutHostSearch {
    std::vector<uint32_t> RX, RY, FX, FY, NX, NY;
};
// one level as k_cut_level runs it, word by word of the bit vectors -> grew; *target as the kernel's atomic min
bool cut_host_level(uint32_t n, uint32_t stride, const uint32_t* M, const uint16_t* link, bool plain, CutHostSearch& s, uint16_t* PX,
                    uint16_t* PY, const uint32_t* stop, uint32_t* target) {
    const uint32_t bw = closure_bit_words(n);
    bool grew = false;
    for (uint32_t g = 0; g < bw; g++) {
        const uint32_t rx = s.RX[g], ry = s.RY[g];
        uint32_t nx = 0, ny = 0;
        for (uint32_t b = 0; b < 32u && 32u * g + b < n; b++) {
            const uint32_t v = 32u * g + b;
            const uint16_t link_v = plain ? kCutNone : link[v];
            bool hx = false, hy = false;
            uint32_t px = v, py = v;
            if (!((rx >> b) & 1u)) {
                if (cut_x_back(link_v, (s.FY[g] >> b) & 1u)) {
                    hx = true;
                } else {
                    const uint32_t* row = M + (size_t)v * stride;
                    for (uint32_t w = 0; w < bw && !hx; w++)
                        if (const uint32_t x = cut_scan_word(row[w], s.FY[w], v, w)) px = cut_first(x, w), hx = true;
                }
            }
            if (plain) {
                hy = hx;
            } else if (!((ry >> b) & 1u)) {
                py = cut_y_source(link_v, v);
                hy = cut_bit(s.FX.data(), py);
            }
            if (hx) {
                nx |= 1u << b;
                if (PX) PX[v] = (uint16_t)px;
            }
            if (hy) {
                ny |= 1u << b;
                if (PY) PY[v] = (uint16_t)py;
            }
        }
        s.NX[g] = nx, s.NY[g] = ny, s.RX[g] = rx | nx, s.RY[g] = ry | ny;
        grew |= (nx | ny) != 0u;
        if (stop && (nx & stop[g])) *target = std::min(*target, cut_first(nx & stop[g], g));
    }
    return grew;
}
// as cut.hip's run_search
uint32_t cut_host_search(uint32_t n, uint32_t stride, const uint32_t* M, const uint16_t* link, bool plain, CutHostSearch& s, uint16_t* PX,
                         uint16_t* PY, const uint32_t* stop, uint32_t* levels) {
    s.NX.assign(stride, 0u), s.NY.assign(stride, 0u);
    for (;;) {
        uint32_t target = kCutNoTarget;
        const bool grew = cut_host_level(n, stride, M, link, plain, s, PX, PY, stop, &target);
        ++*levels;
        if (target != kCutNoTarget || !grew) return target;
        s.FX.swap(s.NX), s.FY.swap(s.NY);
    }
}
}  // namespace

extern "C" {

int pg_reach_cut(pg_ctx* ctx, const pg_reach_cut_spec* spec, uint8_t* out_cut, uint16_t* out_prev, uint16_t* out_next,
                 pg_reach_cut_result* result, void* stream) {
    GUARD_BEGIN
    CutArgs a;
    if (int rc = cut_args(ctx, spec, result, &a)) return rc;
    if (a.empty) return PG_OK;
    DEVICE_GUARD(ctx);
    const CutSpecDev sd{spec->matrix, spec->n, spec->n_svc, a.list.data(), (uint32_t)a.list.size(), a.entry.data(), (uint32_t)a.entry.size(),
                        a.e_bits.data(), a.t_bits.data(), spec->max_cut};
    std::string err;
    CutResult r{};
    const int rc = dev_reach_cut(ctx->eng.tune.blocks_per_cu, sd, out_cut, out_prev, out_next, &r, stream, &err);
    if (rc != 0) return fail(ctx, rc == -2 ? PG_ENOMEM : PG_EIO, err);
    *result = pg_reach_cut_result{r.separable, r.capped, r.n_direct, r.cut_size, r.n_paths, r.near_reach, r.far_reach, r.levels, r.reroutes};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_cut_host(pg_ctx* ctx, const pg_reach_cut_spec* spec, uint8_t* out_cut, uint16_t* out_prev, uint16_t* out_next,
                            pg_reach_cut_result* result) {
    GUARD_BEGIN
    CutArgs a;
    if (int rc = cut_args(ctx, spec, result, &a)) return rc;
    if (a.empty) return PG_OK;
    const uint32_t n = spec->n, stride = closure_stride(n), bw = closure_bit_words(n), rw = (uint32_t)reach_row_words(n);
    const uint32_t *e_bits = a.e_bits.data(), *t_bits = a.t_bits.data();
    // as k_edges_t leaves them: A from dom_edge_word, AT its transpose, padding zero
    std::vector<uint32_t> A((size_t)n * stride, 0u), AT((size_t)n * stride, 0u);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t w = 0; w < bw; w++) {
            const uint32_t x = dom_edge_word(spec->matrix, a.list.data(), (uint32_t)a.list.size(), n, rw, i, w);
            A[(size_t)i * stride + w] = x;
            for (uint32_t d = x; d; d &= d - 1u) AT[(size_t)(32u * w + (uint32_t)__builtin_ctz(d)) * stride + (i >> 5)] |= 1u << (i & 31u);
        }
    std::vector<uint16_t> prev(n, kCutNone), next(n, kCutNone), p_in(n, 0), p_out(n, 0);
    std::vector<uint8_t> flags(n, 0);
    CutResult r{};
    r.cut_size = kCutNoSize;
    // as k_cut_direct
    for (uint32_t e : a.entry)
        for (uint32_t w = 0; w < bw; w++) r.n_direct += (uint32_t)__builtin_popcount(cut_direct_word(A[(size_t)e * stride + w], t_bits[w], e, w));
    // the heads, as dev_reach_cut makes them
    CutHostSearch fwd_t, bwd;
    fwd_t.RX = a.e_bits, fwd_t.FY = a.e_bits, fwd_t.FX.assign(stride, 0u), fwd_t.RY.assign(stride, 0u);
    bwd.RX = a.t_bits, bwd.FY = a.t_bits, bwd.FX.assign(stride, 0u), bwd.RY.assign(stride, 0u);
    for (uint32_t w = 0; w < stride; w++) fwd_t.RY[w] = bwd.RY[w] = e_bits[w] | t_bits[w];
    CutHostSearch fwd = fwd_t;
    if (!r.n_direct) {
        r.separable = 1;
        for (;;) {
            if (r.n_paths == spec->max_cut + 1u) {
                r.capped = 1;
                break;
            }
            fwd = fwd_t;
            const uint32_t target = cut_host_search(n, stride, AT.data(), next.data(), false, fwd, p_in.data(), p_out.data(), t_bits, &r.levels);
            if (target == kCutNoTarget) break;
            r.reroutes += cut_augment(target, p_in.data(), p_out.data(), e_bits, t_bits, prev.data(), next.data(), 2u * n + 2u);
            r.n_paths++;
        }
    }
    if (r.separable && !r.capped) {
        cut_host_search(n, stride, A.data(), prev.data(), false, bwd, nullptr, nullptr, nullptr, &r.levels);
        // as k_cut_sets
        std::vector<uint32_t> near(stride), far(stride);
        CutHostSearch rn, rf;
        rn.RX.resize(stride), rf.RX.resize(stride);
        for (uint32_t w = 0; w < stride; w++) {
            near[w] = cut_near_word(fwd.RX[w], fwd.RY[w], e_bits[w], t_bits[w]);
            far[w] = cut_far_word(bwd.RX[w], bwd.RY[w], e_bits[w], t_bits[w]);
            rn.RX[w] = e_bits[w] | near[w], rf.RX[w] = e_bits[w] | far[w];
        }
        rn.RY = rn.RX, rf.RY = rf.RX, rn.FY = rf.FY = a.e_bits, rn.FX.assign(stride, 0u), rf.FX.assign(stride, 0u);
        cut_host_search(n, stride, AT.data(), nullptr, true, rn, nullptr, nullptr, nullptr, &r.levels);
        cut_host_search(n, stride, AT.data(), nullptr, true, rf, nullptr, nullptr, nullptr, &r.levels);
        // as k_cut_finish
        for (uint32_t w = 0; w < stride; w++) {
            const uint32_t x[4] = {near[w], far[w], cut_reach_word(rn.RY[w], near[w]), cut_reach_word(rf.RY[w], far[w])};
            r.near_reach += (uint32_t)__builtin_popcount(x[2]), r.far_reach += (uint32_t)__builtin_popcount(x[3]);
            for (uint32_t b = 0; b < 32u && 32u * w + b < n; b++)
                flags[32u * w + b] = cut_flags((x[0] >> b) & 1u, (x[1] >> b) & 1u, (x[2] >> b) & 1u, (x[3] >> b) & 1u);
        }
        r.cut_size = r.n_paths;
    }
    if (out_cut) std::copy(flags.begin(), flags.end(), out_cut);
    if (out_prev) std::copy(prev.begin(), prev.end(), out_prev);
    if (out_next) std::copy(next.begin(), next.end(), out_next);
    *result = pg_reach_cut_result{r.separable, r.capped, r.n_direct, r.cut_size, r.n_paths, r.near_reach, r.far_reach, r.levels, r.reroutes};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_cut_plan(pg_ctx* ctx, uint32_t n, pg_reach_cut_plan* plan) {
    if (!ctx || !plan) return PG_EINVAL;
    if (n > kCutMaxN) return fail(ctx, PG_EINVAL, "n: more than 2^15 end points");
    const CutPlan p = cut_plan(n);
    *plan = pg_reach_cut_plan{p.lane_words, p.level_block, p.group_nodes, p.row_steps, p.level_grid,
                              p.t_rows, p.t_cols, p.t_row_tiles, p.t_col_tiles, p.t_grid, p.finish_block, p.finish_grid};
    return PG_OK;
}

}  // extern "C"

// ---- reachability cost (cost.hpp) ----------------------------------------------------------------
namespace {
static_assert(sizeof(pg_reach_cost_result) == sizeof(CostResult), "pg_reach_cost_result is cost.hpp's CostResult");
static_assert(sizeof(pg_reach_cost_plan) == sizeof(CostPlan), "pg_reach_cost_plan is cost.hpp's CostPlan");
static_assert(PG_COST_NONE == kCostNone && PG_COST_NO_PRED == kCostNoPred, "the not-reached marks are cost.hpp's");

// argument checks shared by pg_reach_cost and its host twin: PG_OK with *empty set when there is no
// end point or no source (then *result is zeroed here), else *list = the selected slices
int cost_args(pg_ctx* ctx, const pg_reach_cost_spec* spec, pg_reach_cost_result* result, bool* empty, std::vector<uint32_t>* list) {
    if (!ctx) return PG_EINVAL;
    if (!spec || !result) return fail(ctx, PG_EINVAL, "null spec or result");
    if (spec->n > kCostMaxN) return fail(ctx, PG_EINVAL, "n: more than 2^15 end points");
    if (spec->n_src > kCostMaxSrc) return fail(ctx, PG_EINVAL, "n_src: more than 2^15 sources");
    if ((uint64_t)spec->n_src * spec->n >= kCostMaxCells) return fail(ctx, PG_EINVAL, "n_src * n reaches 2^28");
    if (!spec->n_svc || spec->n_svc > kCostMaxSvc) return fail(ctx, PG_EINVAL, "n_svc is 0 or above 4096");
    if (spec->n && !spec->matrix) return fail(ctx, PG_EINVAL, "null matrix");
    if (spec->n_src && !spec->src) return fail(ctx, PG_EINVAL, "null src with n_src > 0");
    if (spec->n && !spec->weight) return fail(ctx, PG_EINVAL, "null weight with n > 0");
    for (uint32_t k = 0; k < spec->n_src; k++)
        if (spec->src[k] >= spec->n)
            return fail(ctx, PG_EINVAL, "src[" + std::to_string(k) + "] = " + std::to_string(spec->src[k]) + " is not below n");
    for (uint32_t v = 0; v < spec->n; v++)
        if (!spec->weight[v]) return fail(ctx, PG_EINVAL, "weight[" + std::to_string(v) + "] is 0");
    *empty = !spec->n || !spec->n_src;
    if (*empty) *result = pg_reach_cost_result{0, 0, 0, 0};
    for (uint32_t v = 0; v < spec->n_svc; v++)
        if (!spec->svc_select || spec->svc_select[v]) list->push_back(v);
    return PG_OK;
}
}  // namespace

extern "C" {

int pg_reach_cost(pg_ctx* ctx, const pg_reach_cost_spec* spec, uint32_t* out_cost, uint16_t* out_pred, uint16_t* out_len,
                  uint32_t* out_via, pg_reach_cost_result* result, void* stream) {
    GUARD_BEGIN
    bool empty = false;
    std::vector<uint32_t> list;
    if (int rc = cost_args(ctx, spec, result, &empty, &list)) return rc;
    if (empty && !(spec->n && out_via)) return PG_OK;
    DEVICE_GUARD(ctx);
    // (without a source the launch layer only clears out_via)
    const CostSpecDev sd{spec->matrix, spec->n, spec->n_svc, list.data(), (uint32_t)list.size(), spec->src, spec->n_src, spec->weight,
                         spec->max_cost};
    const CostKnobs knobs{ctx->eng.tune.blocks_per_cu, ctx->eng.tune.cost_lds_bytes};
    std::string err;
    CostResult r{};
    const int rc = dev_reach_cost(knobs, sd, out_cost, out_pred, out_len, out_via, &r, stream, &err);
    if (rc != 0) return fail(ctx, rc == -2 ? PG_ENOMEM : PG_EIO, err);
    *result = pg_reach_cost_result{r.n_reached, r.n_via, r.max_cost, r.longest};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_cost_host(pg_ctx* ctx, const pg_reach_cost_spec* spec, uint32_t* out_cost, uint16_t* out_pred, uint16_t* out_len,
                             uint32_t* out_via, pg_reach_cost_result* result) {
    GUARD_BEGIN
    bool empty = false;
    std::vector<uint32_t> list;
    if (int rc = cost_args(ctx, spec, result, &empty, &list)) return rc;
    const uint32_t n = spec->n;
    if (out_via) std::fill(out_via, out_via + n, 0u);
    if (empty) return PG_OK;
    const uint32_t stride = closure_stride(n), bw = closure_bit_words(n), rw = (uint32_t)reach_row_words(n);
    const uint16_t* wts = spec->weight;
    // as k_edges_t leaves them: A from dom_edge_word, ET its transpose, padding zero
    std::vector<uint32_t> A((size_t)n * stride, 0u), ET((size_t)n * stride, 0u);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t w = 0; w < bw; w++) {
            const uint32_t x = dom_edge_word(spec->matrix, list.data(), (uint32_t)list.size(), n, rw, i, w);
            A[(size_t)i * stride + w] = x;
            for (uint32_t d = x; d; d &= d - 1u) ET[(size_t)cost_first(d, w) * stride + (i >> 5)] |= 1u << (i & 31u);
        }
    std::vector<uint32_t> row(n), F(stride), N(stride), held(stride);
    std::vector<uint16_t> pred(n);
    CostResult r{};
    for (uint32_t q = 0; q < spec->n_src; q++) {
        const uint32_t s = spec->src[q];
        std::fill(row.begin(), row.end(), kCostNone);
        for (uint32_t w = 0; w < stride; w++) F[w] = dom_self(s, w), N[w] = 0u;
        // relax, as k_cost_rows: whole-frontier sweeps, here in ascending order
        for (uint32_t round = 0; round <= n; round++) {
            bool fell = false;
            for (uint32_t fw = 0; fw < bw; fw++)
                for (uint32_t px = F[fw]; px; px &= px - 1u) {
                    const uint32_t p = cost_first(px, fw), d = cost_base(row[p], p, s);
                    const uint32_t* arow = &A[(size_t)p * stride];
                    for (uint32_t w = 0; w < bw; w++)
                        for (uint32_t e = arow[w]; e; e &= e - 1u) {
                            const uint32_t v = cost_first(e, w);
                            uint32_t nd;
                            if (!cost_offer(d, wts[v], spec->max_cost, &nd) || nd >= row[v]) continue;
                            row[v] = nd, N[v >> 5] |= 1u << (v & 31u), fell = true;
                        }
                }
            if (!fell) break;
            std::fill(F.begin(), F.end(), 0u);
            std::swap(F, N);
        }
        // store
        std::fill(held.begin(), held.end(), 0u);
        for (uint32_t v = 0; v < n; v++) {
            if (out_cost) out_cost[(size_t)q * n + v] = row[v];
            if (row[v] != kCostNone) r.n_reached++, r.max_cost = std::max(r.max_cost, row[v]);
            if (cost_held(row[v], v, s)) held[v >> 5] |= 1u << (v & 31u);
        }
        // pull
        for (uint32_t v = 0; v < n; v++) {
            uint32_t pv = kCostNoPred;
            const uint32_t* trow = &ET[(size_t)v * stride];
            for (uint32_t w = 0; row[v] != kCostNone && w < bw && pv == kCostNoPred; w++)
                for (uint32_t e = trow[w] & held[w]; e && pv == kCostNoPred; e &= e - 1u) {
                    const uint32_t p = cost_first(e, w);
                    if (cost_ties(cost_base(row[p], p, s), wts[v], row[v])) pv = p;
                }
            pred[v] = (uint16_t)pv;
        }
        if (out_pred) std::copy(pred.begin(), pred.end(), out_pred + (size_t)q * n);
        // walk
        for (uint32_t v = 0; v < n; v++) {
            uint32_t len = 0;
            if (pred[v] != kCostNoPred) {
                len = cost_walk(
                    v, s, n, [&](uint32_t u) { return (uint32_t)pred[u]; },
                    [&](uint32_t k) {
                        if (out_via) out_via[k]++;
                    });
                r.n_via += len - 1u, r.longest = std::max(r.longest, len);
            }
            if (out_len) out_len[(size_t)q * n + v] = (uint16_t)len;
        }
    }
    *result = pg_reach_cost_result{r.n_reached, r.n_via, r.max_cost, r.longest};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_cost_plan(pg_ctx* ctx, uint32_t n, pg_reach_cost_plan* plan) {
    if (!ctx || !plan) return PG_EINVAL;
    if (n > kCostMaxN) return fail(ctx, PG_EINVAL, "n: more than 2^15 end points");
    const CostPlan p = cost_plan(n, ctx->eng.tune.cost_lds_bytes);
    *plan = pg_reach_cost_plan{p.lane_words, p.block, p.lds_bytes, p.row_in_lds, p.weights_in_lds,
                               p.t_rows, p.t_cols, p.t_row_tiles, p.t_col_tiles, p.t_grid};
    return PG_OK;
}

}  // extern "C"

// ---- observed reachability (observed.hpp) --------------------------------------------------------
namespace {
static_assert(sizeof(pg_reach_observed_result) == sizeof(ObservedResult), "pg_reach_observed_result is observed.hpp's ObservedResult");
static_assert(sizeof(pg_reach_observed_plan) == sizeof(ObservedPlan), "pg_reach_observed_plan is observed.hpp's ObservedPlan");
static_assert(PG_OBS_MATCHED == kObsMatched && PG_OBS_NO_SRC == kObsNoSrc && PG_OBS_NO_DST == kObsNoDst && PG_OBS_NO_SVC == kObsNoSvc &&
                  PG_OBSERVED_ACCUMULATE == kObsAccumulate && PG_OBSERVED_MATCH_SRC_PORT == kObsMatchSrcPort,
              "observed.hpp's constants are the header's");

int observed_shape(pg_ctx* ctx, size_t n_src, size_t n_dst, size_t n_svc) {
    if (!n_svc || n_svc > kObsMaxSvc) return fail(ctx, PG_EINVAL, "n_svc is 0 or above 4096");
    if (n_src > kObsMaxSide || n_dst > kObsMaxSide) return fail(ctx, PG_EINVAL, "a side longer than 2^20");
    return PG_OK;
}

// argument checks shared by pg_reach_observed and its host twin
int observed_args(pg_ctx* ctx, const pg_reach_observed_spec* spec, const pg_tuple_soa* flows, uint64_t n,
                  const uint32_t* out_packed, const pg_reach_observed_result* result) {
    if (!ctx) return PG_EINVAL;
    if (!spec || !result || !out_packed) return fail(ctx, PG_EINVAL, "null spec, result or out_packed");
    if (spec->flags & ~kObsFlagsAll) return fail(ctx, PG_EINVAL, "unknown flag bits");
    if (int rc = observed_shape(ctx, spec->n_src, spec->n_dst, spec->n_svc)) return rc;
    // (n_svc * n_src <= 2^32 and row_words <= 2^16: the product fits 64 bits)
    if ((uint64_t)spec->n_svc * spec->n_src * reach_row_words(spec->n_dst) >> 32)
        return fail(ctx, PG_EINVAL, "n_svc * n_src * row_words reaches 2^32");
    if ((spec->n_src && !spec->src_ip) || (spec->n_dst && !spec->dst_ip) || !spec->services)
        return fail(ctx, PG_EINVAL, "null src_ip, dst_ip or services");
    if (n && !flows) return fail(ctx, PG_EINVAL, "null flows");
    if (n && (!flows->src_ip || !flows->dst_ip || !flows->dst_port || !flows->proto))
        return fail(ctx, PG_EINVAL, "null flows src_ip, dst_ip, dst_port or proto");
    if (n && (spec->flags & kObsMatchSrcPort) && !flows->src_port)
        return fail(ctx, PG_EINVAL, "PG_OBSERVED_MATCH_SRC_PORT needs flows src_port");
    return PG_OK;
}

struct ObservedTables {
    ObservedSide src, dst;
    ObservedSvc svc;
    explicit ObservedTables(const pg_reach_observed_spec* spec)
        : src(observed_side(spec->src_ip, (uint32_t)spec->n_src)),
          dst(observed_side(spec->dst_ip, (uint32_t)spec->n_dst)),
          svc(observed_svc((uint32_t)spec->n_svc, (spec->flags & kObsMatchSrcPort) != 0,
                           [&](uint32_t v, uint32_t* p, uint32_t* sp, uint32_t* dp) {
                               const pg_service& s = spec->services[v];
                               *p = (uint32_t)s.protocol, *sp = s.src_port, *dp = s.dst_port;
                           })) {}
};

// an empty side: *result is zeroed whatever the flows were
void observed_finish(const pg_reach_observed_spec* spec, const ObservedResult& r, pg_reach_observed_result* result) {
    if (!spec->n_src || !spec->n_dst) *result = pg_reach_observed_result{0, 0, 0, 0, 0};
    else *result = pg_reach_observed_result{r.n_matched, r.n_no_src, r.n_no_dst, r.n_no_svc, r.n_cells};
}
}  // namespace

extern "C" {

int pg_reach_observed(pg_ctx* ctx, const pg_reach_observed_spec* spec, const pg_tuple_soa* flows, uint64_t n,
                      uint32_t* out_packed, uint8_t* out_flow, uint64_t* out_svc_flows, pg_reach_observed_result* result,
                      void* stream) {
    GUARD_BEGIN
    if (int rc = observed_args(ctx, spec, flows, n, out_packed, result)) return rc;
    DEVICE_GUARD(ctx);
    const ObservedTables T(spec);
    const Tuning& tu = ctx->eng.tune;
    const ObservedKnobs knobs{tu.blocks_per_cu, tu.observed_lds_bytes, tu.observed_test_first, tu.launch_max_tuples};
    ObservedSpecDev sd{&T.src, &T.dst, &T.svc, (uint32_t)spec->n_src, (uint32_t)spec->n_dst, (uint32_t)spec->n_svc, spec->flags,
                       nullptr, nullptr, nullptr, nullptr, nullptr, n};
    if (n) sd.f_src = flows->src_ip, sd.f_dst = flows->dst_ip, sd.f_sport = flows->src_port, sd.f_dport = flows->dst_port, sd.f_proto = flows->proto;
    std::string err;
    ObservedResult r{0, 0, 0, 0, 0};
    const int rc = dev_reach_observed(knobs, sd, out_packed, out_flow, out_svc_flows, &r, stream, &err);
    if (rc != 0) return fail(ctx, rc == -2 ? PG_ENOMEM : PG_EIO, err);
    observed_finish(spec, r, result);
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_observed_host(pg_ctx* ctx, const pg_reach_observed_spec* spec, const pg_tuple_soa* flows, uint64_t n,
                                 uint32_t* out_packed, uint8_t* out_flow, uint64_t* out_svc_flows,
                                 pg_reach_observed_result* result) {
    GUARD_BEGIN
    if (int rc = observed_args(ctx, spec, flows, n, out_packed, result)) return rc;
    const ObservedTables T(spec);
    const uint32_t nv = (uint32_t)spec->n_svc, rw = (uint32_t)reach_row_words(spec->n_dst);
    const uint64_t n_words = (uint64_t)nv * spec->n_src * rw;
    const bool sport = (spec->flags & kObsMatchSrcPort) != 0;
    if (!(spec->flags & kObsAccumulate)) std::fill(out_packed, out_packed + n_words, 0u);
    const ObsView<const uint32_t*> V{T.src.tab.data(), T.dst.tab.data(), T.src.idx.data(), T.dst.idx.data(), T.svc.keys.data(),
                                     T.svc.start.data(), T.svc.idx.data(), T.src.cap - 1u, T.dst.cap - 1u, T.svc.nk,
                                     (uint32_t)spec->n_src, rw, sport};
    // every flow in order, as a lane of k_observed runs it; the counts per key, then per service
    uint64_t status[4] = {0, 0, 0, 0};
    std::vector<uint64_t> kcnt(T.svc.nk, 0);
    for (uint64_t t = 0; t < n; t++) {
        uint32_t k = 0;
        const uint32_t st = obs_flow(V, flows->src_ip[t], flows->dst_ip[t], sport ? flows->src_port[t] : 0u, flows->dst_port[t],
                                     flows->proto[t], &k, [&](uint32_t w, uint32_t bit) { out_packed[w] |= bit; });
        if (st == kObsMatched) kcnt[k]++;
        status[st]++;
        if (out_flow) out_flow[t] = (uint8_t)st;
    }
    if (out_svc_flows) {
        std::fill(out_svc_flows, out_svc_flows + nv, (uint64_t)0);
        for (uint32_t k = 0; k < T.svc.nk; k++)
            for (uint32_t q = T.svc.start[k]; q < T.svc.start[k + 1]; q++) out_svc_flows[T.svc.idx[q]] = kcnt[k];
    }
    uint64_t cells = 0;
    for (uint64_t w = 0; w < n_words; w++) cells += obs_allow_cells(out_packed[w]);
    observed_finish(spec, ObservedResult{status[kObsMatched], status[kObsNoSrc], status[kObsNoDst], status[kObsNoSvc], cells}, result);
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_observed_plan(pg_ctx* ctx, size_t n_src, size_t n_dst, size_t n_svc, pg_reach_observed_plan* plan) {
    if (!ctx || !plan) return PG_EINVAL;
    GUARD_BEGIN
    if (int rc = observed_shape(ctx, n_src, n_dst, n_svc)) return rc;
    // (no DEVICE_GUARD: without a device the queries fail and the grid is their fall-back, the rest is host arithmetic)
    const pg::DeviceGuard guard(ctx);
    const ObservedPlan p = dev_observed_plan((uint32_t)n_src, (uint32_t)n_dst, (uint32_t)n_svc, ctx->eng.tune.observed_lds_bytes,
                                             ctx->eng.tune.blocks_per_cu);
    *plan = pg_reach_observed_plan{p.src_cap, p.dst_cap, p.src_in_lds, p.dst_in_lds, p.svc_bytes, p.lds_bytes, p.block, p.vec_flows, p.grid};
    return PG_OK;
    GUARD_END(ctx)
}

int pg_debug_reach_observed_probe(pg_ctx* ctx, const uint32_t* list, size_t n_list, const uint32_t* ips, uint64_t n,
                                  uint32_t* out_steps, uint32_t* out_slot, uint32_t* out_cap) {
    if (!ctx) return PG_EINVAL;
    GUARD_BEGIN
    if (n_list > kObsMaxSide) return fail(ctx, PG_EINVAL, "a list longer than 2^20");
    if ((n_list && !list) || (n && !ips)) return fail(ctx, PG_EINVAL, "null list or ips");
    const ObservedSide s = observed_side(list, (uint32_t)n_list);
    if (out_cap) *out_cap = s.cap;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t first = 0, count = 0, steps = 0;
        (void)obs_find(s.tab.data(), s.cap - 1u, ips[i], &first, &count, &steps);
        if (out_steps) out_steps[i] = steps;
        if (out_slot) out_slot[i] = obs_hash(ips[i], s.cap - 1u);
    }
    return PG_OK;
    GUARD_END(ctx)
}

}  // extern "C"
