// gfx950 kernels of the reachability matrix (pg_reach_matrix; reach.hpp has the shared code and
// what each form hoists).
//
//  k_reach_ends   prologue, one lane per end point (src then dst): form A the IPv4 class walk over
//                 the node image (read from global memory, as the STAGE 0 classify launches do),
//                 form B the iphash probe
//  k_reach_svcs   prologue, one lane per service: form A the two key-class walks, form B the keys
//  k_reach_pairs  one lane per output word (16 dst of one (service, src)), grid-stride over the
//                 64-bit word count: four rounds of Q = 4 pairs, the 2-bit codes ORed in a
//                 register, one 4-B store. Adjacent lanes take adjacent src of the same 16 dst: a
//                 lane's own values (its src record and class) are one coalesced load per word,
//                 and the dst values of a round are the same addresses in every lane of the wave
//                 -- the other order (adjacent lanes on adjacent words of one row) made every dst
//                 load a 64-line gather and took 1.28 times as long per call. The
//                 full words, when asked for, as 16-B vectors where a row's words are 16-B aligned
//  k_ports_pairs  the port sweep (pg_reach_ports; ports.hpp): one lane per pair, grid-stride; the
//                 interval loop innermost, so a pair's src and dst values are loaded once for all K
//                 intervals. Adjacent lanes take adjacent dst of one src -- the opposite of
//                 k_reach_pairs, because here a lane's output (row_words(K) code words, the open
//                 count, K full words) is contiguous per pair: the dst values and the out_open
//                 stores are coalesced, the out_codes stores too when K <= 16, and the src values
//                 are one or two addresses per wave. The per-interval values are indexed by the
//                 loop counter alone and arrive by scalar loads (the arrays are __restrict__
//                 kernel arguments of their own for that). Prologues: k_reach_ends, k_reach_svcs
//  k_rules_pairs  rule coverage (pg_reach_rules; rules.hpp): k_reach_pairs's word index space and
//                 lane order, but nothing stored per cell -- a workgroup of four waves counts every
//                 evaluation and every final word, times the service's weight, into two windows of
//                 u32 cells in LDS and flushes them to the u64 outputs with global atomics at the
//                 end of its run and whenever the plan's wrap bound is reached. Indices past a
//                 window go to the outputs at once, aggregated per distinct index over the wave.
//                 Prologues: k_reach_ends, k_reach_svcs
//
// No kernel takes or touches a hit counter (k_rules_pairs counts into the caller's arrays).
//
// The three drivers are four steps: stage the inputs in one scratch block (Staged), run each form's
// prologue (run_prologue; run_forms for the matrix and the rules), launch its pair kernel
// (with_words_vec, grid_resident), Scratch::finish.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include "audit_launch.hpp"
#include "ports.hpp"
#include "reach.hpp"
#include "rules.hpp"

namespace pg {

namespace {

constexpr int kReachBlock = 256;
// the pair kernel's workgroup is one wave: nothing in it is shared by a workgroup, and the grid of
// resident workgroups then follows the occupancy in steps of 64 lanes
constexpr int kReachPairBlock = 64;

template <bool UNI>
__global__ __launch_bounds__(kReachBlock) void k_reach_ends(DevTableSet T, const uint32_t* __restrict__ ip, uint32_t n,
                                                            W4* __restrict__ rec, uint32_t* __restrict__ cls) {
    const uint32_t i = blockIdx.x * kReachBlock + threadIdx.x;
    if (i >= n) return;
    W4 r;
    if constexpr (UNI) {
        uint32_t c;
        reach_end_uni(T.node, DevLoader{T.node.img}, ip[i], &r, &c);
        cls[i] = c;
    } else {
        r = reach_end_tab(T, ip[i]);
    }
    *reinterpret_cast<uint4*>(rec + i) = make_uint4(r.x, r.y, r.z, r.w);
}

template <bool UNI>
__global__ __launch_bounds__(kReachBlock) void k_reach_svcs(DevTableSet T, const W4* __restrict__ svc,
                                                            const uint32_t* __restrict__ list, uint32_t n_list,
                                                            W2* __restrict__ out) {
    const uint32_t k = blockIdx.x * kReachBlock + threadIdx.x;
    if (k >= n_list) return;
    const uint32_t v = list[k];
    const uint4 q = *reinterpret_cast<const uint4*>(svc + v);
    const W4 s{q.x, q.y, q.z, q.w};
    W2 g;
    if constexpr (UNI) g = reach_svc_uni(T.node, DevLoader{T.node.img}, s);
    else g = reach_svc_tab(s);
    *reinterpret_cast<uint2*>(out + v) = make_uint2(g.x, g.y);
}

// The full verdict words of one round of Q = 4, the first `valid` of them, to base[at ...]; nothing
// without WORDS (base is null then). VEC: base + at is 16-B aligned and every round is whole
template <bool WORDS, bool VEC>
__device__ __forceinline__ void store_round(uint32_t* base, uint32_t at, const uint32_t (&o)[kReachQ], uint32_t valid) {
    if constexpr (WORDS) {
        uint32_t* p = base + at;
        if (VEC) {
            *reinterpret_cast<uint4*>(p) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (uint32_t q = 0; q < kReachQ; q++)
                if (q < valid) p[q] = o[q];
        }
    }
}

// VEC: every row of out_words starts 16-B aligned (n_dst a multiple of 4, the array 16-B aligned)
template <bool UNI, bool WIDE, bool WORDS, bool VEC>
__global__ __launch_bounds__(kReachPairBlock) void k_reach_pairs(DevTableSet T, ReachPass P, uint64_t n_words) {
    const uint32_t rw = (uint32_t)reach_row_words(P.n_dst);
    const uint64_t per_svc = (uint64_t)rw * P.n_src;
    const uint64_t step = (uint64_t)gridDim.x * kReachPairBlock;
    for (uint64_t w = (uint64_t)blockIdx.x * kReachPairBlock + threadIdx.x; w < n_words; w += step) {
        // lanes run over the src of one (service, 16 dst): w = (k * row_words + jw) * n_src + i
        uint32_t k, i, jw;
        if (n_words >> 32) {  // (uniform) 64-bit word indices; 32-bit divisions otherwise
            k = (uint32_t)(w / per_svc);
            const uint64_t rem = w - (uint64_t)k * per_svc;
            jw = (uint32_t)(rem / P.n_src), i = (uint32_t)(rem - (uint64_t)jw * P.n_src);
        } else {
            const uint32_t w32 = (uint32_t)w, ps = (uint32_t)per_svc;
            k = w32 / ps;
            const uint32_t rem = w32 - k * ps;
            jw = rem / P.n_src, i = rem - jw * P.n_src;
        }
        const uint32_t v = P.svc_list[k];
        const uint64_t row = (uint64_t)v * P.n_src + i;
        const uint32_t j0 = jw * kReachWordPairs;
        const uint2 gq = *reinterpret_cast<const uint2*>(P.svc + v);
        const W2 g{gq.x, gq.y};
        const uint4 sq = *reinterpret_cast<const uint4*>(P.rec_s + i);
        const W4 rs{sq.x, sq.y, sq.z, sq.w};
        uint32_t* ow = WORDS ? P.out_words + row * P.n_dst + j0 : nullptr;
        auto emit = [&](uint32_t r, const uint32_t(&o)[kReachQ], uint32_t valid) {
            store_round<WORDS, VEC>(ow, r * kReachQ, o, valid);
        };
        uint32_t packed;
        if constexpr (UNI)
            packed = reach_word_uni<WIDE>(T, T.node, DevLoader{T.node.img}, rs, P.cls_s[i], P.rec_d, P.cls_d, j0, P.n_dst,
                                          g, emit);
        else
            packed = reach_word_tab(T, rs, P.rec_d, j0, P.n_dst, g, emit);
        P.out_packed[row * rw + jw] = packed;
    }
}

// the port sweep (ports.hpp). VEC: every pair's K words start 16-B aligned (K a multiple of 4, the
// array 16-B aligned)
template <bool UNI, bool WIDE, bool WORDS, bool VEC>
__global__ __launch_bounds__(kReachPairBlock) void k_ports_pairs(DevTableSet T, ReachEnds E, const W2* __restrict__ iv,
                                                                 const uint32_t* __restrict__ len, uint32_t K,
                                                                 uint32_t n_pairs, uint32_t* __restrict__ out_codes,
                                                                 uint32_t* __restrict__ out_open,
                                                                 uint32_t* __restrict__ out_words) {
    const uint32_t rw = (uint32_t)reach_row_words(K);
    const uint64_t step = (uint64_t)gridDim.x * kReachPairBlock;
    // n_pairs * rw < 2^32 (the host checks), so a pair and its code words index in 32 bits
    for (uint64_t p64 = (uint64_t)blockIdx.x * kReachPairBlock + threadIdx.x; p64 < n_pairs; p64 += step) {
        const uint32_t p = (uint32_t)p64, i = p / E.n_dst, j = p - i * E.n_dst;
        const uint4 sq = *reinterpret_cast<const uint4*>(E.rec_s + i);
        const uint4 dq = *reinterpret_cast<const uint4*>(E.rec_d + j);
        const W4 rs{sq.x, sq.y, sq.z, sq.w}, rd{dq.x, dq.y, dq.z, dq.w};
        uint32_t* oc = out_codes + p * rw;
        uint32_t* ow = WORDS ? out_words + (uint64_t)p * K : nullptr;
        auto emit_code = [&](uint32_t w, uint32_t word) { oc[w] = word; };
        auto emit_words = [&](uint32_t k0, const uint32_t(&o)[kReachQ], uint32_t valid) {
            store_round<WORDS, VEC>(ow, k0, o, valid);
        };
        uint32_t open;
        if constexpr (UNI)
            open = ports_pair_uni<WIDE>(T, T.node, DevLoader{T.node.img}, rs, E.cls_s[i], rd, E.cls_d[j], iv, len, K,
                                        emit_code, emit_words);
        else
            open = ports_pair_tab(T, rs, rd, iv, len, K, emit_code, emit_words);
        if (out_open) out_open[p] = open;
    }
}

// rule coverage (rules.hpp): a workgroup's window cells to the output array, the cells cleared.
// Between two barriers: no lane counts while another reads and clears
__device__ __forceinline__ void rules_flush(uint32_t* win, const RulesWindow& w, uint32_t n, unsigned long long* out) {
    for (uint32_t c = threadIdx.x; c < w.cells; c += kRulesBlock) {
        const uint32_t v = win[c];
        if (v) {
            atomicAdd(&out[rules_index_of_cell(w, n, c)], (unsigned long long)v);
            win[c] = 0;
        }
    }
}

// Every workgroup makes the same rounds of kRulesBlock words (a lane past n_words idles), so the
// barriers of a flush are uniform. `since` counts whole rounds: a flush comes before the round that
// could take the words since the last one past A.flush_words (rules_plan: no cell can wrap before)
template <bool UNI, bool WIDE, bool EVALS, bool CELLS, bool AGG>
__global__ __launch_bounds__(kRulesBlock) void k_rules_pairs(DevTableSet T, ReachPass P, RulesArgs A, uint64_t n_words) {
    extern __shared__ uint32_t rules_win[];  // [evals cells | cells cells]
    uint32_t *we = rules_win, *wc = rules_win + A.evals.cells;
    for (uint32_t c = threadIdx.x; c < A.evals.cells + A.cells.cells; c += kRulesBlock) rules_win[c] = 0;
    __syncthreads();
    const uint32_t rw = (uint32_t)reach_row_words(P.n_dst);
    const uint64_t step = (uint64_t)gridDim.x * kRulesBlock;
    uint32_t since = 0;
    for (uint64_t w0 = (uint64_t)blockIdx.x * kRulesBlock; w0 < n_words; w0 += step) {
        if (since + kRulesBlock > A.flush_words) {
            __syncthreads();
            if (EVALS) rules_flush(we, A.evals, A.n_slots, A.out_evals);
            if (CELLS) rules_flush(wc, A.cells, 4u * A.n_slots, A.out_cells);
            __syncthreads();
            since = 0;
        }
        since += kRulesBlock;
        const uint64_t w = w0 + threadIdx.x;
        if (w >= n_words) continue;
        const RulesWord x = rules_word_of(w, n_words, rw, P.n_src);
        const uint32_t v = P.svc_list[x.k], j0 = x.jw * kReachWordPairs, wgt = A.weight[v];
        const uint2 gq = *reinterpret_cast<const uint2*>(P.svc + v);
        const W2 g{gq.x, gq.y};
        const uint4 sq = *reinterpret_cast<const uint4*>(P.rec_s + x.i);
        const W4 rs{sq.x, sq.y, sq.z, sq.w};
        const RulesSink<AGG> se{we, A.out_evals, A.evals, A.n_slots, wgt, nullptr};
        const RulesSink<AGG> sc{wc, A.out_cells, A.cells, 4u * A.n_slots, wgt, nullptr};
        if constexpr (UNI)
            rules_word_uni<WIDE, EVALS, CELLS>(T, T.node, DevLoader{T.node.img}, rs, P.cls_s[x.i], P.rec_d, P.cls_d, j0, P.n_dst,
                                               g, se, sc);
        else
            rules_word_tab<EVALS, CELLS>(T, rs, P.rec_d, j0, P.n_dst, g, se, sc);
    }
    __syncthreads();
    if (EVALS) rules_flush(we, A.evals, A.n_slots, A.out_evals);
    if (CELLS) rules_flush(wc, A.cells, 4u * A.n_slots, A.out_cells);
}

// ---- what the drivers are made of --------------------------------------------------------------------
// the prologue of one form: rec (and cls, form A) of the ne end points, g of the n services in list
template <bool UNI>
void run_prologue(const DevTableSet& T, const uint32_t* ip, uint32_t ne, const W4* svc, const uint32_t* list, uint32_t n,
                  W4* rec, uint32_t* cls, W2* g, hipStream_t st) {
    hipLaunchKernelGGL(k_reach_ends<UNI>, dim3((ne + kReachBlock - 1) / kReachBlock), dim3(kReachBlock), 0, st, T, ip, ne,
                       rec, cls);
    hipLaunchKernelGGL(k_reach_svcs<UNI>, dim3((n + kReachBlock - 1) / kReachBlock), dim3(kReachBlock), 0, st, T, svc, list,
                       n, g);
}

// f(WORDS, VEC) as two std::integral_constant<bool>: a pair kernel's last two template arguments,
// from whether the full words are asked for and whether they can go out as 16-B vectors
template <class F>
void with_words_vec(bool words, bool vec, const F& f) {
    if (!words) f(std::false_type{}, std::false_type{});
    else if (vec) f(std::true_type{}, std::true_type{});
    else f(std::true_type{}, std::false_type{});
}

// The inputs of a call, staged. The block is [ip of src ++ dst | list | extra | cls | svc | rec | end | g]:
// the host fills it up to svc and copies that prefix in with one synchronous copy (cls, which the
// kernels fill, goes over as zeros); rec are form A's records, end form B's ends.
struct Staged {
    Scratch blk;
    uint32_t ns, nd;
    const uint32_t *ip, *list, *extra;
    const W4* svc;
    uint32_t* cls;
    W4 *rec, *end;
    W2* g;
    // list: the ordered services, at most n_svc; extra: one u32 per service, or null; with_end: room for end
    int make(const ReachSpecDev& s, const std::vector<uint32_t>& list_h, const uint32_t* extra_h, bool with_end, std::string* err) {
        ns = s.n_src, nd = s.n_dst;
        const size_t ne = (size_t)ns + nd, nv = s.n_svc;
        enum { IP, LIST, EXTRA, CLS, SVC, REC, END, G };
        const auto l = lay_out({4u * ne, 4u * nv, extra_h ? 4u * nv : 0u, 4u * ne, 16u * nv, 16u * ne, with_end ? 16u * ne : 0u,
                                8u * nv});
        std::vector<unsigned char> h(l.off[SVC] + 16u * nv, 0);  // the copied prefix
        l.put(h, IP, IP, s.src_ip, ns), std::copy_n(s.dst_ip, nd, l.in<uint32_t>(h, IP, IP) + ns);
        l.put(h, IP, LIST, list_h), l.put(h, IP, EXTRA, extra_h, extra_h ? nv : 0u), l.put(h, IP, SVC, s.services, nv);
        if (Scratch::make(&blk, l.total, err) != 0) return -1;
        HIPCHK(hipMemcpy(blk.at<unsigned char>(0), h.data(), h.size(), hipMemcpyHostToDevice));
        ip = l.at<uint32_t>(blk, IP), list = l.at<uint32_t>(blk, LIST), extra = l.at<uint32_t>(blk, EXTRA);
        cls = l.at<uint32_t>(blk, CLS), svc = l.at<W4>(blk, SVC);
        rec = l.at<W4>(blk, REC), end = l.at<W4>(blk, END), g = l.at<W2>(blk, G);
        return 0;
    }
};

// The passes of a call whose list is [na form-A services | nb form-B services]: each form's prologue,
// then launch(uni, wide, the pass without outputs, its words) for the caller's pair kernel
template <class F>
void run_forms(const DevTableSet& T, const Staged& in, uint32_t na, uint32_t nb, hipStream_t st, const F& launch) {
    // one form: its n services lst, its end-point records r and (form A) classes c
    auto pass = [&](auto uni, auto wide, const uint32_t* lst, uint32_t n, W4* r, uint32_t* c) {
        run_prologue<decltype(uni)::value>(T, in.ip, in.ns + in.nd, in.svc, lst, n, r, c, in.g, st);
        launch(uni, wide, ReachPass{{r, r + in.ns, c, c ? c + in.ns : nullptr, in.ns, in.nd}, in.g, lst, n, nullptr, nullptr},
               (uint64_t)n * in.ns * reach_row_words(in.nd));
    };
    if (na && T.node.wide) pass(std::true_type{}, std::true_type{}, in.list, na, in.rec, in.cls);
    else if (na) pass(std::true_type{}, std::false_type{}, in.list, na, in.rec, in.cls);
    if (nb) pass(std::false_type{}, std::false_type{}, in.list + na, nb, in.end, nullptr);
}

}  // namespace

int dev_reach_matrix(const DevTableSet& T, const Tuning& tu, const ReachSpecDev& spec, uint32_t* out_packed,
                     uint32_t* out_words, void* stream, std::string* err) {
    const uint32_t ns = spec.n_src, nd = spec.n_dst, nv = spec.n_svc;
    if (!ns || !nd || !nv) return 0;
    hipStream_t st = (hipStream_t)stream;
    std::vector<uint32_t> list;
    const uint32_t na = reach_form_split(reach_form_a(T.node, tu), spec.services, nv, nullptr, &list);
    Staged in;
    if (in.make(spec, list, nullptr, true, err) != 0) return -1;
    run_forms(T, in, na, nv - na, st, [&](auto uni, auto wide, ReachPass P, uint64_t n_words) {
        P.out_packed = out_packed, P.out_words = out_words;
        const bool vec = nd % 4u == 0 && ((uintptr_t)out_words & 15u) == 0;
        with_words_vec(out_words != nullptr, vec, [&](auto words, auto v16) {
            auto k = k_reach_pairs<decltype(uni)::value, decltype(wide)::value, decltype(words)::value, decltype(v16)::value>;
            hipLaunchKernelGGL(k, dim3(grid_resident(k, kReachPairBlock, 0, n_words, tu.blocks_per_cu)),
                               dim3(kReachPairBlock), 0, st, T, P, n_words);
        });
    });
    HIPCHK(hipGetLastError());
    return in.blk.finish(st, "reach matrix", err);
}

int dev_reach_ports(const DevTableSet& T, const Tuning& tu, const PortsSpecDev& spec, uint32_t* out_codes,
                    uint32_t* out_open, uint32_t* out_words, void* stream, std::string* err) {
    const uint32_t ns = spec.n_src, nd = spec.n_dst, K = spec.K;
    if (!ns || !nd || !K) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool form_a = reach_form_a(T.node, tu);  // (TCP / UDP: every interval takes the same form)
    // the intervals as services, all in one pass, and their lengths
    std::vector<uint32_t> list(K), lens(K);
    std::vector<W4> svc(K);
    for (uint32_t k = 0; k < K; k++) {
        list[k] = k, lens[k] = ports_len(spec.lo, K, k);
        svc[k] = reach_service((int32_t)spec.protocol, spec.src_port, spec.lo[k]);
    }
    Staged in;
    if (in.make(ReachSpecDev{spec.src_ip, spec.dst_ip, svc.data(), ns, nd, K}, list, lens.data(), false, err) != 0) return -1;
    uint32_t* cls = form_a ? in.cls : nullptr;
    const ReachEnds E{in.rec, in.rec + ns, cls, form_a ? cls + ns : nullptr, ns, nd};
    auto pairs = [&](auto uni, auto wide) {
        run_prologue<decltype(uni)::value>(T, in.ip, ns + nd, in.svc, in.list, K, in.rec, cls, in.g, st);
        const bool vec = K % 4u == 0 && ((uintptr_t)out_words & 15u) == 0;
        with_words_vec(out_words != nullptr, vec, [&](auto words, auto v16) {
            auto k = k_ports_pairs<decltype(uni)::value, decltype(wide)::value, decltype(words)::value, decltype(v16)::value>;
            hipLaunchKernelGGL(k, dim3(grid_resident(k, kReachPairBlock, 0, ns * nd, tu.blocks_per_cu)),
                               dim3(kReachPairBlock), 0, st, T, E, in.g, in.extra, K, ns * nd, out_codes, out_open, out_words);
        });
    };
    if (!form_a) pairs(std::false_type{}, std::false_type{});
    else if (T.node.wide) pairs(std::true_type{}, std::true_type{});
    else pairs(std::true_type{}, std::false_type{});
    HIPCHK(hipGetLastError());
    return in.blk.finish(st, "port sweep", err);
}

namespace {
// f(k_rules_pairs<UNI, WIDE, EVALS, CELLS, AGG>) for the histograms asked for and the "rules_wave_agg" knob
template <bool UNI, bool WIDE, class F>
void with_rules_kernel(bool evals, bool cells, bool agg, const F& f) {
    auto pick = [&](auto ev, auto ce) {
        if (agg) f(k_rules_pairs<UNI, WIDE, decltype(ev)::value, decltype(ce)::value, true>);
        else f(k_rules_pairs<UNI, WIDE, decltype(ev)::value, decltype(ce)::value, false>);
    };
    if (evals && cells) pick(std::true_type{}, std::true_type{});
    else if (evals) pick(std::true_type{}, std::false_type{});
    else pick(std::false_type{}, std::true_type{});
}
}  // namespace

int dev_rules_resident(const Tuning& tu, uint32_t lds_bytes) {
    auto k = k_rules_pairs<false, false, true, true, true>;
    (void)allow_dynamic_lds(k, lds_bytes);
    const int g = grid_resident(k, (int)kRulesBlock, lds_bytes, ~(uint64_t)0 >> 1, tu.blocks_per_cu);
    (void)hipGetLastError();  // (a failed occupancy query is answered by grid_resident's fall-back)
    return g;
}

int dev_reach_rules(const DevTableSet& T, const Tuning& tu, const RulesSpecDev& spec, unsigned long long* out_evals,
                    unsigned long long* out_cells, std::vector<uint64_t>* evals_host, void* stream, std::string* err) {
    const ReachSpecDev& rs = spec.reach;
    const uint32_t ns = rs.n_src, nd = rs.n_dst, nv = rs.n_svc, n_slots = spec.n_slots;
    hipStream_t st = (hipStream_t)stream;
    if (out_evals) HIPCHK(hipMemsetAsync(out_evals, 0, (size_t)n_slots * sizeof(uint64_t), st));
    if (out_cells) HIPCHK(hipMemsetAsync(out_cells, 0, 4u * (size_t)n_slots * sizeof(uint64_t), st));
    auto read_back = [&]() -> int {
        if (!out_evals || !evals_host) return 0;
        evals_host->assign(n_slots, 0);
        HIPCHK(hipMemcpy(evals_host->data(), out_evals, (size_t)n_slots * sizeof(uint64_t), hipMemcpyDeviceToHost));
        return 0;
    };
    if (!ns || !nd || !nv) {
        HIPCHK(hipStreamSynchronize(st));
        return read_back();
    }
    // (the services that weigh anything)
    std::vector<uint32_t> list;
    const uint32_t na = reach_form_split(reach_form_a(T.node, tu), rs.services, nv, spec.weight, &list);
    if (list.empty()) {
        HIPCHK(hipStreamSynchronize(st));
        return read_back();
    }
    Staged in;
    if (in.make(rs, list, spec.weight, true, err) != 0) return -1;
    const RulesPlan plan = rules_plan(n_slots, spec.n_tail, out_evals != nullptr, out_cells != nullptr, tu.rules_hist_cells,
                                      spec.max_weight);
    const RulesArgs A{in.extra, out_evals, out_cells, plan.evals, plan.cells, n_slots, plan.flush_words};
    int rc = 0;
    run_forms(T, in, na, (uint32_t)list.size() - na, st, [&](auto uni, auto wide, const ReachPass& P, uint64_t n_words) {
        with_rules_kernel<decltype(uni)::value, decltype(wide)::value>(
            out_evals != nullptr, out_cells != nullptr, tu.rules_wave_agg != 0, [&](auto k) {
                if (allow_dynamic_lds(k, plan.lds_bytes) != hipSuccess) rc = -1;
                const int grid = grid_resident(k, (int)kRulesBlock, plan.lds_bytes, n_words, tu.blocks_per_cu);
                (void)hipGetLastError();  // (a failed occupancy query is answered by grid_resident's fall-back)
                if (rc == 0) hipLaunchKernelGGL(k, dim3(grid), dim3(kRulesBlock), plan.lds_bytes, st, T, P, A, n_words);
            });
    });
    if (rc != 0) {
        if (err) *err = "rule coverage: the LDS window was refused";
        return -1;
    }
    HIPCHK(hipGetLastError());
    if (in.blk.finish(st, "rule coverage", err) != 0) return -1;
    return read_back();
}

}  // namespace pg
