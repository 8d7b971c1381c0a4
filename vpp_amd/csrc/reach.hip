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
//
// No kernel takes or touches a hit counter.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ports.hpp"
#include "reach.hpp"

namespace pg {

namespace {

constexpr int kReachBlock = 256;
// the pair kernel's workgroup is one wave: nothing in it is shared by a workgroup, and the grid of
// resident workgroups then follows the occupancy in steps of 64 lanes
constexpr int kReachPairBlock = 64;

#define REACH_CHK(expr)                                                      \
    do {                                                                     \
        hipError_t e_ = (expr);                                              \
        if (e_ != hipSuccess) {                                              \
            if (err) *err = std::string(#expr ": ") + hipGetErrorString(e_); \
            return -1;                                                       \
        }                                                                    \
    } while (0)

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
            if constexpr (WORDS) {
                uint32_t* p = ow + r * kReachQ;
                if (VEC) {  // (n_dst a multiple of 4: every round is whole)
                    *reinterpret_cast<uint4*>(p) = make_uint4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (uint32_t q = 0; q < kReachQ; q++)
                        if (q < valid) p[q] = o[q];
                }
            }
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

uint32_t reach_cus() {
    int dev = 0;
    hipDeviceProp_t p;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess || p.multiProcessorCount < 1)
        return 256;
    return (uint32_t)p.multiProcessorCount;
}

// the workgroups resident at once (capped by the work and by blocks_per_cu when set), like the
// classify launches
template <class K>
int reach_grid(K kernel, uint64_t items, uint32_t blocks_per_cu, uint32_t cus) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kReachPairBlock, 0) != hipSuccess || per_cu < 1)
        per_cu = 1;
    if (blocks_per_cu) per_cu = std::min<int>(per_cu, (int)blocks_per_cu);
    const uint64_t g = (items + kReachPairBlock - 1) / kReachPairBlock;
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(g, (uint64_t)cus * per_cu));
}

template <bool UNI, bool WIDE, bool WORDS, bool VEC>
void launch_pairs(const DevTableSet& T, const ReachPass& P, uint64_t n_words, uint32_t bpc, uint32_t cus,
                  hipStream_t st) {
    auto k = k_reach_pairs<UNI, WIDE, WORDS, VEC>;
    hipLaunchKernelGGL(k, dim3(reach_grid(k, n_words, bpc, cus)), dim3(kReachPairBlock), 0, st, T, P, n_words);
}
template <bool UNI, bool WIDE>
void launch_pairs(const DevTableSet& T, const ReachPass& P, uint64_t n_words, uint32_t bpc, uint32_t cus,
                  hipStream_t st) {
    const bool vec = P.n_dst % 4u == 0 && ((uintptr_t)P.out_words & 15u) == 0;
    if (!P.out_words) launch_pairs<UNI, WIDE, false, false>(T, P, n_words, bpc, cus, st);
    else if (vec) launch_pairs<UNI, WIDE, true, true>(T, P, n_words, bpc, cus, st);
    else launch_pairs<UNI, WIDE, true, false>(T, P, n_words, bpc, cus, st);
}

}  // namespace

int dev_reach_matrix(const DevTableSet& T, const Tuning& tu, const ReachSpecDev& spec, uint32_t* out_packed,
                     uint32_t* out_words, void* stream, std::string* err) {
    const uint32_t ns = spec.n_src, nd = spec.n_dst, nv = spec.n_svc, ne = ns + nd;
    if (!ns || !nd || !nv) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool form_a = reach_form_a(T.node, tu);
    // the services of each form (the host partitions them): list = [form A ..., form B ...]
    std::vector<uint32_t> list;
    for (uint32_t v = 0; v < nv; v++)
        if (form_a && spec.services[v].x <= 2u) list.push_back(v);
    const uint32_t na = (uint32_t)list.size(), nb = nv - na;
    for (uint32_t v = 0; v < nv; v++)
        if (!(form_a && spec.services[v].x <= 2u)) list.push_back(v);
    // one scratch block: [ip u32[ne] | list u32[nv] | cls u32[ne]] (padded to 16 B) | svc W4[nv] |
    // rec W4[ne] (form A) | end W4[ne] (form B) | g W2[nv]
    auto pad = [](size_t b) { return (b + 15u) & ~(size_t)15u; };
    const size_t o_ip = 0, o_list = pad(o_ip + 4u * (size_t)ne), o_cls = pad(o_list + 4u * (size_t)nv);
    const size_t o_svc = pad(o_cls + 4u * (size_t)ne), o_rec = o_svc + 16u * (size_t)nv;
    const size_t o_end = o_rec + 16u * (size_t)ne, o_g = o_end + 16u * (size_t)ne, total = o_g + 8u * (size_t)nv;
    // the host arrays go in as one copy: [ip | list | (cls, not copied) | svc]
    std::vector<unsigned char> h(o_rec, 0);
    std::copy(spec.src_ip, spec.src_ip + ns, reinterpret_cast<uint32_t*>(h.data() + o_ip));
    std::copy(spec.dst_ip, spec.dst_ip + nd, reinterpret_cast<uint32_t*>(h.data() + o_ip) + ns);
    std::copy(list.begin(), list.end(), reinterpret_cast<uint32_t*>(h.data() + o_list));
    std::copy(spec.services, spec.services + nv, reinterpret_cast<W4*>(h.data() + o_svc));
    unsigned char* d = nullptr;
    REACH_CHK(hipMalloc(&d, total));
    auto run = [&]() -> int {
        REACH_CHK(hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice));
        const uint32_t* ip = reinterpret_cast<const uint32_t*>(d + o_ip);
        const uint32_t* dl = reinterpret_cast<const uint32_t*>(d + o_list);
        uint32_t* cls = reinterpret_cast<uint32_t*>(d + o_cls);
        const W4* svc = reinterpret_cast<const W4*>(d + o_svc);
        W4* rec = reinterpret_cast<W4*>(d + o_rec);
        W4* end = reinterpret_cast<W4*>(d + o_end);
        W2* g = reinterpret_cast<W2*>(d + o_g);
        const uint32_t cus = reach_cus();
        const unsigned ge = (ne + kReachBlock - 1) / kReachBlock;
        const uint64_t row_words = reach_row_words(nd);
        if (na) {
            hipLaunchKernelGGL(k_reach_ends<true>, dim3(ge), dim3(kReachBlock), 0, st, T, ip, ne, rec, cls);
            hipLaunchKernelGGL(k_reach_svcs<true>, dim3((na + kReachBlock - 1) / kReachBlock), dim3(kReachBlock), 0, st,
                               T, svc, dl, na, g);
            const ReachPass P{rec, rec + ns, cls, cls + ns, g, dl, na, ns, nd, out_packed, out_words};
            const uint64_t n_words = (uint64_t)na * ns * row_words;
            if (T.node.wide) launch_pairs<true, true>(T, P, n_words, tu.blocks_per_cu, cus, st);
            else launch_pairs<true, false>(T, P, n_words, tu.blocks_per_cu, cus, st);
        }
        if (nb) {
            hipLaunchKernelGGL(k_reach_ends<false>, dim3(ge), dim3(kReachBlock), 0, st, T, ip, ne, end, nullptr);
            hipLaunchKernelGGL(k_reach_svcs<false>, dim3((nb + kReachBlock - 1) / kReachBlock), dim3(kReachBlock), 0, st,
                               T, svc, dl + na, nb, g);
            const ReachPass P{end, end + ns, nullptr, nullptr, g, dl + na, nb, ns, nd, out_packed, out_words};
            launch_pairs<false, false>(T, P, (uint64_t)nb * ns * row_words, tu.blocks_per_cu, cus, st);
        }
        REACH_CHK(hipGetLastError());
        return 0;
    };
    const int rc = run();
    // the kernels have read the scratch block before it is released
    const hipError_t es = hipStreamSynchronize(st);
    (void)hipFree(d);
    if (rc == 0 && es != hipSuccess) {
        if (err) *err = std::string("reach matrix: ") + hipGetErrorString(es);
        return -1;
    }
    return rc;
}

// ---- port sweep (ports.hpp) ----------------------------------------------------------------------
namespace {

// the hoisted end-point arrays of one form (ReachPass's first four)
struct PortsEnds {
    const W4* rec_s;
    const W4* rec_d;
    const uint32_t* cls_s;
    const uint32_t* cls_d;
    uint32_t n_dst;
};

// VEC: every pair's K words start 16-B aligned (K a multiple of 4, the array 16-B aligned)
template <bool UNI, bool WIDE, bool WORDS, bool VEC>
__global__ __launch_bounds__(kReachPairBlock) void k_ports_pairs(DevTableSet T, PortsEnds E, const W2* __restrict__ iv,
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
            if constexpr (WORDS) {
                uint32_t* q4 = ow + k0;
                if (VEC) {  // (K a multiple of 4: every round is whole)
                    *reinterpret_cast<uint4*>(q4) = make_uint4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (uint32_t q = 0; q < kReachQ; q++)
                        if (q < valid) q4[q] = o[q];
                }
            }
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

template <bool UNI, bool WIDE, bool WORDS, bool VEC>
void launch_ports(const DevTableSet& T, const PortsEnds& E, const W2* iv, const uint32_t* len, uint32_t K,
                  uint32_t n_pairs, uint32_t* codes, uint32_t* open, uint32_t* words, uint32_t bpc, uint32_t cus,
                  hipStream_t st) {
    auto k = k_ports_pairs<UNI, WIDE, WORDS, VEC>;
    hipLaunchKernelGGL(k, dim3(reach_grid(k, n_pairs, bpc, cus)), dim3(kReachPairBlock), 0, st, T, E, iv, len, K, n_pairs,
                       codes, open, words);
}
template <bool UNI, bool WIDE>
void launch_ports(const DevTableSet& T, const PortsEnds& E, const W2* iv, const uint32_t* len, uint32_t K,
                  uint32_t n_pairs, uint32_t* codes, uint32_t* open, uint32_t* words, uint32_t bpc, uint32_t cus,
                  hipStream_t st) {
    const bool vec = K % 4u == 0 && ((uintptr_t)words & 15u) == 0;
    if (!words) launch_ports<UNI, WIDE, false, false>(T, E, iv, len, K, n_pairs, codes, open, words, bpc, cus, st);
    else if (vec) launch_ports<UNI, WIDE, true, true>(T, E, iv, len, K, n_pairs, codes, open, words, bpc, cus, st);
    else launch_ports<UNI, WIDE, true, false>(T, E, iv, len, K, n_pairs, codes, open, words, bpc, cus, st);
}

}  // namespace

int dev_reach_ports(const DevTableSet& T, const Tuning& tu, const PortsSpecDev& spec, uint32_t* out_codes,
                    uint32_t* out_open, uint32_t* out_words, void* stream, std::string* err) {
    const uint32_t ns = spec.n_src, nd = spec.n_dst, K = spec.K, ne = ns + nd;
    if (!ns || !nd || !K) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool form_a = reach_form_a(T.node, tu);  // (TCP / UDP: every interval takes the same form)
    // one scratch block: [ip u32[ne] | list u32[K] | len u32[K] | cls u32[ne]] (padded to 16 B) |
    // svc W4[K] | rec W4[ne] | g W2[K]; the host arrays go in as one copy: [ip | list | len | (cls,
    // not copied) | svc]
    auto pad = [](size_t b) { return (b + 15u) & ~(size_t)15u; };
    const size_t o_ip = 0, o_list = pad(o_ip + 4u * (size_t)ne), o_len = pad(o_list + 4u * (size_t)K);
    const size_t o_cls = pad(o_len + 4u * (size_t)K), o_svc = pad(o_cls + 4u * (size_t)ne);
    const size_t o_rec = o_svc + 16u * (size_t)K, o_g = o_rec + 16u * (size_t)ne, total = o_g + 8u * (size_t)K;
    std::vector<unsigned char> h(o_rec, 0);
    std::copy(spec.src_ip, spec.src_ip + ns, reinterpret_cast<uint32_t*>(h.data() + o_ip));
    std::copy(spec.dst_ip, spec.dst_ip + nd, reinterpret_cast<uint32_t*>(h.data() + o_ip) + ns);
    for (uint32_t k = 0; k < K; k++) {
        reinterpret_cast<uint32_t*>(h.data() + o_list)[k] = k;
        reinterpret_cast<uint32_t*>(h.data() + o_len)[k] = ports_len(spec.lo, K, k);
        reinterpret_cast<W4*>(h.data() + o_svc)[k] = reach_service((int32_t)spec.protocol, spec.src_port, spec.lo[k]);
    }
    unsigned char* d = nullptr;
    REACH_CHK(hipMalloc(&d, total));
    auto run = [&]() -> int {
        REACH_CHK(hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice));
        const uint32_t* ip = reinterpret_cast<const uint32_t*>(d + o_ip);
        const uint32_t* dl = reinterpret_cast<const uint32_t*>(d + o_list);
        const uint32_t* len = reinterpret_cast<const uint32_t*>(d + o_len);
        uint32_t* cls = reinterpret_cast<uint32_t*>(d + o_cls);
        const W4* svc = reinterpret_cast<const W4*>(d + o_svc);
        W4* rec = reinterpret_cast<W4*>(d + o_rec);
        W2* g = reinterpret_cast<W2*>(d + o_g);
        const uint32_t cus = reach_cus(), bpc = tu.blocks_per_cu, np = ns * nd;
        const unsigned ge = (ne + kReachBlock - 1) / kReachBlock, gk = (K + kReachBlock - 1) / kReachBlock;
        if (form_a) {
            hipLaunchKernelGGL(k_reach_ends<true>, dim3(ge), dim3(kReachBlock), 0, st, T, ip, ne, rec, cls);
            hipLaunchKernelGGL(k_reach_svcs<true>, dim3(gk), dim3(kReachBlock), 0, st, T, svc, dl, K, g);
            const PortsEnds E{rec, rec + ns, cls, cls + ns, nd};
            if (T.node.wide) launch_ports<true, true>(T, E, g, len, K, np, out_codes, out_open, out_words, bpc, cus, st);
            else launch_ports<true, false>(T, E, g, len, K, np, out_codes, out_open, out_words, bpc, cus, st);
        } else {
            hipLaunchKernelGGL(k_reach_ends<false>, dim3(ge), dim3(kReachBlock), 0, st, T, ip, ne, rec, nullptr);
            hipLaunchKernelGGL(k_reach_svcs<false>, dim3(gk), dim3(kReachBlock), 0, st, T, svc, dl, K, g);
            const PortsEnds E{rec, rec + ns, nullptr, nullptr, nd};
            launch_ports<false, false>(T, E, g, len, K, np, out_codes, out_open, out_words, bpc, cus, st);
        }
        REACH_CHK(hipGetLastError());
        return 0;
    };
    const int rc = run();
    // the kernels have read the scratch block before it is released
    const hipError_t es = hipStreamSynchronize(st);
    (void)hipFree(d);
    if (rc == 0 && es != hipSuccess) {
        if (err) *err = std::string("port sweep: ") + hipGetErrorString(es);
        return -1;
    }
    return rc;
}

}  // namespace pg
