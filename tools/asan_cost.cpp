// Stand-alone sanitizer run of pg_reach_cost's host twin (pg_debug_reach_cost_host: cost.hpp's per-word
// code, the sweeps, the pull pass and cost_walk) and of its plan -- a program of its own, nothing loaded
// into Python:
//   make -C vpp_amd/csrc asan
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/asan_cost.cpp \
//       -o build/asan_cost vpp_amd/libpolicygpu_asan.so -Wl,-rpath,$PWD/vpp_amd -Wl,-rpath,/opt/rocm/lib
//   ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1 build/asan_cost
// Random matrices of 1 to 2049 end points in exactly sized buffers (an over-read is a report), random
// source lists with duplicates, weights from 1 to 65535, svc_select on and off, max_cost on and off, every
// combination of the four outputs, each exactly sized; then the plan over the whole range of n under
// every kind of budget.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "policygpu.h"
int main() {
    pg_ctx* ctx = pg_create(0);
    if (!ctx) { std::puts("no ctx"); return 2; }
    std::mt19937 g(11);
    unsigned long long reached = 0, vias = 0, runs = 0;
    for (uint32_t n : {1u, 2u, 15u, 31u, 32u, 33u, 64u, 65u, 129u, 257u, 2049u}) {
        const size_t rw = pg_reach_row_words(n);
        for (int rep = 0; rep < (n > 1000 ? 2 : 10); rep++) {
            const uint32_t n_svc = 1 + g() % 3;
            std::vector<uint32_t> m(n_svc * n * rw);   // exactly sized: an over-read is a report
            const uint32_t dens = 1 + g() % 6;
            for (auto& w : m) {
                uint32_t x = 0;
                for (int c = 0; c < 16; c++) x |= ((g() % (n / dens + 2) == 0) ? 2u : (g() & 1u ? 3u : g() % 2)) << (2 * c);
                w = x;
            }
            std::vector<uint32_t> src(g() % 5);
            for (auto& s : src) s = g() % n;
            std::vector<uint16_t> weight(n);
            for (auto& w : weight) w = (uint16_t)(g() % 8 == 0 ? 65535u : 1u + g() % 9);
            std::vector<uint8_t> sel(n_svc);
            for (auto& s : sel) s = g() % 4 != 0;
            for (int combo = 0; combo < 16; combo++)
                for (uint32_t max_cost : {0u, 7u}) {
                    std::vector<uint32_t> cost(src.size() * n), via(n);
                    std::vector<uint16_t> pred(src.size() * n), len(src.size() * n);
                    pg_reach_cost_spec spec{m.data(), n, n_svc, combo & 5 ? sel.data() : nullptr, src.empty() ? nullptr : src.data(),
                                            (uint32_t)src.size(), weight.data(), max_cost};
                    pg_reach_cost_result r;
                    const int rc = pg_debug_reach_cost_host(ctx, &spec, combo & 1 ? cost.data() : nullptr, combo & 2 ? pred.data() : nullptr,
                                                            combo & 4 ? len.data() : nullptr, combo & 8 ? via.data() : nullptr, &r);
                    if (rc) { std::printf("rc %d: %s\n", rc, pg_last_error(ctx)); return 1; }
                    unsigned long long sum = 0;
                    for (uint32_t v : via) sum += v;
                    if ((combo & 8) && sum != r.n_via) { std::printf("n %u: sum of via %llu != n_via %llu\n", n, sum, (unsigned long long)r.n_via); return 1; }
                    if (max_cost && r.max_cost > max_cost) { std::printf("n %u: a cost above max_cost\n", n); return 1; }
                    reached += r.n_reached, vias += r.n_via, runs++;
                }
        }
    }
    pg_reach_cost_plan p;
    for (int budget : {160 << 10, 64 << 10, 4096, 0}) {
        if (pg_ctx_set_tuning(ctx, "cost_lds_bytes", budget)) return 1;
        for (uint32_t n = 0; n <= (1u << 15); n += 997) {
            if (pg_debug_reach_cost_plan(ctx, n, &p)) return 1;
            if (p.lds_bytes > (160u << 10) || p.weights_in_lds > p.row_in_lds) { std::printf("plan of %u under %d\n", n, budget); return 1; }
        }
    }
    std::printf("ok: %llu runs, %llu reached cells, %llu intermediates\n", runs, reached, vias);
    pg_destroy(ctx);
    return 0;
}
