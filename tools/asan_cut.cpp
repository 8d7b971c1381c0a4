// Stand-alone sanitizer run of pg_reach_cut's host twin (pg_debug_reach_cut_host: cut.hpp's per-word
// code, cut_augment and the searches) -- a program of its own, nothing loaded into Python:
//   make -C vpp_amd/csrc asan
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/asan_cut.cpp \
//       -o build/asan_cut vpp_amd/libpolicygpu_asan.so -Wl,-rpath,$PWD/vpp_amd -Wl,-rpath,/opt/rocm/lib
//   ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1 build/asan_cut
// Random matrices of 1 to 2049 end points in exactly sized buffers (an over-read is a report), random
// entry and target lists with duplicates, svc_select on and off, max_cut 0, 1 and 64, every combination
// of the outputs; then the plan over the whole range of n.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "policygpu.h"
int main() {
    pg_ctx* ctx = pg_create(0);
    if (!ctx) { std::puts("no ctx"); return 2; }
    std::mt19937 g(7);
    unsigned long total_levels = 0, runs = 0;
    for (uint32_t n : {1u, 2u, 15u, 31u, 32u, 33u, 64u, 65u, 129u, 257u, 2049u}) {
        const size_t rw = pg_reach_row_words(n);
        for (int rep = 0; rep < (n > 1000 ? 2 : 12); rep++) {
            const uint32_t n_svc = 1 + g() % 3;
            std::vector<uint32_t> m(n_svc * n * rw);   // exactly sized: an over-read is a report
            const uint32_t dens = 1 + g() % 6;
            for (auto& w : m) {
                uint32_t x = 0;
                for (int c = 0; c < 16; c++) x |= ((g() % (n / dens + 2) == 0) ? 2u : (g() & 1u ? 3u : g() % 2)) << (2 * c);
                w = x;
            }
            std::vector<uint32_t> E(g() % 4), T(g() % 4);
            for (auto& e : E) e = g() % n;
            for (auto& t : T) t = g() % n;
            std::vector<uint8_t> sel(n_svc);
            for (auto& s : sel) s = g() % 4 != 0;
            for (int combo = 0; combo < 8; combo++) {
                std::vector<uint8_t> cut(n);
                std::vector<uint16_t> prev(n), next(n);
                pg_reach_cut_spec spec{m.data(), n, n_svc, combo & 1 ? sel.data() : nullptr, E.empty() ? nullptr : E.data(), (uint32_t)E.size(),
                                       T.empty() ? nullptr : T.data(), (uint32_t)T.size(), combo == 3 ? 0u : combo == 5 ? 1u : 64u};
                pg_reach_cut_result r;
                const int rc = pg_debug_reach_cut_host(ctx, &spec, combo & 1 ? cut.data() : nullptr, combo & 2 ? prev.data() : nullptr,
                                                       combo & 4 ? next.data() : nullptr, &r);
                if (rc) { std::printf("rc %d: %s\n", rc, pg_last_error(ctx)); return 1; }
                total_levels += r.levels, runs++;
            }
        }
    }
    pg_reach_cut_plan p;
    for (uint32_t n = 0; n <= (1u << 15); n += 997) if (pg_debug_reach_cut_plan(ctx, n, &p)) return 1;
    std::printf("ok: %lu runs, %lu levels\n", runs, total_levels);
    pg_destroy(ctx);
    return 0;
}
