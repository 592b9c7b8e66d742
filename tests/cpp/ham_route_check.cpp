// ham_route_check.cpp -- ham_search_route and the tile rules of triple_accel_amd/csrc/ham_search_plan.h against the launcher's cascade as it
// stood before the route was a function, written out here independently; the kernel each (n, k) of the GPU test's spot table takes.
// Plain g++, no GPU.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ham_search_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond) && failures++ < 10) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

// the five ifs of hamming_search_launch, each reading its switches again
struct Expect {
    int kind;                  // 0 phase, 1 bits, 2 swar16, 3 shift-add, 4 round 1
    uint32_t Q, L; int B; uint32_t NW;
};
static Expect cascade(uint32_t n, uint32_t k, bool SWAR, bool SA, bool NO_BITS, bool NO_PHASE, uint32_t phase_q) {
    Expect e{};
    {
        uint32_t Q = 0, L = 0; int B = 0;
        const uint32_t swar_x4 = 4u * (3u * ((n + 3u) / 4u) + 4u);
        if (ta::ham_phase_plan(n, k, Q, L, B) && (n > 64u || ta::ham_phase_cost_x4(Q, B) < swar_x4) && !SWAR && !SA && !NO_BITS && !NO_PHASE) {
            if ((phase_q == 1u || phase_q == 2u) && phase_q < Q) {
                uint32_t l = (n + phase_q - 1u) / phase_q;
                if (l > 32u / phase_q) l = 32u / phase_q;
                Q = phase_q; L = l;
            }
            e.kind = 0; e.Q = Q; e.L = L; e.B = B;
            return e;
        }
    }
    const int planes = ta::ham_bits_planes(k);
    if (n >= 9 && n <= 32 && planes && k < n && 3 * planes + 3 < 3 * (int)((n + 3) / 4) + 1 && !SWAR && !SA && !NO_BITS) {
        e.kind = 1; e.B = planes;
        return e;
    }
    if (n <= 64 && !SWAR && !SA) {
        e.kind = 2; e.NW = (n + 3) / 4;
        return e;
    }
    if (n <= 32 && !SWAR) {
        const uint32_t nws = (n + 3) / 4;
        e.kind = 3; e.NW = nws <= 2 ? 2u : nws <= 4 ? 4u : 8u;
        return e;
    }
    e.kind = 4;
    return e;
}

static void check_route() {
    std::vector<uint32_t> lengths;
    for (uint32_t n = 1; n <= 72; n++) lengths.push_back(n);
    for (uint32_t n : {100u, 128u, 255u, 300u, 512u, 1000u}) lengths.push_back(n);
    static const ta::HamSearchKind KIND[] = {ta::HAM_SEARCH_PHASE, ta::HAM_SEARCH_BITS, ta::HAM_SEARCH_SWAR16, ta::HAM_SEARCH_SA, ta::HAM_SEARCH_ROUND1};
    for (uint32_t n : lengths) for (uint32_t ki = 0; ki <= n + 2; ki++) for (int set = 0; set < 16; set++) for (uint32_t pq = 0; pq <= 2; pq++) {
        const uint32_t k = ki == n + 2 ? 0xFFFFFFFFu : ki;
        ta::HamSearchSwitches sw{};
        sw.swar = set & 1; sw.sa = set & 2; sw.no_bits = set & 4; sw.no_phase = set & 8; sw.phase_q = pq;
        const ta::HamSearchRoute r = ta::ham_search_route(n, k, sw);
        const Expect e = cascade(n, k, sw.swar, sw.sa, sw.no_bits, sw.no_phase, pq);
        CHECK(r.kind == KIND[e.kind], "n=%u k=%u switches=%d q=%u: kind %u, the cascade's %d", n, k, set, pq, (unsigned)r.kind, e.kind);
        if (r.kind != KIND[e.kind]) continue;
        if (e.kind == 0) CHECK(r.Q == e.Q && r.L == e.L && r.B == e.B, "n=%u k=%u switches=%d q=%u: phase <%u,%u,%d>", n, k, set, pq, r.Q, r.L, r.B);
        if (e.kind == 1) CHECK(r.B == e.B, "n=%u k=%u switches=%d: bits <%d>", n, k, set, r.B);
        if (e.kind == 2 || e.kind == 3) CHECK(r.NW == e.NW, "n=%u k=%u switches=%d: NW %u", n, k, set, r.NW);
        CHECK(r.needs_needle_dev == (e.kind == 4 || (e.kind == 0 && n > 64)), "n=%u k=%u switches=%d: needs_needle_dev", n, k, set);
        CHECK(r.scans_nul == (e.kind <= 2), "n=%u k=%u switches=%d: scans_nul", n, k, set);
    }
}

// tests/test_gpu_search.py, test_hamming_search_forms_and_fused_nul_scan: the kernel each (n, k) takes with every switch clear
static void check_names() {
    static const struct { uint32_t n, k; const char *name; } ROW[] = {
        {4, 1, "hamming_search_swar16_kernel<1>"}, {8, 2, "hamming_search_swar16_kernel<2>"}, {12, 3, "hamming_search_phase_kernel<1,2>"},
        {16, 7, "hamming_search_phase_kernel<1,3>"}, {16, 8, "hamming_search_swar16_kernel<4>"}, {24, 6, "hamming_search_phase_kernel<2,3>"},
        {32, 8, "hamming_search_phase_kernel<2,4>"}, {32, 2, "hamming_search_phase_kernel<4,2>"}, {32, 31, "hamming_search_phase_kernel<1,5>"},
        {32, 32, "hamming_search_swar16_kernel<8>"}, {40, 9, "hamming_search_phase_kernel<1,4>"}, {64, 16, "hamming_search_phase_kernel<1,5>"},
        {64, 20, "hamming_search_swar16_kernel<16>"}, {9, 1, "hamming_search_phase_kernel<2,1>"}, {16, 4, "hamming_search_phase_kernel<2,3>"},
        {70, 10, "hamming_search_phase_kernel<1,4>"}, {300, 40, "hamming_search_kernel"},
    };
    for (const auto &row : ROW) {
        char name[64];
        ta::ham_search_kernel_name(ta::ham_search_route(row.n, row.k, ta::HamSearchSwitches{}), name, sizeof(name));
        CHECK(strcmp(name, row.name) == 0, "(%u, %u): %s, not %s", row.n, row.k, name, row.name);
    }
    // the forms behind their switches, as the loader test of tests/test_gpu_search.py names them
    char name[64];
    ta::HamSearchSwitches sw{};
    sw.no_phase = true;
    ta::ham_search_kernel_name(ta::ham_search_route(12, 3, sw), name, sizeof(name));
    CHECK(strcmp(name, "hamming_search_bits_kernel<2>") == 0, "(12, 3) without phase: %s", name);
    sw = ta::HamSearchSwitches{}; sw.sa = true;
    ta::ham_search_kernel_name(ta::ham_search_route(8, 2, sw), name, sizeof(name));
    CHECK(strcmp(name, "hamming_search_sa_kernel<2>") == 0, "(8, 2) shift-add: %s", name);
    sw = ta::HamSearchSwitches{}; sw.swar = true;
    ta::ham_search_kernel_name(ta::ham_search_route(8, 2, sw), name, sizeof(name));
    CHECK(strcmp(name, "hamming_search_kernel") == 0, "(8, 2) round 1: %s", name);
}

// the tiles at the edges of their rules; the values are those of the launcher's expressions before they were functions
static void check_tiles() {
    static const struct { uint64_t len; uint32_t line, sa8, sa32; } ROW[] = {
        {1, 256, 64, 256}, {255, 256, 64, 256}, {256, 256, 64, 256}, {257, 256, 64, 256},
        {(1ull << 25) - 1, 256, 128, 256}, {1ull << 25, 256, 128, 256}, {(1ull << 25) + 1, 256, 129, 256},
        {1ull << 40, 4194304, 4194304, 4194304},
        {1ull << 62, 0x7FFFFF80u, 0x7FFFFFFFu, 0x7FFFFFFFu},           // the caps
    };
    for (const auto &row : ROW) {
        CHECK(ta::ham_search_line_tile(row.len) == row.line, "line tile of %llu: %u", (unsigned long long)row.len, ta::ham_search_line_tile(row.len));
        CHECK(ta::ham_search_sa_tile(row.len, 8) == row.sa8, "shift-add tile of %llu, n=8: %u", (unsigned long long)row.len, ta::ham_search_sa_tile(row.len, 8));
        CHECK(ta::ham_search_sa_tile(row.len, 32) == row.sa32, "shift-add tile of %llu, n=32: %u", (unsigned long long)row.len, ta::ham_search_sa_tile(row.len, 32));
        CHECK(ta::ham_search_line_tile(row.len) % 128 == 0, "line tile of %llu is whole lines", (unsigned long long)row.len);
    }
}

int main() {
    check_route();
    check_names();
    check_tiles();
    if (failures) { printf("ham route: %d failures\n", failures); return 1; }
    printf("ham route: ok\n");
    return 0;
}
