// host_rules_check.cpp -- the pure host rules of triple_accel_amd/csrc/lev_plan.h (lev_costs_valid, lev_is_unit, lev_cost_scale,
// lev_unit_scale, cross_qtile, lev_wants_length_order) against their definitions, written out here independently.  Plain g++, no GPU.
#include <stdint.h>
#include <stdio.h>

#include "lev_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond) && failures++ < 10) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static const uint32_t FIELD[] = {0, 1, 2, 3, 4, 5, 127, 128, 254, 255};

// EditCosts::new (the reference's src/levenshtein.rs:44-52): three assertions on the transposition cost, two on the others
static bool new_accepts(uint32_t mc, uint32_t gc, bool has_t, uint32_t tc) {
    if (!(mc > 0)) return false;
    if (!(gc > 0)) return false;
    if (has_t) {
        if (!(tc > 0)) return false;
        if (!((tc >> 1) < mc)) return false;
        if (!((tc >> 1) < gc)) return false;
    }
    return true;
}

static void check_costs() {
    for (uint32_t mc : FIELD) for (uint32_t gc : FIELD) for (uint32_t sg : FIELD) for (uint32_t tc : FIELD) for (int t = 0; t < 2; t++) {
        const bool has_t = t != 0;
        CHECK(ta::lev_costs_valid(mc, gc, has_t, tc) == new_accepts(mc, gc, has_t, tc), "costs (%u, %u, %u, %d:%u)", mc, gc, sg, t, tc);
        // (1, 1, 0, None) and (1, 1, 0, Some(1)), nothing else
        const bool unit = mc == 1 && gc == 1 && sg == 0 && (has_t ? tc == 1 : true);
        CHECK(ta::lev_is_unit(mc, gc, sg, has_t, tc) == unit, "unit (%u, %u, %u, %d:%u)", mc, gc, sg, t, tc);
        // (g, g, 0, None) and (g, g, 0, Some(g)) with g >= 2: g
        uint32_t multiple = 0;
        if (mc >= 2 && gc == mc && sg == 0 && (has_t ? tc == mc : true)) multiple = mc;
        CHECK(ta::lev_cost_scale(mc, gc, sg, has_t, tc) == (unit ? 1u : multiple), "scale (%u, %u, %u, %d:%u)", mc, gc, sg, t, tc);
        CHECK(ta::lev_unit_scale(mc, gc, sg, has_t, tc) == multiple, "unit_scale (%u, %u, %u, %d:%u)", mc, gc, sg, t, tc);
    }
}

// the query tiles as ta_levenshtein_cross and ta_hamming_cross computed them before cross_qtile, kept here as the expected values
static uint64_t lev_cross_qtile_before(uint64_t nq, uint64_t nt, int forced) {
    const uint64_t tgroups = (nt + 63) / 64;
    uint64_t qtile = (nq * tgroups + 16383) / 16384;
    if (qtile < 16) qtile = 16;
    if (qtile > 512) qtile = 512;
    if (forced > 0) qtile = (uint64_t)forced;
    if ((nq + qtile - 1) / qtile > 65535) qtile = (nq + 65534) / 65535;
    return qtile;
}
static uint64_t ham_cross_qtile_before(uint64_t nq, uint64_t nt, uint64_t chunk, int forced) {
    const uint64_t tgroups = (nt + 63) / 64;
    uint64_t qtile = (nq * tgroups + 16383) / 16384;
    qtile = (qtile + chunk - 1) / chunk * chunk;
    if (qtile > 512) qtile = 512;
    if (forced > 0) qtile = (uint64_t)forced;
    if ((nq + qtile - 1) / qtile > 65535) qtile = (nq + 65534) / 65535;
    return qtile;
}

static void check_qtile() {
    static const uint64_t N[] = {1, 15, 16, 17, 63, 64, 65, 4096, 65535ull * 16, 65535ull * 16 + 1, 0xFFFFFFFFull};
    static const int FORCED[] = {0, 5};
    static const uint32_t CHUNK[] = {16, 32, 64};                       // 256 / nw for nw = 16, 8, 4 (ham_cross_body.h)
    auto sane = [](uint64_t nq, uint32_t q, const char *what) {
        CHECK(q >= 1, "%s nq=%llu", what, (unsigned long long)nq);
        if (q) CHECK((nq + q - 1) / q <= 65535, "%s nq=%llu qtile=%u", what, (unsigned long long)nq, q);
    };
    for (uint64_t nq : N) for (uint64_t nt : N) for (int f : FORCED) {
        const uint32_t lev = ta::cross_qtile(nq, nt, 16, 1, f);
        CHECK(lev == lev_cross_qtile_before(nq, nt, f), "lev nq=%llu nt=%llu forced=%d: %u", (unsigned long long)nq, (unsigned long long)nt, f, lev);
        sane(nq, lev, "lev");
        for (uint32_t chunk : CHUNK) {
            const uint32_t ham = ta::cross_qtile(nq, nt, 0, chunk, f);
            CHECK(ham == ham_cross_qtile_before(nq, nt, chunk, f), "ham nq=%llu nt=%llu chunk=%u forced=%d: %u", (unsigned long long)nq,
                  (unsigned long long)nt, chunk, f, ham);
            sane(nq, ham, "ham");
        }
    }
}

static void check_length_order() {
    static const uint64_t PAIRS[] = {4095, 4096}, LEN[] = {15, 16};
    for (uint64_t n : PAIRS) for (uint64_t len : LEN) for (int csr = 0; csr < 2; csr++)
        CHECK(ta::lev_wants_length_order(csr != 0, n, len) == (csr && n == 4096 && len == 16), "csr=%d n=%llu max_len=%llu", csr,
              (unsigned long long)n, (unsigned long long)len);
    CHECK(ta::lev_wants_length_order(true, 1ull << 32, 1ull << 40), "a big ragged batch");
}

int main() {
    check_costs();
    check_qtile();
    check_length_order();
    if (failures) { printf("host rules: %d failures\n", failures); return 1; }
    printf("host rules: ok\n");
    return 0;
}
