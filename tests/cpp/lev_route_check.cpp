// lev_route_check.cpp -- lev_pass_route, lev_select and the exp schedule of triple_accel_amd/csrc/lev_route.h against the code they
// replaced, written out here independently: the cascade lev_pass was (its switches as plain parameters, its self-recursion for unit costs
// times g), ta_levenshtein_select's arithmetic, and the two copies of the threshold schedule ta_levenshtein_exp_batch held; the rows of the
// GPU spot test (tests/test_gpu_lev_route.py) as literals.  Plain g++, no GPU; -DTA_EXPERIMENTAL adds the pair-sliced kind.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "lev_route.h"

using namespace ta;

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond) && failures++ < 10) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

// ---- ta_levenshtein_select as it stood (src/levenshtein.rs:731-791)
static uint32_t select_cell_bits(uint64_t a_len, uint64_t b_len, uint32_t k, uint32_t mc, uint32_t gc, uint32_t sg, uint32_t *max_k_out = nullptr,
                                 uint32_t *unit_k_out = nullptr, uint32_t *lanes_out = nullptr) {
    const uint32_t mn = (uint32_t)(a_len < b_len ? a_len : b_len), mx = (uint32_t)(a_len < b_len ? b_len : a_len);
    uint32_t sub_all = mn * mc;
    uint32_t gaps_all = (mn << 1) * gc + (mn == 0 ? 0u : sg + (mx == mn ? sg : 0u));
    uint32_t bound = (sub_all < gaps_all ? sub_all : gaps_all) + (mx - mn) * gc + (mx == mn ? 0u : sg);
    uint32_t max_k = k < bound ? k : bound;
    uint32_t unit_k = lev_sat_sub(max_k, sg) / gc;
    if (unit_k > mx) unit_k = mx;
    if (max_k_out) *max_k_out = max_k;
    if (unit_k_out) *unit_k_out = unit_k;
    if (lanes_out) *lanes_out = 0;
    uint32_t cell_bits = 32;
    static const uint32_t ub[4] = {32, 64, 128, 256};
    if (max_k <= 254u) {
        for (int t = 0; t < 4; t++)
            if (unit_k <= ub[t] - 2) { if (lanes_out) *lanes_out = ub[t]; return 8; }
    }
    if (max_k <= 65534u) cell_bits = 16;
    return cell_bits;
}

// ---- lev_pass as it stood: every env_int("TA_X") is the parameter X, every launch the record of what it was given.  What the old code left
// unset in LevParams (the geometry of the branches that do not read it) is zero here.
struct Sw {
    int NO_BITS, NO_UNIT_SCALE, FORCE_D, FORCE_L, FORCE_CH, FORCE_NA, BITS_STATIC, FORCE_AFFINE, FORCE_TRANS_SELECT, FORCE_WIDE, FORCE_WIDEBITS,
        WB_NO_TILES, NO_LATENCY_RULE, FORCE_SLICED, NO_ONE, NO_BITS2;
};
struct Side { bool off; uint64_t len; };
static LevPassRoute expected(const Side *a, const Side *b, uint32_t n_work, bool subset, uint32_t k, LevCosts c, uint64_t max_len, bool columns_ordered,
                             bool n_dev, uint32_t strips_fact, const Sw &S) {
    const uint32_t gc = c.gc, sg = c.sg;
    if (const uint32_t g = lev_unit_scale(c.mc, gc, sg, c.has_t, c.tc);
        g && !S.NO_BITS && !S.NO_UNIT_SCALE && !S.FORCE_D && !S.FORCE_L) {
        const LevCosts uc = {1, 1, 0, c.has_t, c.has_t ? 1u : 0u};
        LevPassRoute r = expected(a, b, n_work, subset, k / g, uc, max_len, columns_ordered, n_dev, strips_fact, S);
        r.scale = g;
        r.single_store = false;
        r.info.cell_bits = select_cell_bits(max_len, max_len, k, c.mc, gc, sg);
        return r;
    }
    LevPassRoute r{};
    LevPlan pl = lev_make_plan(k, c.mc, gc, sg, max_len, S.FORCE_D, S.FORCE_L, S.FORCE_CH);
    struct { uint32_t mc, tc, u, o, L, PW, lds_per_wave, Tw, ch, tune; } P = {};
    P.mc = c.mc; P.tc = c.has_t ? c.tc : 0;
    P.u = pl.u; P.o = pl.o;
    if (columns_ordered && subset) P.tune |= 4u;
    if (n_dev) P.tune |= 8u;
    const bool affine = sg > 0 || S.FORCE_AFFINE, trans = c.has_t;
    LevLaunchInfo li = {};
    li.band_offset = pl.o; li.affine = affine; li.transpose = trans;
    bool single_store = true;
    li.cell_bits = select_cell_bits(max_len, max_len, k, c.mc, gc, sg);
    const uint32_t tcost = c.has_t ? c.tc : 0;
    const LevBitsPlan bp = lev_bits_make_plan(k, c.mc, gc, sg, trans, tcost, max_len, S.FORCE_NA, S.FORCE_CH, S.BITS_STATIC);
    const bool dp_forced = S.NO_BITS || S.FORCE_D || S.FORCE_L || S.FORCE_AFFINE || S.FORCE_TRANS_SELECT || S.FORCE_WIDE;
    const bool pinned = S.NO_LATENCY_RULE || S.FORCE_NA || S.BITS_STATIC || S.FORCE_CH || S.FORCE_SLICED;
    LevChoice ch = lev_choose(k, c.mc, gc, sg, trans, tcost, max_len, dp_forced, pinned ? 0xFFFFFFFFu : n_work);
    const bool unit = lev_is_unit(c.mc, gc, sg, c.has_t, c.tc);
    if (unit && !dp_forced && ch.kernel != LEV_K_BITS && (n_work == 1 || (n_work <= 16 && !subset)) && !a->off && !b->off &&
        (a->len < b->len ? a->len : b->len) > 2ull * 4096ull && !S.WB_NO_TILES) {
        ch.kernel = LEV_K_WIDEBITS;
        ch.rows_per_lane = 64;
    }
    if (S.FORCE_WIDEBITS && unit && !dp_forced) {
        ch.kernel = LEV_K_WIDEBITS;
        ch.rows_per_lane = S.FORCE_WIDEBITS == 64 ? 64 : 32;
    }
    auto done = [&]() {
        r.u = P.u; r.o = P.o; r.L = P.L; r.PW = P.PW; r.lds_per_wave = P.lds_per_wave; r.Tw = P.Tw; r.ch = P.ch; r.tune = P.tune;
        r.affine = affine; r.pl = pl; r.bp = bp; r.info = li; r.single_store = single_store;
        return r;
    };
#ifdef TA_EXPERIMENTAL
    const bool sliced = ch.kernel == LEV_K_BITS && unit && !trans && !subset && !dp_forced && S.FORCE_SLICED && strips_fact;
    if (sliced) {
        r.kind = LEV_PASS_SLICED;
        li.kernel = 5; li.diags_per_lane = 3; li.lanes_per_pair = strips_fact; li.pairs_per_wave = 0 /* the launcher's */;
        li.band_offset = 0;
        return done();
    }
#else
    (void)strips_fact;
#endif
    uint32_t u_one = 0;
    if (n_work == 1 && !dp_forced && !pinned && !S.FORCE_WIDEBITS && !S.NO_ONE &&
        lev_one_applies(k, c.mc, gc, sg, trans, tcost, max_len, &u_one)) {
        P.u = u_one; P.o = 0; P.L = 64; P.PW = 1; P.lds_per_wave = 0; P.Tw = 0; P.ch = 0;
        r.kind = LEV_PASS_ONE;
        li.kernel = 6; li.diags_per_lane = 64; li.lanes_per_pair = 64; li.pairs_per_wave = 1;
        li.band_offset = 0;
        return done();
    }
    const LevBits2Plan b2 = lev_bits2_make_plan(k, c.mc, gc, sg, trans, tcost, max_len, !a->off && !b->off, n_work);
    r.b2 = b2;
    if (ch.kernel == LEV_K_BITS && b2.ok && !pinned && !S.NO_BITS2) {
        P.u = b2.u; P.o = 0; P.L = 1; P.PW = 128; P.lds_per_wave = b2.lds_per_wave; P.Tw = b2.Tw; P.ch = 64;
        r.kind = LEV_PASS_BITS2;
        li.kernel = 3; li.diags_per_lane = 15; li.lanes_per_pair = 1; li.pairs_per_wave = 128;
        li.band_offset = 0;
    } else if (ch.kernel == LEV_K_BITS) {
        P.u = bp.u; P.o = 0; P.L = 1; P.PW = 64; P.lds_per_wave = bp.lds_per_wave; P.Tw = bp.Tw; P.ch = bp.ch;
        r.kind = LEV_PASS_BITS;
        li.kernel = 3; li.diags_per_lane = bp.s8 ? 33u : 4u * (uint32_t)bp.NA; li.lanes_per_pair = 1; li.pairs_per_wave = 64;
        li.band_offset = 0;
    } else if (ch.kernel == LEV_K_WIDEBITS && (n_work == 1 || (n_work <= 16 && !subset)) && !a->off && !b->off &&
               a->len <= 0xFFFFFFF0ull && b->len <= 0xFFFFFFF0ull &&
               (a->len < b->len ? a->len : b->len) > 2ull * 64ull * (uint64_t)ch.rows_per_lane &&
               (a->len > b->len ? a->len - b->len : b->len - a->len) <= bp.u && !S.WB_NO_TILES) {
        single_store = false;
        r.kind = LEV_PASS_HUGE; r.rows_per_lane = ch.rows_per_lane;
        li.kernel = 4; li.diags_per_lane = (uint32_t)ch.rows_per_lane; li.lanes_per_pair = 64; li.pairs_per_wave = 1;
        li.band_offset = 0;
    } else if (ch.kernel == LEV_K_WIDEBITS) {
        P.u = bp.u; P.o = 0; P.L = 64; P.PW = 1; P.lds_per_wave = 0; P.Tw = 0; P.ch = 0;
        r.kind = LEV_PASS_ROWS; r.rows_per_lane = ch.rows_per_lane;
        li.kernel = 4; li.diags_per_lane = (uint32_t)ch.rows_per_lane; li.lanes_per_pair = 64; li.pairs_per_wave = 1;
        li.band_offset = 0;
    } else if (pl.ok && !S.FORCE_WIDE) {
        P.L = pl.L; P.PW = pl.PW; P.lds_per_wave = pl.lds_per_wave; P.Tw = pl.Tw; P.ch = pl.ch;
        r.tmode = !trans ? 0 : ((2u * P.mc <= 255u + P.tc && !S.FORCE_TRANS_SELECT) ? 1 : 2);
        r.kind = LEV_PASS_BAND;
        li.kernel = 1; li.diags_per_lane = pl.D; li.lanes_per_pair = pl.L; li.pairs_per_wave = pl.PW;
    } else {
        P.L = 0; P.PW = 1; P.Tw = 0;
        P.lds_per_wave = (uint32_t)((max_len + 2 > 0xFFFFFFF0ull) ? 0xFFFFFFF0ull : max_len + 2);
        r.kind = LEV_PASS_WIDE;
        li.kernel = 2; li.diags_per_lane = 0 /* the launcher's */; li.lanes_per_pair = 0 /* the launcher's */; li.pairs_per_wave = 0;
        li.affine = 1;
    }
    return done();
}

// every field of a route; 0: the same, else the number of the first field that differs
static int differs(const LevPassRoute &x, const LevPassRoute &y) {
    int f = 0;
#define SAME(m) do { f++; if (!(x.m == y.m)) return f; } while (0)
    SAME(kind); SAME(scale); SAME(u); SAME(o); SAME(L); SAME(PW); SAME(lds_per_wave); SAME(Tw); SAME(ch); SAME(tune);
    SAME(rows_per_lane); SAME(tmode); SAME(affine); SAME(single_store);
    SAME(pl.u); SAME(pl.o); SAME(pl.need); SAME(pl.D); SAME(pl.L); SAME(pl.PW); SAME(pl.lds_per_wave); SAME(pl.ok);
    if (x.pl.ok) { SAME(pl.Tw); SAME(pl.ch); }              // (lev_make_plan sets them for a band that fits)
    SAME(bp.ok); SAME(bp.u); SAME(bp.NA); SAME(bp.stat); SAME(bp.s8); SAME(bp.Tw); SAME(bp.ch); SAME(bp.lds_per_wave);
    SAME(b2.ok); SAME(b2.NA); SAME(b2.u); SAME(b2.Tw); SAME(b2.lds_per_wave);
    SAME(info.kernel); SAME(info.diags_per_lane); SAME(info.lanes_per_pair); SAME(info.pairs_per_wave); SAME(info.band_offset);
    SAME(info.affine); SAME(info.transpose); SAME(info.cell_bits);
#undef SAME
    return 0;
}

static const uint32_t NWORK[] = {1, 2, 16, 17, 1024, 1025, 262143, 262144};
static const uint64_t LENS[] = {1, 100, 128, 129, 4096, 8192, 8193, 32000, 32001, 65000, 65001, 70000};
static const uint32_t KS[] = {0, 1, 6, 7, 12, 13, 14, 15, 30, 31, 32, 33, 62, 63, 64, 126, 254, 1000, 0xFFFFFFFFu};
static const LevCosts COSTS[] = {{1, 1, 0, false, 0}, {1, 1, 0, true, 1}, {2, 2, 0, false, 0}, {2, 2, 0, true, 2}, {1, 1, 1, false, 0},
                                 {3, 2, 0, false, 0}, {2, 3, 1, true, 2}, {255, 255, 255, false, 0}};
// (subset, n_dev, columns_ordered): a list's length on the device needs a list; columns_ordered without one must change nothing
static const bool LISTS[][3] = {{false, false, false}, {true, false, false}, {true, true, false}, {true, false, true}, {true, true, true}, {false, false, true}};

// the switch sets: all clear, each switch alone, and the further values of the ones that carry a number
struct SwSet { const char *name; Sw old; LevSwitches now; };
static std::vector<SwSet> switch_sets() {
    std::vector<SwSet> v;
    auto add = [&](const char *name, int Sw::*o, int value, auto LevSwitches::*n) {
        SwSet s{name, Sw{}, LevSwitches{}};
        if (o) { s.old.*o = value; s.now.*n = value; }
        v.push_back(s);
    };
    add("clear", nullptr, 0, &LevSwitches::no_bits);
    add("TA_NO_BITS", &Sw::NO_BITS, 1, &LevSwitches::no_bits);
    add("TA_NO_UNIT_SCALE", &Sw::NO_UNIT_SCALE, 1, &LevSwitches::no_unit_scale);
    add("TA_FORCE_D", &Sw::FORCE_D, 8, &LevSwitches::force_d);
    add("TA_FORCE_L", &Sw::FORCE_L, 4, &LevSwitches::force_l);
    add("TA_FORCE_CH", &Sw::FORCE_CH, 16, &LevSwitches::force_ch);
    add("TA_FORCE_NA", &Sw::FORCE_NA, 16, &LevSwitches::force_na);
    add("TA_BITS_STATIC", &Sw::BITS_STATIC, 1, &LevSwitches::bits_static);
    add("TA_BITS_STATIC", &Sw::BITS_STATIC, 2, &LevSwitches::bits_static);
    add("TA_BITS_STATIC", &Sw::BITS_STATIC, 3, &LevSwitches::bits_static);
    add("TA_FORCE_AFFINE", &Sw::FORCE_AFFINE, 1, &LevSwitches::force_affine);
    add("TA_FORCE_TRANS_SELECT", &Sw::FORCE_TRANS_SELECT, 1, &LevSwitches::force_trans_select);
    add("TA_FORCE_WIDE", &Sw::FORCE_WIDE, 1, &LevSwitches::force_wide);
    add("TA_FORCE_WIDEBITS", &Sw::FORCE_WIDEBITS, 32, &LevSwitches::force_widebits);
    add("TA_FORCE_WIDEBITS", &Sw::FORCE_WIDEBITS, 64, &LevSwitches::force_widebits);
    add("TA_WB_NO_TILES", &Sw::WB_NO_TILES, 1, &LevSwitches::wb_no_tiles);
    add("TA_NO_LATENCY_RULE", &Sw::NO_LATENCY_RULE, 1, &LevSwitches::no_latency_rule);
    add("TA_FORCE_SLICED", &Sw::FORCE_SLICED, 1, &LevSwitches::force_sliced);
    add("TA_NO_ONE", &Sw::NO_ONE, 1, &LevSwitches::no_one);
    add("TA_NO_BITS2", &Sw::NO_BITS2, 1, &LevSwitches::no_bits2);
    return v;
}

// the length pairs: every length against itself, and unequal ones whose difference sits on either side of the bands the thresholds give
// (1 against k = 0 and 1; 28 and 29 against 15 .. 33; thousands against 1000 and the unbounded pass)
static std::vector<std::pair<uint64_t, uint64_t>> length_pairs() {
    std::vector<std::pair<uint64_t, uint64_t>> v;
    for (uint64_t l : LENS) v.push_back({l, l});
    static const uint64_t UNEQ[][2] = {{128, 129}, {8192, 8193}, {32000, 32001}, {65000, 65001}, {100, 128}, {100, 129}, {1, 100},
                                       {4096, 8193}, {8193, 32000}, {32001, 65000}, {65001, 70000}};
    for (const auto &p : UNEQ) { v.push_back({p[0], p[1]}); v.push_back({p[1], p[0]}); }
    return v;
}

static void check_route() {
    const std::vector<SwSet> sets = switch_sets();
    const auto lens = length_pairs();
    uint64_t kinds_clear[8] = {}, kinds_any[8] = {}, points = 0, tick = 0;
    std::vector<uint64_t> changed(sets.size(), 0);
    for (uint32_t n_work : NWORK) for (const auto &lst : LISTS) for (int layout = 0; layout < 4; layout++) for (const auto &len : lens)
    for (uint32_t k : KS) for (const LevCosts &c : COSTS) {
        const Side a = {(layout & 1) != 0, len.first}, b = {(layout & 2) != 0, len.second};
        LevPassFacts f{};
        f.n_work = n_work; f.subset = lst[0]; f.n_dev = lst[1]; f.columns_ordered = lst[2];
        f.a_csr = a.off; f.b_csr = b.off; f.a_len = a.len; f.b_len = b.len; f.max_len = std::max(a.len, b.len);
        f.k = k; f.c = c;
        uint32_t strips = 0;
#ifdef TA_EXPERIMENTAL
        // the caller's fact (lev_sliced_applies): the plan of the strided lengths and the unit-cost pass's band
        if (const uint32_t g = lev_cost_scale(c.mc, c.gc, c.sg, c.has_t, c.tc); g && !a.off && !b.off) {
            const LevSlicedPlan sp = lev_sliced_make_plan(a.len, b.len, lev_batch_unit_k(k / g, 1, 1, 0, f.max_len));
            strips = sp.ok ? sp.S : 0;
        }
        f.sliced_strips = strips;
#endif
        LevPassRoute clear{};
        // thinning: the facts in full with every switch clear; each other switch set at every 7th point (a stride
        // coprime to every dimension of the grid), the sets taking turns on the phase
        for (size_t s = 0; s < sets.size(); s++) {
            if (s && (tick + s) % 7) continue;
            const LevPassRoute r = lev_pass_route(f, sets[s].now);
            const LevPassRoute e = expected(&a, &b, n_work, lst[0], k, c, f.max_len, lst[2], lst[1], strips, sets[s].old);
            const int d = differs(r, e);
            CHECK(d == 0, "n=%u list=%d%d%d layout=%d len=%llu/%llu k=%u costs=(%u,%u,%u,%d,%u) %s=%d: field %d differs (kind %u, the cascade's %u)", n_work,
                  lst[0], lst[1], lst[2], layout, (unsigned long long)a.len, (unsigned long long)b.len, k, c.mc, c.gc, c.sg, (int)c.has_t, c.tc,
                  sets[s].name, s ? 1 : 0, d, (unsigned)r.kind, (unsigned)e.kind);
            points++;
            kinds_any[r.kind]++;
            if (!s) { clear = r; kinds_clear[r.kind]++; }
            else if (differs(r, clear)) changed[s]++;
        }
        tick++;
    }
    // the thinning hid no hole: every kind of this build with all switches clear, every switch set with an effect somewhere
#ifdef TA_EXPERIMENTAL
    CHECK(kinds_any[LEV_PASS_SLICED] > 0, "the grid never reaches the pair-sliced kind");
#else
    CHECK(kinds_any[LEV_PASS_SLICED] == 0, "pair-sliced outside a TA_EXPERIMENTAL build");
#endif
    CHECK(kinds_clear[LEV_PASS_SLICED] == 0, "pair-sliced without its switch");
    for (uint32_t kind = LEV_PASS_ONE; kind <= LEV_PASS_WIDE; kind++) CHECK(kinds_clear[kind] > 0, "the grid never reaches kind %u with the switches clear", kind);
    for (size_t s = 1; s < sets.size(); s++) CHECK(changed[s] > 0, "%s (set %zu) changes no route of the grid", sets[s].name, s);
    printf("lev route: %llu grid points; kinds with the switches clear:", (unsigned long long)points);
    for (uint32_t kind = 0; kind < 8; kind++) printf(" %llu", (unsigned long long)kinds_clear[kind]);
    printf("\n");
}

// tests/test_gpu_lev_route.py: what ta_last_launch_info says of the smallest shape that reaches each kind with every switch clear
// (strided batches of equal lengths; the same literals there)
static void check_spots() {
    static const struct { uint32_t n; uint64_t len; uint32_t k; LevCosts c; LevPassKind kind; uint32_t scale, kernel, D, L, PW, o; bool single_store; } ROW[] = {
        {1, 40, 5, {1, 1, 0, false, 0}, LEV_PASS_ONE, 0, 6, 64, 64, 1, 0, true},
        {64, 100, 10, {1, 1, 0, false, 0}, LEV_PASS_BITS, 0, 3, 12, 1, 64, 0, true},
        {262144, 16, 3, {1, 1, 0, false, 0}, LEV_PASS_BITS2, 0, 3, 15, 1, 128, 0, true},
        {1, 3000, 0xFFFFFFFFu, {1, 1, 0, false, 0}, LEV_PASS_ROWS, 0, 4, 64, 64, 1, 0, true},
        {1, 8200, 0xFFFFFFFFu, {1, 1, 0, false, 0}, LEV_PASS_HUGE, 0, 4, 64, 64, 1, 0, false},
        {64, 100, 10, {3, 2, 1, false, 0}, LEV_PASS_BAND, 0, 1, 6, 1, 64, 3, true},
        {2, 2816, 0xFFFFFFFFu, {3, 2, 1, false, 0}, LEV_PASS_WIDE, 0, 2, 0, 0, 0, 2113, true},        // (D and L: the launcher's)
        {64, 100, 20, {2, 2, 0, false, 0}, LEV_PASS_BITS, 2, 3, 12, 1, 64, 0, false},
    };
    for (const auto &row : ROW) {
        LevPassFacts f{};
        f.n_work = row.n; f.a_len = f.b_len = f.max_len = row.len; f.k = row.k; f.c = row.c;
        const LevPassRoute r = lev_pass_route(f, LevSwitches{});
        CHECK(r.kind == row.kind && r.scale == row.scale && r.info.kernel == row.kernel && r.info.diags_per_lane == row.D && r.info.lanes_per_pair == row.L &&
              r.info.pairs_per_wave == row.PW && r.info.band_offset == row.o && r.single_store == row.single_store,
              "n=%u len=%llu k=%u costs=(%u,%u,%u): kind %u scale %u kernel %u D %u L %u PW %u o %u single_store %d", row.n, (unsigned long long)row.len, row.k,
              row.c.mc, row.c.gc, row.c.sg, (unsigned)r.kind, r.scale, r.info.kernel, r.info.diags_per_lane, r.info.lanes_per_pair, r.info.pairs_per_wave,
              r.info.band_offset, (int)r.single_store);
    }
}

// ---- the two loops of ta_levenshtein_exp_batch as they stood, reduced to their thresholds: a list that never shrinks (the device-driven
// loop's premise; the host-driven one with n_left = pairs throughout)
static uint32_t old_first_k(const LevCosts &c, bool faithful) {
    uint32_t k_first = 30;
    if (!faithful && !c.has_t && c.sg == 0 && c.mc == c.gc) k_first = 32u * c.gc;
    return k_first;
}
static std::vector<uint32_t> old_device_loop(const LevCosts &costs, uint64_t max_len, bool dpo, uint32_t n, bool faithful) {
    std::vector<uint32_t> ks;
    const uint32_t k_first = old_first_k(costs, faithful), tcx = costs.has_t ? costs.tc : 0;
    uint32_t k = k_first;
    constexpr int MAX_ROUNDS = 40;
    for (int round = 0; round < MAX_ROUNDS; round++) {
        if (!faithful && k != 0xFFFFFFFFu) {
            const double c_this = lev_choose(k, costs.mc, costs.gc, costs.sg, costs.has_t, tcx, max_len, dpo, n).cost;
            const double c_full = lev_choose(0xFFFFFFFFu, costs.mc, costs.gc, costs.sg, costs.has_t, tcx, max_len, dpo, n).cost;
            if (c_this > 0.25 * c_full) k = 0xFFFFFFFFu;
        }
        ks.push_back(k);
        if (k == 0xFFFFFFFFu) break;
        k = (k > 0x7FFFFFFFu) ? 0xFFFFFFFFu : (round == 0 && k == k_first && k_first != 30u ? 60u * costs.gc : k * 2);
    }
    return ks;
}
static std::vector<uint32_t> old_host_loop(const LevCosts &costs, uint64_t max_len, bool dpo, uint32_t n, bool faithful) {
    std::vector<uint32_t> ks;
    const uint32_t k_first = old_first_k(costs, faithful), tcx = costs.has_t ? costs.tc : 0;
    uint32_t k = k_first, n_left = n;
    for (int round = 0; round < 40 && n_left > 0; round++) {
        if (!faithful && k != 0xFFFFFFFFu) {
            const double c_this = lev_choose(k, costs.mc, costs.gc, costs.sg, costs.has_t, tcx, max_len, dpo, n_left).cost;
            const double c_full = lev_choose(0xFFFFFFFFu, costs.mc, costs.gc, costs.sg, costs.has_t, tcx, max_len, dpo, n_left).cost;
            if (c_this > 0.25 * c_full) k = 0xFFFFFFFFu;
        }
        ks.push_back(k);
        if (k == 0xFFFFFFFFu) break;
        k = (k > 0x7FFFFFFFu) ? 0xFFFFFFFFu : (round == 0 && k == k_first && k_first != 30u ? 60u * costs.gc : k * 2);
    }
    return ks;
}
// the loop both are now: lev_exp_first_k, lev_exp_finish_now, lev_exp_next_k
static std::vector<uint32_t> new_loop(const LevCosts &costs, uint64_t max_len, bool dpo, uint32_t n, bool faithful) {
    std::vector<uint32_t> ks;
    const uint32_t k_first = lev_exp_first_k(costs, faithful);
    uint32_t k = k_first;
    for (int round = 0; round < 40; round++) {
        if (!faithful && k != 0xFFFFFFFFu && lev_exp_finish_now(k, costs, max_len, dpo, n)) k = 0xFFFFFFFFu;
        ks.push_back(k);
        if (k == 0xFFFFFFFFu) break;
        k = lev_exp_next_k(k, round, k_first, costs.gc);
    }
    return ks;
}
static void check_exp() {
    uint64_t rounds = 0;
    bool finished_early = false, ran_out = false, widened = false;
    for (const LevCosts &c : COSTS) for (uint64_t max_len : {1ull, 63ull, 64ull, 1000ull, 100000ull}) for (uint32_t pairs : {1u, 1023u, 1024u, 1000000u})
    for (int faithful = 0; faithful < 2; faithful++) for (int dpo = 0; dpo < 2; dpo++) {
        const std::vector<uint32_t> dev = old_device_loop(c, max_len, dpo, pairs, faithful), host = old_host_loop(c, max_len, dpo, pairs, faithful),
                                    now = new_loop(c, max_len, dpo, pairs, faithful);
        CHECK(now == dev && now == host, "costs=(%u,%u,%u,%d,%u) max_len=%llu pairs=%u faithful=%d dp_only=%d: %zu rounds, the loops' %zu and %zu", c.mc, c.gc, c.sg,
              (int)c.has_t, c.tc, (unsigned long long)max_len, pairs, faithful, dpo, now.size(), dev.size(), host.size());
        rounds += now.size();
        if (now.back() == 0xFFFFFFFFu && now.size() >= 2 && now[now.size() - 2] > 0x7FFFFFFFu) ran_out = true;        // the doubling saturated
        else if (now.back() == 0xFFFFFFFFu) finished_early = true;                                                   // the quarter rule
        if (now.size() > 1 && now[0] == 32u * c.gc && now[1] == 60u * c.gc) widened = true;
    }
    CHECK(finished_early && ran_out && widened, "the exp grid misses a rule: quarter rule %d, saturation %d, widened first round %d", (int)finished_early, (int)ran_out, (int)widened);
    printf("lev route: %llu exp rounds\n", (unsigned long long)rounds);
}

static void check_select() {
    for (uint64_t la : LENS) for (uint64_t lb : LENS) for (uint32_t k : KS) for (const LevCosts &c : COSTS) {
        uint32_t max_k = 0, unit_k = 0, lanes = 0;
        const uint32_t bits = select_cell_bits(la, lb, k, c.mc, c.gc, c.sg, &max_k, &unit_k, &lanes);
        const LevSelect s = lev_select(la, lb, k, c.mc, c.gc, c.sg);
        CHECK(s.cell_bits == bits && s.max_k == max_k && s.unit_k == unit_k && s.ref_lanes == lanes, "select(%llu, %llu, %u, (%u,%u,%u)): %u bits, max_k %u, unit_k %u, lanes %u",
              (unsigned long long)la, (unsigned long long)lb, k, c.mc, c.gc, c.sg, s.cell_bits, s.max_k, s.unit_k, s.ref_lanes);
    }
    // lengths beyond 32 bits wrap as the reference's u32 arithmetic does
    CHECK(lev_select((1ull << 32) + 5, (1ull << 32) + 5, 3, 1, 1, 0).cell_bits == select_cell_bits((1ull << 32) + 5, (1ull << 32) + 5, 3, 1, 1, 0), "wrapped lengths");
}

int main() {
    check_route();
    check_spots();
    check_exp();
    check_select();
    if (failures) { printf("lev route: %d failures\n", failures); return 1; }
    printf("lev route: ok\n");
    return 0;
}
