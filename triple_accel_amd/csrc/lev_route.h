// lev_route.h -- which kernel a distance pass takes (lev_pass, ta_api.hip), as a pure rule over what the host knows: the tuning switches
// read once (LevSwitches), the facts of the pass (LevPassFacts) and the route they give (lev_pass_route); the reference's width-class
// arithmetic (lev_select) and the threshold schedule of ta_levenshtein_exp_batch (lev_exp_*), each stated once.  Plain integer logic over
// lev_plan.h: tests/cpp/lev_route_check.cpp checks it with plain g++ against the cascade lev_pass was before.
#pragma once
#include "lev_plan.h"

namespace ta {

// EditCosts as the planners take them; tc is 0 without a transposition
struct LevCosts {
    uint32_t mc, gc, sg;
    bool has_t;
    uint32_t tc;
};

// The tuning switches the distance path consults when it chooses a kernel or an order: the field f holds the
// switch named TA_ + f in capitals.  Read in ONE place (lev_switches, ta_api.hip); all clear in a process without TA_TUNING.
struct LevSwitches {
    bool no_bits, no_unit_scale;
    int force_d, force_l, force_ch, force_na;       // pin the DP band's D / L, the ring chunk, the bit-parallel window's dwords
    int bits_static;                                // lev_bits_make_plan's force_static
    bool force_affine, force_trans_select, force_wide;
    int force_widebits;                             // 64: 64 rows per lane; any other value: 32
    bool wb_no_tiles, no_latency_rule, force_sliced, no_one, no_bits2;
    // the unit-cost (bit-parallel) kernels are off: weighted costs that are unit costs times g keep the DP kernels, orders count steps
    bool unit_off() const { return no_bits || force_d || force_l; }
    // a DP kernel is asked for
    bool dp_forced() const { return unit_off() || force_affine || force_trans_select || force_wide; }
    // a kernel layout is pinned: the chooser keeps the throughput choice whatever the pair count, no single-pair / two-pair kernel
    bool pinned() const { return no_latency_rule || force_na || bits_static || force_ch || force_sliced; }
};

// what the host knows about a pass before it launches
struct LevPassFacts {
    uint32_t n_work;             // pairs (with n_dev: their upper bound)
    bool subset, n_dev;          // the pass runs over a list of pairs; the list's length lives on the device
    bool columns_ordered;        // the list is ordered by exact column count
    bool a_csr, b_csr;           // per side: CSR (else strided, every string a_len / b_len bytes)
    uint64_t a_len, b_len;
    uint64_t max_len;
    uint32_t k;
    LevCosts c;
#ifdef TA_EXPERIMENTAL
    uint32_t sliced_strips;      // strips of the pair-sliced kernel (lev_sliced_applies) for this pass's unit_k; 0: it does not apply
#endif
};

enum LevPassKind : uint32_t {
    LEV_PASS_SLICED,             // lev_sliced_launch (TA_EXPERIMENTAL builds)
    LEV_PASS_ONE,                // lev_one_launch: a single pair, the recurrence on the scalar unit
    LEV_PASS_BITS2,              // lev_bits2_launch: two pairs per lane
    LEV_PASS_BITS,               // lev_bits_launch: the bit-parallel band
    LEV_PASS_HUGE,               // lev_widebits_huge_launch per pair: row-blocked, tiled over many wavefronts
    LEV_PASS_ROWS,               // lev_widebits_launch: row-blocked, one wavefront per pair
    LEV_PASS_BAND,               // lev_band_launch: the DP band
    LEV_PASS_WIDE,               // lev_wide_launch: the wide DP
};

// the fields of ta_launch_info the host knows before it launches (the launchers say grid and lds_bytes; the wide DP also
// diags_per_lane and lanes_per_pair, the pair-sliced kernel pairs_per_wave)
struct LevLaunchInfo {
    uint32_t kernel, diags_per_lane, lanes_per_pair, pairs_per_wave, band_offset, affine, transpose, cell_bits;
};

struct LevPassRoute {
    LevPassKind kind;
    uint32_t scale;              // 0, or g: the costs are unit costs times g -- everything below describes the unit-cost pass with k / g, whose
                                 // answers are then multiplied by g (info.cell_bits alone is that of the caller's costs and k)
    uint32_t u, o, L, PW, lds_per_wave, Tw, ch, tune;   // LevParams' geometry (tune: bits 4 and 8)
    int rows_per_lane;           // the row-blocked kinds: 32 or 64
    int tmode;                   // the DP band: 0 no transposition, 1 dot4 penalty, 2 select form
    bool affine;                 //   ... and its affine instantiation
    LevPlan pl;                  // what the launchers take: the DP band's plan,
    LevBitsPlan bp;              //   the bit-parallel band's (its u is the band of the row-blocked and pair-sliced kinds too),
    LevBits2Plan b2;             //   two pairs per lane (made once no kind before it applies)
    LevLaunchInfo info;
    bool single_store;           // ONE kernel whose only store to a pair's result slot is the answer
};

// The dispatcher arithmetic of levenshtein_simd_k_with_opts (src/levenshtein.rs:731-791) in the reference's 32-bit arithmetic: the clamped
// k, unit_k and the cell width it would pick.  Valid costs (gc > 0).
struct LevSelect {
    uint32_t max_k, unit_k, cell_bits, ref_lanes;
};
static inline LevSelect lev_select(uint64_t a_len, uint64_t b_len, uint32_t k, uint32_t mc, uint32_t gc, uint32_t sg) {
    const uint32_t mn = (uint32_t)(a_len < b_len ? a_len : b_len), mx = (uint32_t)(a_len < b_len ? b_len : a_len);
    const uint32_t sub_all = mn * mc;
    const uint32_t gaps_all = (mn << 1) * gc + (mn == 0 ? 0u : sg + (mx == mn ? sg : 0u));
    const uint32_t bound = (sub_all < gaps_all ? sub_all : gaps_all) + (mx - mn) * gc + (mx == mn ? 0u : sg);
    LevSelect s;
    s.max_k = k < bound ? k : bound;
    s.unit_k = lev_sat_sub(s.max_k, sg) / gc;
    if (s.unit_k > mx) s.unit_k = mx;
    s.cell_bits = s.max_k <= 65534u ? 16 : 32;
    s.ref_lanes = 0;
    if (s.max_k <= 254u)
        for (uint32_t lanes = 32; lanes <= 256 && !s.ref_lanes; lanes *= 2)
            if (s.unit_k <= lanes - 2) { s.cell_bits = 8; s.ref_lanes = lanes; }
    return s;
}

// Which kernel runs the pass, with what geometry, and what ta_last_launch_info will say of it.
//   unit costs times g (lev_unit_scale): the unit-cost pass with k / g;
//   the unit-cost families: the chooser's pick (lev_choose) among the bit-parallel band, the row-blocked kernel and the DP kernels, with
//     the single-pair kernel for a lone pair and two pairs per lane for big fixed-length batches of narrow bands before the bit-parallel
//     band, and the tiled form of the row-blocked kernel for a handful of long fixed-length pairs;
//   everything else: the DP band where a wavefront holds the band, else the wide DP.
static inline LevPassRoute lev_pass_route(const LevPassFacts &f, const LevSwitches &sw) {
    LevPassRoute r{};
    const bool trans = f.c.has_t, dp_forced = sw.dp_forced(), pinned = sw.pinned();
    uint32_t k = f.k, mc = f.c.mc, gc = f.c.gc, tc = trans ? f.c.tc : 0u;
    const uint32_t sg = f.c.sg;
    r.info.cell_bits = lev_select(f.max_len, f.max_len, k, mc, gc, sg).cell_bits;
    if (const uint32_t g = lev_unit_scale(mc, gc, sg, trans, tc); g && !sw.unit_off() && !sw.no_unit_scale) {
        r.scale = g;
        k /= g; mc = gc = 1; tc = trans ? 1u : 0u;
    }
    const bool unit = lev_is_unit(mc, gc, sg, trans, tc);
    r.pl = lev_make_plan(k, mc, gc, sg, f.max_len, sw.force_d, sw.force_l, sw.force_ch);
    r.bp = lev_bits_make_plan(k, mc, gc, sg, trans, tc, f.max_len, sw.force_na, sw.force_ch, sw.bits_static);
    r.u = r.pl.u; r.o = r.pl.o;
    if (f.columns_ordered && f.subset) r.tune |= 4u;
    if (f.n_dev) r.tune |= 8u;                         // (tune bit 3: the grid of the upper bound, lev_bits.hip)
    r.affine = sg > 0 || sw.force_affine;
    r.info.affine = r.affine; r.info.transpose = trans;
    r.single_store = !r.scale;                         // (scaled: two stores to the result slot)
    // a pass of few pairs is as slow as its slowest wavefront: the chooser then compares wavefronts, not pairs (lev_plan.h);
    // the switches that pin a kernel layout keep the throughput choice
    LevChoice ch = lev_choose(k, mc, gc, sg, trans, tc, f.max_len, dp_forced, pinned ? 0xFFFFFFFFu : f.n_work);
    // a handful of long fixed-length pairs (the single-call API, small strided batches): the tiled row-blocked form cuts a pair's stripe
    // sweeps into tiles and spreads them over many wavefronts -- where both strings span more than two stripes of `rows` rows per lane
    const uint64_t lo = f.a_len < f.b_len ? f.a_len : f.b_len, hi = f.a_len < f.b_len ? f.b_len : f.a_len;
    auto tiles = [&](int rows) {
        return (f.n_work == 1 || (f.n_work <= 16 && !f.subset)) && !f.a_csr && !f.b_csr && lo > 2ull * 64ull * (uint64_t)rows && !sw.wb_no_tiles;
    };
    if (unit && !dp_forced && ch.kernel != LEV_K_BITS && tiles(64)) {      // ... whatever the band
        ch.kernel = LEV_K_WIDEBITS;
        ch.rows_per_lane = 64;
    }
    if (sw.force_widebits && unit && !dp_forced) {
        ch.kernel = LEV_K_WIDEBITS;
        ch.rows_per_lane = sw.force_widebits == 64 ? 64 : 32;
    }
    auto take = [&](LevPassKind kind, uint32_t kernel, uint32_t D, uint32_t L, uint32_t PW) {
        r.kind = kind;
        r.info.kernel = kernel; r.info.diags_per_lane = D; r.info.lanes_per_pair = L; r.info.pairs_per_wave = PW;
    };
#ifdef TA_EXPERIMENTAL
    // fixed-length batches with a band of 25..45 diagonals: 32 pairs per register, three band cells per lane (lev_sliced.hip);
    // opt-in -- fewer instructions than the bit-parallel band kernel but bound by the refetch of its string lines
    if (ch.kernel == LEV_K_BITS && unit && !trans && !f.subset && !dp_forced && sw.force_sliced && f.sliced_strips) {
        take(LEV_PASS_SLICED, 5, 3, f.sliced_strips, 0);
        return r;
    }
#endif
    uint32_t u_one = 0;
    if (f.n_work == 1 && !dp_forced && !pinned && !sw.force_widebits && !sw.no_one && lev_one_applies(k, mc, gc, sg, trans, tc, f.max_len, &u_one)) {
        // a lone pair with a band of up to 64 diagonals: match vectors 64 columns at a time, the recurrence on the scalar unit
        take(LEV_PASS_ONE, 6, 64, 64, 1);
        r.u = u_one; r.o = 0; r.L = 64; r.PW = 1;
        return r;
    }
    r.b2 = lev_bits2_make_plan(k, mc, gc, sg, trans, tc, f.max_len, !f.a_csr && !f.b_csr, f.n_work);
    if (ch.kernel == LEV_K_BITS && r.b2.ok && !pinned && !sw.no_bits2) {
        // narrow band, big fixed-length batch: two pairs per lane share the recurrence AND the byte test (lev_bits2_body.h, the
        // stride-8 window with both pairs' bytes in every register): 27 % fewer instructions per pair, 16 wavefronts per CU;
        // cfg4 0.118 against 0.135 ms (profiles/r03/ab_band_kernel.md)
        take(LEV_PASS_BITS2, 3, 15, 1, 128);
        r.u = r.b2.u; r.o = 0; r.L = 1; r.PW = 128; r.lds_per_wave = r.b2.lds_per_wave; r.Tw = r.b2.Tw; r.ch = 64;
    } else if (ch.kernel == LEV_K_BITS) {
        take(LEV_PASS_BITS, 3, r.bp.s8 ? 33u : 4u * (uint32_t)r.bp.NA, 1, 64);
        r.u = r.bp.u; r.o = 0; r.L = 1; r.PW = 64; r.lds_per_wave = r.bp.lds_per_wave; r.Tw = r.bp.Tw; r.ch = r.bp.ch;
    } else if (ch.kernel == LEV_K_WIDEBITS && tiles(ch.rows_per_lane) && hi <= 0xFFFFFFF0ull && hi - lo <= r.bp.u) {
        // (the launcher takes the strings themselves, pair after pair: no LevParams geometry)
        take(LEV_PASS_HUGE, 4, (uint32_t)ch.rows_per_lane, 64, 1);
        r.rows_per_lane = ch.rows_per_lane;
        r.single_store = false;                        // many launches per pair; only the last tile stores the answer
    } else if (ch.kernel == LEV_K_WIDEBITS) {
        take(LEV_PASS_ROWS, 4, (uint32_t)ch.rows_per_lane, 64, 1);
        r.rows_per_lane = ch.rows_per_lane;
        r.u = r.bp.u; r.o = 0; r.L = 64; r.PW = 1;
    } else if (r.pl.ok && !sw.force_wide) {
        take(LEV_PASS_BAND, 1, (uint32_t)r.pl.D, r.pl.L, r.pl.PW);
        r.L = r.pl.L; r.PW = r.pl.PW; r.lds_per_wave = r.pl.lds_per_wave; r.Tw = r.pl.Tw; r.ch = r.pl.ch;
        r.tmode = !trans ? 0 : ((2u * mc <= 255u + tc && !sw.force_trans_select) ? 1 : 2);
        r.info.band_offset = r.pl.o;
    } else {
        take(LEV_PASS_WIDE, 2, 0, 0, 0);               // (diagonals per thread and threads per pair: the launcher's)
        r.PW = 1;
        r.lds_per_wave = (uint32_t)((f.max_len + 2 > 0xFFFFFFF0ull) ? 0xFFFFFFF0ull : f.max_len + 2);   // boundary line length
        r.info.band_offset = r.pl.o; r.info.affine = 1;
    }
    return r;
}

// ---- the threshold schedule of ta_levenshtein_exp_batch, shared by its host-driven and its device-driven rounds.  levenshtein_exp
// returns the distance: any schedule of thresholds finds the same value (src/levenshtein.rs:1445-1454).
// The FIRST threshold is as wide as the cheapest kernel's window: the stride-8 form holds 33 diagonals whatever k <= 32 asks for (31 with the
// transposition term's two extra ones: k = 30), so unit costs start at k = 32 (g x unit costs: 32 g) for the price of 30 -- a pair at distance
// 31 or 32 is answered by the first round instead of the 61-diagonal one (cfg3 on similar strings: 32 substitutions per pair; 2.29 -> 0.9 ms per
// 100K pairs).  faithful (TA_EXP_FAITHFUL=1) keeps the reference's 30 (:1446, 1486, 1517).
static inline uint32_t lev_exp_first_k(const LevCosts &c, bool faithful) {
    return (!faithful && !c.has_t && c.sg == 0 && c.mc == c.gc) ? 32u * c.gc : 30u;    // (gap_cost <= 255: no overflow)
}
// k *= 2 (:1452), saturating instead of wrapping; after a widened first round the reference's 60, 120, ... stand
static inline uint32_t lev_exp_next_k(uint32_t k, int round, uint32_t k_first, uint32_t gc) {
    if (k > 0x7FFFFFFFu) return 0xFFFFFFFFu;
    return (round == 0 && k == k_first && k_first != 30u) ? 60u * gc : k * 2;
}
// Once a bounded pass would cost more than a quarter of the unbounded one (kernel cost model, lev_choose: per pair for big passes, per
// wavefront for small ones), it is cheaper in expectation to finish the unresolved pairs with k = u32::MAX right away.
static inline bool lev_exp_finish_now(uint32_t k, const LevCosts &c, uint64_t max_len, bool dp_only, uint32_t pairs) {
    const double c_this = lev_choose(k, c.mc, c.gc, c.sg, c.has_t, c.tc, max_len, dp_only, pairs).cost;
    const double c_full = lev_choose(0xFFFFFFFFu, c.mc, c.gc, c.sg, c.has_t, c.tc, max_len, dp_only, pairs).cost;
    return c_this > 0.25 * c_full;
}

}  // namespace ta
