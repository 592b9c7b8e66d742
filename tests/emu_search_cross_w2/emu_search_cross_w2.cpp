// emu_search_cross_w2.cpp -- host emulation driver of the search cross two-word route (lev_search_cross_w2_body.h).  TESTS ONLY: the
// whole call as the kernels of lev_search_cross_w2.hip run it -- the sub-batch loop, per workgroup the 512-thread build of the
// [256][32][2] table, per wavefront 64 emulated lanes (lane l on column l mod 32) with the group's own G, the candidate list in ballot
// order, the exact pass per record over its span with the column in memory (one column per resident lane, element-major, poisoned
// before every pair), the nearest / per-haystack folds and the finish pass.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "emu_wave.h"
#include "lev_search_cross_w2_body.h"

using namespace ta;

namespace {

struct Side {
    const uint8_t *blob;
    const uint64_t *off;
    const uint8_t *ptr(uint32_t i) const { return blob + off[i]; }
    uint64_t len(uint32_t i) const { return off[i + 1] - off[i]; }
};

struct Call {
    Side nd, hs;
    uint32_t nn, nh;
    SearchCosts C;
    bool trans;
    uint32_t kf, halo, max_needle;
    ta_search_cross_hit *hits;
    uint64_t *count, cap;
    uint64_t *nearest;
    ta_match *best;
    uint32_t *per_haystack, *spans;
    std::vector<SxRec> rec;
    uint32_t n_rec;
    std::vector<uint32_t> col;
    uint32_t col_lanes;
};

// one scan workgroup: blockIdx = (bx, group), haystacks [h0, h1) of the sub-batch, hpw per workgroup.  Returns 0, or what went wrong.
template <bool TRANS>
int scan_workgroup(Call &c, uint32_t bx, uint32_t group, uint32_t h0, uint32_t h1, uint32_t hpw) {
    static uint32_t peq[256 * SX2_GROUP * 2];
    const uint32_t g0 = group * SX2_GROUP, size = sx2_group_size(c.nn, group), G = sx_group_cols(size), S = 64 / G;
    if (size == 0 || G < size || G > SX2_GROUP || (G & (G - 1)) || (G > 1 && G / 2 >= size) || S < 2) return 10;
    const uint8_t *np[64];
    uint32_t n[64];
    bool has[64], scans[64];
    for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t col = lane & (G - 1);
        has[lane] = col < size;
        np[lane] = has[lane] ? c.nd.ptr(g0 + col) : nullptr;
        n[lane] = has[lane] ? (uint32_t)c.nd.len(g0 + col) : 0;
        scans[lane] = has[lane] && sx_scans(n[lane], c.kf);
    }
    // the table, thread by thread as the kernel fills it: the wildcard words, (barrier), the needles' bits
    memset(peq, 0xA5, sizeof peq);
    for (uint32_t wave = 0; wave < SX_WAVES; wave++)
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t column = lane & (SX2_GROUP - 1), half = lane >> 5;
            for (uint32_t ch = wave * 32; ch < wave * 32 + 32; ch++) peq[sx2_peq_at(ch, column, half)] = scans[lane] ? sx2_peq_wild(n[lane], half) : 0u;
        }
    for (uint32_t wave = 0; wave < SX_WAVES; wave++)
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t column = lane & (SX2_GROUP - 1), half = lane >> 5;
            if (scans[lane])
                for (uint32_t j = wave * 2 + half; j < n[lane]; j += 2 * SX_WAVES) {
                    uint32_t w;
                    const uint32_t bit = sx2_peq_bit(n[lane], j, w);
                    peq[sx2_peq_at((uint32_t)np[lane][j], column, w)] |= bit;
                }
        }
    for (uint32_t lane = 0; lane < 64; lane++)                    // column l mod 32 = lev_filter_peq_word of lane l's needle, row by row
        for (uint32_t ch = 0; ch < 256; ch++)
            for (uint32_t w = 0; w < 2; w++)
                if (peq[sx2_peq_at(ch, lane & (SX2_GROUP - 1), w)] != (scans[lane] ? lev_filter_peq_word(np[lane], n[lane], 2, ch, w) : 0u)) return 11;

    const uint64_t wg0 = (uint64_t)h0 + (uint64_t)bx * hpw, wg1 = wg0 + hpw < h1 ? wg0 + hpw : h1;
    for (uint32_t wave = 0; wave < SX_WAVES; wave++) {
        for (uint32_t it = 0;; it++) {
            if (wg0 + sx_local_hay(it, wave, S, 0) >= wg1) break;
            for (uint32_t lane = 0; lane < 64; lane++) {          // (lane order = the ballot's prefix order)
                const uint32_t col = lane & (G - 1), slot = lane / G, column = lane & (SX2_GROUP - 1);
                const uint64_t hi = wg0 + sx_local_hay(it, wave, S, slot);
                if (!has[lane] || hi >= wg1) continue;
                uint32_t first = 0, last = 0;
                sx2_scan_pair<TRANS>(c.hs.ptr((uint32_t)hi), c.hs.len((uint32_t)hi), [&](uint32_t ch, uint32_t (&Eq)[2]) {
                    Eq[0] = peq[sx2_peq_at(ch, column, 0)]; Eq[1] = peq[sx2_peq_at(ch, column, 1)];
                }, n[lane], c.kf, first, last);
                const uint32_t needle = g0 + col;
                if (c.spans) {
                    uint32_t *sp = c.spans + 2 * ((uint64_t)hi * c.nn + needle);
                    if (sp[0] != 0xFFFFFFFFu) return 12;           // a pair the scan meets twice
                    sp[0] = first; sp[1] = last;
                }
                if (!first) continue;
                if (c.n_rec >= c.rec.size()) return 13;            // the list outgrows its sub-batch's room
                c.rec[c.n_rec++] = SxRec{(uint32_t)hi, needle, first, last, TA_NONE};
            }
        }
    }
    return 0;
}

// the exact pass over the sub-batch's records (scan: the list; anchored: one per (haystack, needle)), then the finish pass.  Record idx is
// taken by resident lane idx mod col_lanes, as the persistent grid strides.  Returns 0, or what went wrong.
template <bool TRANS>
int exact_and_finish(Call &c, uint32_t h0, uint32_t h1, bool listed) {
    const uint64_t n_work = listed ? c.n_rec : (uint64_t)(h1 - h0) * c.nn;
    const uint64_t lanes = c.col_lanes;
    for (uint64_t idx = 0; idx < n_work; idx++) {
        SxRec r = {0u, 0u, 1u, 0u, TA_NONE};
        if (listed) r = c.rec[idx];
        else { r.hay = h0 + (uint32_t)(idx / c.nn); r.needle = (uint32_t)(idx % c.nn); }
        ta_match m = {0, 0, TA_NONE, 0u};
        const uint64_t nl = c.nd.len(r.needle);
        const uint32_t n = nl < (uint64_t)SX2_MAX_NEEDLE ? (uint32_t)nl : SX2_MAX_NEEDLE;
        const uint64_t lane = idx % lanes;
        if ((6ull * (n + 1) - 1) * lanes + lane >= c.col.size()) return 14;     // the column's last element lies outside the scratch
        for (uint64_t e = 0; e < SX2_COL_WORDS; e++) c.col[e * lanes + lane] = 0xDEADBEEFu;   // (what an earlier pair left there)
        const uint32_t n_matches = sx2_exact_pair<TRANS>(c.hs.ptr(r.hay), c.hs.len(r.hay), c.nd.ptr(r.needle), n, c.C, listed, r.a, r.b, c.halo,
                                                  c.col.data() + lane, lanes, m);
        const bool hit = n_matches != 0;
        c.rec[idx] = SxRec{r.hay, r.needle, (uint32_t)m.start, (uint32_t)m.end, hit ? m.k : TA_NONE};
        if (!hit) continue;
        const uint64_t at = (*c.count)++;
        if (at < c.cap) c.hits[at] = ta_search_cross_hit{r.hay, r.needle, (uint32_t)m.start, (uint32_t)m.end, m.k, n_matches};
        if (c.nearest && sx_word(m.k, r.needle) < c.nearest[r.hay]) c.nearest[r.hay] = sx_word(m.k, r.needle);
        if (c.per_haystack) c.per_haystack[r.hay]++;
    }
    if (c.best && c.nearest)
        for (uint64_t idx = 0; idx < n_work; idx++) {
            const SxRec &r = c.rec[idx];
            if (sx_wins(r, c.nearest[r.hay])) c.best[r.hay] = ta_match{r.a, r.b, r.k, 0u};
        }
    return 0;
}

}  // namespace

// The whole call over CSR sides (n + 1 offsets each), always on the two-word route (the library takes it when the longest needle is
// beyond 32 bytes; it is valid for any panel of needles up to 64).  forced_sub: TA_SEARCH_CROSS_SUB, 0 = the budget's.  nearest / best /
// per_haystack: nh entries or NULL (best without nearest: the emulation keeps its own words, as the library does).  spans: 2 nn nh words
// preset to all ones -- [2 (i nn + p)] = the scanned span of the pair -- or NULL.  *n_subs: the sub-batches taken.  Returns 0, or a code
// that names what the emulation caught.
extern "C" int emu_search_cross_w2(const uint8_t *nblob, const uint64_t *noff, uint32_t nn, const uint8_t *hblob, const uint64_t *hoff, uint32_t nh,
                                   uint32_t k, uint32_t mc, uint32_t gc, uint32_t sg, int has_t, uint32_t tc, int anchored,
                                   uint32_t forced_sub, ta_search_cross_hit *hits, uint64_t *count, uint64_t cap, uint64_t *nearest, ta_match *best,
                                   uint32_t *per_haystack, uint32_t *spans, uint32_t *n_subs) {
    Call c;
    c.nd = Side{nblob, noff}; c.hs = Side{hblob, hoff};
    c.nn = nn; c.nh = nh;
    c.C = SearchCosts{k, mc, gc, sg, has_t ? tc : 0u, anchored ? 1u : 0u};
    c.trans = has_t != 0;
    c.kf = lev_is_unit(mc, gc, sg, has_t != 0, tc) ? k : srch_filter_k(k, mc, gc, sg, has_t != 0, tc);
    c.max_needle = 0;
    for (uint32_t p = 0; p < nn; p++)
        if (c.nd.len(p) > c.max_needle) c.max_needle = (uint32_t)c.nd.len(p);
    if (c.max_needle > SX2_MAX_NEEDLE) return 1;
    const uint64_t halo = (uint64_t)c.max_needle + c.kf + 2;
    c.halo = halo > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)halo;
    c.hits = hits; c.count = count; c.cap = cap; c.best = best; c.per_haystack = per_haystack; c.spans = spans;
    std::vector<uint64_t> own_nearest;
    if (!nearest && best) { own_nearest.resize(nh); nearest = own_nearest.data(); }
    c.nearest = nearest;
    *count = 0;
    *n_subs = 0;
    for (uint32_t i = 0; i < nh; i++) {
        if (nearest) nearest[i] = ~0ull;
        if (per_haystack) per_haystack[i] = 0;
        if (best) best[i] = ta_match{0, 0, TA_NONE, 0u};
    }
    if (nn == 0 || nh == 0) return 0;
    const SxPlan plan = sx_plan(nn, nh, forced_sub, SX2_GROUP);
    if (plan.groups != (nn + SX2_GROUP - 1) / SX2_GROUP) return 2;
    if (plan.sub == 0 || plan.hpw == 0 || (plan.sub < nh && plan.sub % plan.hpw) || (uint64_t)plan.sub * nn * sizeof(SxRec) > SX_BUDGET) return 2;
    c.rec.resize((size_t)plan.sub * nn);
    c.col_lanes = sx2_exact_lanes((uint64_t)plan.sub * nn);
    if (c.col_lanes == 0 || c.col_lanes % 256 || (uint64_t)c.col_lanes * SX2_COL_WORDS * 4 > SX_BUDGET) return 3;
    c.col.resize((size_t)c.col_lanes * SX2_COL_WORDS);
    for (uint64_t h0 = 0; h0 < nh; h0 += plan.sub) {
        const uint32_t h1 = (uint32_t)(h0 + plan.sub < nh ? h0 + plan.sub : nh);
        ++*n_subs;
        c.n_rec = 0;
        if (!anchored) {
            const uint32_t gx = (h1 - (uint32_t)h0 + plan.hpw - 1) / plan.hpw;
            for (uint32_t group = 0; group < plan.groups; group++)
                for (uint32_t bx = 0; bx < gx; bx++) {
                    const int rc = c.trans ? scan_workgroup<true>(c, bx, group, (uint32_t)h0, h1, plan.hpw)
                                           : scan_workgroup<false>(c, bx, group, (uint32_t)h0, h1, plan.hpw);
                    if (rc) return rc;
                }
        }
        if (const int rc = c.trans ? exact_and_finish<true>(c, (uint32_t)h0, h1, !anchored) : exact_and_finish<false>(c, (uint32_t)h0, h1, !anchored)) return rc;
    }
    return 0;
}

// the exact pass's resident lanes for `work` records and the cap on them (the host rule, for the tests)
extern "C" uint32_t emu_search_cross_w2_lanes(uint64_t work) { return sx2_exact_lanes(work); }
