// ta_cross.hip -- ta_levenshtein_cross, ta_levenshtein_cross_with_opts, ta_levenshtein_cross_tokens, ta_hamming_cross, ta_levenshtein_search_cross,
// ta_levenshtein_search_cross_with_opts, ta_hamming_search_cross and ta_hamming_search_cross_with_opts
// (include/triple_accel_amd.h): validation, the length bounds, the query tile / the sub-batches and the launches of
// lev_cross.hip / lev_cross_win.hip / lev_cross_tok.hip / ham_cross.hip / lev_search_cross.hip / lev_search_cross_w2.hip / ham_search_cross.hip /
// ham_search_cross_w2.hip.  Everything is enqueued on the caller's stream; with every length bound given (strided sides, or CSR max_len)
// there is no synchronisation and the call can be captured into a graph.  The shared host rules (cost check and scale, length bounds,
// measured maxima) and the scratch slots' names (SLOT_CROSS_CTL, SLOT_SX_*) are those of ta_internal.h; the query tile's rule is
// lev_plan.h's cross_qtile, the sub-batches' lev_search_cross_body.h's sx_plan.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ham_search_cross_w2_body.h"
#include "lev_cross_win_body.h"
#include "lev_search_cross_w2_body.h"
#include "ta_internal.h"

namespace ta {

// the checks the cross entries share, in their order: counts, pointers and sizes, then the length bounds that are known without measuring
// (max_query: the entry's limit on a query's length)
// the two length limits' messages (tokens: the sides of ta_levenshtein_cross_tokens, lengths in items)
static const char *cross_query_msg(uint32_t max_query, bool tokens) {
    return tokens ? "cross: a query longer than 64 tokens" : max_query > 64 ? "cross: a query longer than 256 bytes" : "cross: a query longer than 64 bytes";
}
static const char *cross_target_msg(bool tokens) { return tokens ? "cross: a target of 2^32 tokens or more" : "cross: a target of 2^32 bytes or more"; }

static int cross_check_args(const ta_strings *queries, size_t nq, const ta_strings *targets, size_t nt, const ta_cross_hit *hits_dev, size_t cap,
                            uint32_t max_query = 64, bool tokens = false) {
    if ((uint64_t)nq >> 32 || (uint64_t)nt >> 32) { set_last_error_msg("2^32 or more queries / targets"); return TA_ERR_ARG; }
    if (nq && nt && (!queries->blob || !targets->blob)) { set_last_error_msg(tokens ? "null data" : "null blob"); return TA_ERR_ARG; }
    if (cap && !hits_dev) { set_last_error_msg("cap > 0 with null hits_dev"); return TA_ERR_ARG; }
    if (cap > SIZE_MAX / sizeof(ta_cross_hit)) { set_last_error_msg("cap * sizeof(ta_cross_hit) overflows"); return TA_ERR_ARG; }
    if (side_bound_known(queries) && side_bound(queries) > max_query) { set_last_error_msg(cross_query_msg(max_query, tokens)); return TA_ERR_UNSUPPORTED; }
    if (side_bound_known(targets) && side_bound(targets) >> 32) { set_last_error_msg(cross_target_msg(tokens)); return TA_ERR_UNSUPPORTED; }
    return device_ready() ? TA_OK : TA_ERR_HIP;
}

// the longest query and target (measure_max_lens: one synchronisation where a CSR side gives no max_len), under the same two limits
static int cross_max_lens(const ta_strings *qs, uint32_t nq, const ta_strings *ts, uint32_t nt, hipStream_t st, uint64_t *mq, uint64_t *mt,
                          uint32_t max_query = 64, bool tokens = false) {
    unsigned long long *dst = nullptr;
    if (!side_bound_known(qs) || !side_bound_known(ts)) {
        Scratch &c = tls_scratch(SLOT_CROSS_CTL);
        if (int rc = c.ensure(64)) return rc;
        dst = (unsigned long long *)c.dev;
    }
    if (int rc = measure_max_lens(qs, nq, ts, nt, dst, st, mq, mt)) return rc;
    if (*mq > max_query) { set_last_error_msg(cross_query_msg(max_query, tokens)); return TA_ERR_UNSUPPORTED; }
    if (*mt >> 32) { set_last_error_msg(cross_target_msg(tokens)); return TA_ERR_UNSUPPORTED; }
    return TA_OK;
}

// p[0 .. n) = v for n 64-bit words whose halves are equal, by the graph-safe fill kernel
static int cross_fill64(unsigned long long *p, uint32_t half, uint64_t n, hipStream_t st) {
    uint32_t *w = (uint32_t *)p;
    for (uint64_t done = 0; done < 2 * n;) {
        const uint64_t part = 2 * n - done < 0x80000000ull ? 2 * n - done : 0x80000000ull;
        TA_HIP(fill_u32_launch(w + done, half, (uint32_t)part, st));
        done += part;
    }
    return TA_OK;
}

// the limits of the search cross entries over the counts and the length bounds known so far (0: not known yet); max_needle_limit: the
// entry's limit on a needle's length (32, or 64 for the two with_opts entries)
static int search_cross_limits(uint64_t nn, uint64_t nh, uint64_t max_needle, uint64_t max_hay, uint32_t max_needle_limit = SX_MAX_NEEDLE) {
    if (max_needle > max_needle_limit) {
        set_last_error_msg(max_needle_limit > SX_MAX_NEEDLE ? "search cross: a needle longer than 64 bytes" : "search cross: a needle longer than 32 bytes");
        return TA_ERR_UNSUPPORTED;
    }
    if (nn > 65535u) { set_last_error_msg("search cross: more than 65,535 needles"); return TA_ERR_UNSUPPORTED; }
    if (max_hay >> 32 || nh >> 32) { set_last_error_msg("search cross: a haystack of 2^32 bytes or more, or 2^32 or more haystacks"); return TA_ERR_UNSUPPORTED; }
    return TA_OK;
}

}  // namespace ta

using namespace ta;

extern "C" int ta_levenshtein_cross(const ta_strings *queries, size_t nq, const ta_strings *targets, size_t nt,
                                    uint32_t k, const ta_edit_costs *costs,
                                    ta_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                    uint64_t *nearest_dev, void *stream) {
    if (!queries || !targets || !costs || !count_dev) { set_last_error_msg("null queries / targets / costs / count_dev"); return TA_ERR_ARG; }
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;                                 // EditCosts::new, src/levenshtein.rs:44-52
    const bool trans = costs->has_transpose != 0;
    const uint32_t g = costs_scale(costs);                                         // LEVENSHTEIN_COSTS / RDAMERAU_COSTS: 1; g times one: g
    if (!g) { set_last_error_msg("cross: unit-cost families and their multiples only"); return TA_ERR_UNSUPPORTED; }
    int rc = cross_check_args(queries, nq, targets, nt, hits_dev, cap);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    if (nq == 0 || nt == 0) {
        if ((rc = cross_fill64(count_dev, 0u, 1, st))) return rc;
        if (nearest_dev && (rc = cross_fill64((unsigned long long *)nearest_dev, 0xFFFFFFFFu, nq, st))) return rc;
        return TA_OK;
    }
    uint64_t max_q = 0, max_t = 0;
    if ((rc = cross_max_lens(queries, (uint32_t)nq, targets, (uint32_t)nt, st, &max_q, &max_t))) return rc;

    CrossParams P = {};
    P.q = view_of(queries); P.t = view_of(targets);
    P.nq = (uint32_t)nq; P.nt = (uint32_t)nt;
    P.k = k / g; P.g = g;
    P.hits = hits_dev; P.cap = cap; P.count = count_dev; P.nearest = (unsigned long long *)nearest_dev;
    // The query tile: a wavefront keeps its 64 targets' lengths, pointers and first 16 bytes across the tile, so a longer tile amortises
    // them further; a shorter one makes more wavefronts (lev_plan.h: cross_qtile).
    P.qtile = cross_qtile(nq, nt, CROSS_MIN_QTILE, 1, env_int("TA_CROSS_QTILE"));
    if ((rc = cross_fill64(count_dev, 0u, 1, st))) return rc;
    if (nearest_dev && (rc = cross_fill64((unsigned long long *)nearest_dev, 0xFFFFFFFFu, nq, st))) return rc;
    TA_HIP(lev_cross_launch(P, max_q <= 32 ? 1 : 2, trans, st));
    return TA_OK;
}

extern "C" int ta_levenshtein_cross_with_opts(const ta_strings *queries, size_t nq, const ta_strings *targets, size_t nt,
                                              uint32_t k, const ta_edit_costs *costs, uint32_t flags,
                                              ta_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                              uint64_t *nearest_dev, uint32_t *per_query_dev, void *stream) {
    if (!queries || !targets || !costs || !count_dev) { set_last_error_msg("null queries / targets / costs / count_dev"); return TA_ERR_ARG; }
    if (flags & ~TA_CROSS_UPPER) { set_last_error_msg("levenshtein cross: unknown flag bits"); return TA_ERR_ARG; }
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;                                 // EditCosts::new, src/levenshtein.rs:44-52
    const bool trans = costs->has_transpose != 0;
    const uint32_t g = costs_scale(costs);                                         // LEVENSHTEIN_COSTS / RDAMERAU_COSTS: 1; g times one: g
    if (!g) { set_last_error_msg("cross: unit-cost families and their multiples only"); return TA_ERR_UNSUPPORTED; }
    int rc = cross_check_args(queries, nq, targets, nt, hits_dev, cap, WIN_MAX_QUERY);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    // a measured query of more than 256 bytes is refused before any output is written, as ta_levenshtein_cross does it
    uint64_t max_q = 0, max_t = 0;
    if (nq && nt && (rc = cross_max_lens(queries, (uint32_t)nq, targets, (uint32_t)nt, st, &max_q, &max_t, WIN_MAX_QUERY))) return rc;
    if ((rc = cross_fill64(count_dev, 0u, 1, st))) return rc;
    if (nearest_dev && (rc = cross_fill64((unsigned long long *)nearest_dev, 0xFFFFFFFFu, nq, st))) return rc;
    if (per_query_dev && nq) TA_HIP(fill_u32_launch(per_query_dev, 0u, (uint32_t)nq, st));
    if (nq == 0 || nt == 0) return TA_OK;

    CrossParams P = {};
    P.q = view_of(queries); P.t = view_of(targets);
    P.nq = (uint32_t)nq; P.nt = (uint32_t)nt;
    P.k = k / g; P.g = g;
    P.flags = flags;
    P.hits = hits_dev; P.cap = cap; P.count = count_dev; P.nearest = (unsigned long long *)nearest_dev; P.per_query = per_query_dev;
    P.qtile = cross_qtile(nq, nt, CROSS_MIN_QTILE, 1, env_int("TA_CROSS_QTILE"));   // ta_levenshtein_cross's tile
    // Up to 64 bytes: the whole column in one or two words (3.13).  Beyond: a window of the column, the smallest that holds the band of
    // P.k (3.17); TA_CROSS_FULL (tuning) takes the whole column instead.
    if (max_q <= 64) TA_HIP(lev_cross_launch(P, max_q <= 32 ? 1 : 2, trans, st));
    else TA_HIP(lev_cross_win_launch(P, env_int("TA_CROSS_FULL") ? (int)WIN_NB : win_ww(P.k), trans, st));
    return TA_OK;
}

// The sides of a token call as the byte entries' host rules read them: the same five fields, every length, stride and offset in ITEMS
// (measure_max_lens takes differences of offsets; a CSR side's `len`, the items `data` holds, plays no part here: side_bound reads max_len).
static ta_strings tokens_as_side(const ta_tokens *t) { return ta_strings{(const uint8_t *)t->data, t->off, t->stride, t->len, t->max_len}; }

extern "C" int ta_levenshtein_cross_tokens(const ta_tokens *queries, size_t nq, const ta_tokens *targets, size_t nt,
                                           uint32_t k, const ta_edit_costs *costs, uint32_t flags,
                                           ta_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                           uint64_t *nearest_dev, uint32_t *per_query_dev, void *stream) {
    if (!queries || !targets || !costs || !count_dev) { set_last_error_msg("null queries / targets / costs / count_dev"); return TA_ERR_ARG; }
    if (flags & ~TA_CROSS_UPPER) { set_last_error_msg("levenshtein cross tokens: unknown flag bits"); return TA_ERR_ARG; }
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;                                 // EditCosts::new, src/levenshtein.rs:44-52
    const bool trans = costs->has_transpose != 0;
    const uint32_t g = costs_scale(costs);                                         // LEVENSHTEIN_COSTS / RDAMERAU_COSTS: 1; g times one: g
    if (!g) { set_last_error_msg("cross: unit-cost families and their multiples only"); return TA_ERR_UNSUPPORTED; }
    const ta_strings qs = tokens_as_side(queries), ts = tokens_as_side(targets);
    int rc = cross_check_args(&qs, nq, &ts, nt, hits_dev, cap, 64, true);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    // a measured query of more than 64 tokens is refused before any output is written, as ta_levenshtein_cross_with_opts does it
    uint64_t max_q = 0, max_t = 0;
    if (nq && nt && (rc = cross_max_lens(&qs, (uint32_t)nq, &ts, (uint32_t)nt, st, &max_q, &max_t, 64, true))) return rc;
    if ((rc = cross_fill64(count_dev, 0u, 1, st))) return rc;
    if (nearest_dev && (rc = cross_fill64((unsigned long long *)nearest_dev, 0xFFFFFFFFu, nq, st))) return rc;
    if (per_query_dev && nq) TA_HIP(fill_u32_launch(per_query_dev, 0u, (uint32_t)nq, st));
    if (nq == 0 || nt == 0) return TA_OK;

    CrossParams P = {};
    P.q = view_of(&qs); P.t = view_of(&ts);                                        // (items: lev_cross_tok.hip scales by four)
    P.nq = (uint32_t)nq; P.nt = (uint32_t)nt;
    P.k = k / g; P.g = g;
    P.flags = flags;
    P.hits = hits_dev; P.cap = cap; P.count = count_dev; P.nearest = (unsigned long long *)nearest_dev; P.per_query = per_query_dev;
    P.qtile = cross_qtile(nq, nt, CROSS_MIN_QTILE, 1, env_int("TA_CROSS_QTILE"));   // ta_levenshtein_cross's tile
    TA_HIP(lev_cross_tok_launch(P, max_q <= 32 ? 1 : 2, trans, st));
    return TA_OK;
}

extern "C" int ta_hamming_cross(const ta_strings *queries, size_t nq, const ta_strings *targets, size_t nt,
                                uint32_t k, uint32_t flags,
                                ta_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                uint64_t *nearest_dev, uint32_t *per_query_dev, void *stream) {
    if (!queries || !targets || !count_dev) { set_last_error_msg("null queries / targets / count_dev"); return TA_ERR_ARG; }
    if (flags & ~TA_CROSS_UPPER) { set_last_error_msg("hamming cross: unknown flag bits"); return TA_ERR_ARG; }
    int rc = cross_check_args(queries, nq, targets, nt, hits_dev, cap);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    if ((rc = cross_fill64(count_dev, 0u, 1, st))) return rc;
    if (nearest_dev && (rc = cross_fill64((unsigned long long *)nearest_dev, 0xFFFFFFFFu, nq, st))) return rc;
    if (per_query_dev && nq) TA_HIP(fill_u32_launch(per_query_dev, 0u, (uint32_t)nq, st));
    if (nq == 0 || nt == 0) return TA_OK;
    uint64_t max_q = 0, max_t = 0;
    if ((rc = cross_max_lens(queries, (uint32_t)nq, targets, (uint32_t)nt, st, &max_q, &max_t))) return rc;

    const int nw = max_q <= 16 ? 4 : max_q <= 32 ? 8 : 16;
    const uint32_t chunk = 256u / (uint32_t)nw;                                    // queries staged at a time (ham_cross_body.h)
    HamCrossParams P = {};
    P.q = view_of(queries); P.t = view_of(targets);
    P.nq = (uint32_t)nq; P.nt = (uint32_t)nt;
    P.k8 = 8u * (k < 64u ? k : 64u) + 7u;                                          // (no string is longer than 64 bytes: k above that changes nothing)
    P.upper = flags & TA_CROSS_UPPER;
    P.hits = hits_dev; P.cap = cap; P.count = count_dev; P.nearest = (unsigned long long *)nearest_dev; P.per_query = per_query_dev;
    // The query tile, as ta_levenshtein_cross sizes it, in whole staging chunks (lev_plan.h: cross_qtile)
    P.qtile = cross_qtile(nq, nt, 0, chunk, env_int("TA_HCROSS_QTILE"));
    TA_HIP(ham_cross_launch(P, nw, st));
    return TA_OK;
}

// ta_levenshtein_search_cross and ta_levenshtein_search_cross_with_opts: one host path.  max_needle_limit: the entry's limit on a needle's
// length; flags: the reserved word of the with_opts entry (the other passes 0), checked right behind the NULL pointers.
static int search_cross_run(const ta_strings *needles, size_t nn, const ta_strings *haystacks, size_t nh,
                            uint32_t k, const ta_edit_costs *costs, int anchored, uint32_t flags, uint32_t max_needle_limit,
                            ta_search_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                            uint64_t *nearest_dev, ta_match *best_dev, uint32_t *per_haystack_dev, void *stream) {
    if (!costs || !needles || !haystacks || !count_dev) { set_last_error_msg("null costs / needles / haystacks / count_dev"); return TA_ERR_ARG; }
    if (flags) { set_last_error_msg("levenshtein search cross: unknown flag bits (the word is reserved: 0)"); return TA_ERR_ARG; }
    if (!costs_ok(costs) || ta_edit_costs_check_search(costs) != TA_OK) return TA_ERR_BAD_COSTS;   // EditCosts::new; :1965, for the whole call
    if (nn && nh && (!needles->blob || !haystacks->blob)) { set_last_error_msg("null blob"); return TA_ERR_ARG; }
    if (cap && !hits_dev) { set_last_error_msg("cap > 0 with null hits_dev"); return TA_ERR_ARG; }
    if (cap > SIZE_MAX / sizeof(ta_search_cross_hit)) { set_last_error_msg("cap * sizeof(ta_search_cross_hit) overflows"); return TA_ERR_ARG; }
    int rc = search_cross_limits(nn, nh, side_bound_known(needles) ? side_bound(needles) : 0, side_bound_known(haystacks) ? side_bound(haystacks) : 0,
                                 max_needle_limit);
    if (rc) return rc;
    if (!device_ready()) return TA_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    // the nearest words: the caller's, or the library's own when only best_dev is asked for
    unsigned long long *nearest = (unsigned long long *)nearest_dev;
    if (!nearest && best_dev && nh) {
        Scratch &ns = tls_scratch(SLOT_SX_NEAR);
        if ((rc = ns.ensure(nh * sizeof(unsigned long long)))) return rc;
        nearest = (unsigned long long *)ns.dev;
    }
    if ((rc = cross_fill64(count_dev, 0u, 1, st))) return rc;
    if (nearest && (rc = cross_fill64(nearest, 0xFFFFFFFFu, nh, st))) return rc;
    if (per_haystack_dev && nh) TA_HIP(fill_u32_launch(per_haystack_dev, 0u, (uint32_t)nh, st));
    if (best_dev) TA_HIP(search_cross_init_best_launch(best_dev, (uint32_t)nh, st));
    if (nn == 0 || nh == 0) return TA_OK;
    Scratch &ctl = tls_scratch(SLOT_SX_CTL);
    if ((rc = ctl.ensure(64))) return rc;
    uint64_t max_n = 0, max_h = 0;
    if ((rc = measure_max_lens(needles, (uint32_t)nn, haystacks, (uint32_t)nh, (unsigned long long *)ctl.dev + 2, st, &max_n, &max_h))) return rc;
    if ((rc = search_cross_limits(nn, nh, max_n, max_h, max_needle_limit))) return rc;

    SearchCrossParams P = {};
    P.nd = view_of(needles); P.hs = view_of(haystacks);
    P.nn = (uint32_t)nn;
    P.k = k; P.mc = costs->mismatch_cost; P.gc = costs->gap_cost; P.sg = costs->start_gap_cost;
    P.tc = costs->has_transpose ? costs->transpose_cost : 0;
    P.anchored = anchored ? 1u : 0u;
    P.max_needle = (uint32_t)max_n;
    const bool trans = costs->has_transpose != 0;
    // The route, once per call from the longest-needle bound: up to 32 bytes the one-word kernels (lev_search_cross.hip), beyond them the
    // two-word ones for the whole panel (lev_search_cross_w2.hip) -- groups of 32 needles, the exact pass's column in memory
    const bool w2 = max_n > SX_MAX_NEEDLE;
    // the scan's threshold and the packed form's conditions: ta_levenshtein_search_batch's (ta_search_batch.hip)
    P.kf = costs_unit(costs) ? k : srch_filter_k(k, P.mc, P.gc, P.sg, trans, P.tc);
    const uint64_t halo = max_n + P.kf + 2;                                             // (only needles with kf < n use it)
    P.halo = halo > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)halo;
    const uint32_t unit_k = lev_sat_sub(k, P.sg) / P.gc;
    const uint64_t cols = anchored ? (max_h < max_n + unit_k ? max_h : max_n + unit_k) : max_h;
    bool packed = !needles->off && max_n >= 1 && max_n <= 32 && k <= 30000u && cols <= 60000u && !env_int("TA_SEARCH_BATCH_UNPACKED");
    if (anchored) packed = packed && srch_anchored_packed_ok(cols, (uint32_t)max_n, P.mc, P.gc, P.sg);
    P.hits = hits_dev; P.cap = cap; P.count = count_dev; P.nearest = nearest; P.per_haystack = per_haystack_dev; P.best = best_dev;

    // Sub-batches of whole workgroups: the records of one stay within SX_BUDGET; their number depends on nn, nh and the budget only
    const int forced = env_int("TA_SEARCH_CROSS_SUB");
    const SxPlan plan = sx_plan(nn, nh, forced > 0 ? (uint64_t)forced : 0, w2 ? SX2_GROUP : SX_GROUP);
    Scratch &rs = tls_scratch(SLOT_SX_REC);
    if ((rc = rs.ensure((size_t)plan.sub * nn * sizeof(SxRec)))) return rc;
    P.rec = (SxRec *)rs.dev;
    if (w2) {                          // one memory-backed column per resident lane of the exact pass, within SX_BUDGET (from nn and nh alone)
        P.col_lanes = sx2_exact_lanes((uint64_t)plan.sub * nn);
        Scratch &cs = tls_scratch(SLOT_SX_COL);
        if ((rc = cs.ensure((size_t)P.col_lanes * SX2_COL_WORDS * sizeof(uint32_t)))) return rc;
        P.col = (uint32_t *)cs.dev;
    }
    P.hpw = plan.hpw;
    P.n_rec = anchored ? nullptr : (uint32_t *)ctl.dev;
    for (uint64_t h0 = 0; h0 < nh; h0 += plan.sub) {
        P.h0 = (uint32_t)h0;
        P.h1 = (uint32_t)(h0 + plan.sub < nh ? h0 + plan.sub : nh);
        if (!anchored) {
            TA_HIP(fill_u32_launch(P.n_rec, 0u, 1, st));
            TA_HIP(w2 ? search_cross_w2_scan_launch(P, trans, st) : search_cross_scan_launch(P, trans, st));
        }
        TA_HIP(w2 ? search_cross_w2_exact_launch(P, trans, st) : search_cross_exact_launch(P, trans, packed, st));
        TA_HIP(search_cross_finish_launch(P, st));
    }
    if (!anchored) set_last_kernel_name(w2 ? "lev_search_cross_w2_scan_kernel<%s>" : "lev_search_cross_scan_kernel<%s>", trans ? "true" : "false");
    return TA_OK;
}

extern "C" int ta_levenshtein_search_cross(const ta_strings *needles, size_t nn, const ta_strings *haystacks, size_t nh,
                                           uint32_t k, const ta_edit_costs *costs, int anchored,
                                           ta_search_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                           uint64_t *nearest_dev, ta_match *best_dev, uint32_t *per_haystack_dev, void *stream) {
    return search_cross_run(needles, nn, haystacks, nh, k, costs, anchored, 0u, SX_MAX_NEEDLE, hits_dev, count_dev, cap, nearest_dev, best_dev,
                            per_haystack_dev, stream);
}

extern "C" int ta_levenshtein_search_cross_with_opts(const ta_strings *needles, size_t nn, const ta_strings *haystacks, size_t nh,
                                                     uint32_t k, const ta_edit_costs *costs, int anchored, uint32_t flags,
                                                     ta_search_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                                     uint64_t *nearest_dev, ta_match *best_dev, uint32_t *per_haystack_dev, void *stream) {
    return search_cross_run(needles, nn, haystacks, nh, k, costs, anchored, flags, SX2_MAX_NEEDLE, hits_dev, count_dev, cap, nearest_dev, best_dev,
                            per_haystack_dev, stream);
}

// ta_hamming_search_cross and ta_hamming_search_cross_with_opts: one host path.  max_needle_limit: the entry's limit on a needle's length;
// flags: the reserved word of the with_opts entry (the other passes 0), checked right behind the NULL pointers.
static int ham_search_cross_run(const ta_strings *needles, size_t nn, const ta_strings *haystacks, size_t nh,
                                uint32_t k, uint32_t flags, uint32_t max_needle_limit,
                                ta_search_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                uint64_t *nearest_dev, ta_match *best_dev, uint32_t *per_haystack_dev, void *stream) {
    if (!needles || !haystacks || !count_dev) { set_last_error_msg("null needles / haystacks / count_dev"); return TA_ERR_ARG; }
    if (flags) { set_last_error_msg("hamming search cross: unknown flag bits (the word is reserved: 0)"); return TA_ERR_ARG; }
    if (nn && nh && (!needles->blob || !haystacks->blob)) { set_last_error_msg("null blob"); return TA_ERR_ARG; }
    if (cap && !hits_dev) { set_last_error_msg("cap > 0 with null hits_dev"); return TA_ERR_ARG; }
    if (cap > SIZE_MAX / sizeof(ta_search_cross_hit)) { set_last_error_msg("cap * sizeof(ta_search_cross_hit) overflows"); return TA_ERR_ARG; }
    int rc = search_cross_limits(nn, nh, side_bound_known(needles) ? side_bound(needles) : 0, side_bound_known(haystacks) ? side_bound(haystacks) : 0,
                                 max_needle_limit);
    if (rc) return rc;
    if (!device_ready()) return TA_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    if ((rc = cross_fill64(count_dev, 0u, 1, st))) return rc;
    if (per_haystack_dev && nh) TA_HIP(fill_u32_launch(per_haystack_dev, 0u, (uint32_t)nh, st));
    if (nn == 0 || nh == 0) {
        if (nearest_dev && (rc = cross_fill64((unsigned long long *)nearest_dev, 0xFFFFFFFFu, nh, st))) return rc;
        if (best_dev) TA_HIP(search_cross_init_best_launch(best_dev, (uint32_t)nh, st));
        return TA_OK;
    }
    Scratch &ctl = tls_scratch(SLOT_HSX_CTL);
    if ((rc = ctl.ensure(64))) return rc;
    uint64_t max_n = 0, max_h = 0;
    if ((rc = measure_max_lens(needles, (uint32_t)nn, haystacks, (uint32_t)nh, (unsigned long long *)ctl.dev, st, &max_n, &max_h))) return rc;
    if ((rc = search_cross_limits(nn, nh, max_n, max_h, max_needle_limit))) return rc;

    HamSearchCrossParams P = {};
    P.nd = view_of(needles); P.hs = view_of(haystacks);
    P.nn = (uint32_t)nn; P.nh = (uint32_t)nh;
    P.kc = hsx_threshold(k, (uint32_t)max_n);
    P.hits = hits_dev; P.cap = cap; P.count = count_dev; P.per_haystack = per_haystack_dev;
    P.nearest = (unsigned long long *)nearest_dev; P.best = best_dev;
    // the packed nearest words: every haystack's minimum over its hits, unpacked into nearest_dev / best_dev by the finish kernel
    if (nearest_dev || best_dev) {
        Scratch &ws = tls_scratch(SLOT_HSX_WORD);
        if ((rc = ws.ensure(nh * sizeof(unsigned long long)))) return rc;
        P.packed = (unsigned long long *)ws.dev;
        if ((rc = cross_fill64(P.packed, 0xFFFFFFFFu, nh, st))) return rc;
    }
    // The route, once per call from the longest-needle bound: up to 32 bytes the one-word kernel (ham_search_cross.hip), beyond them the
    // two-word one for the whole panel (ham_search_cross_w2.hip) -- groups of 32 needles, two haystacks or more per wavefront step
    const bool w2 = max_n > SX_MAX_NEEDLE;
    const int forced = env_int("TA_HSEARCH_CROSS_HPW");
    P.hpw = hsx_hpw(nn, nh, forced > 0 ? (uint64_t)forced : 0, w2 ? HSX2_GROUP : SX_GROUP, w2 ? HSX2_MIN_HPW : SX_WAVES);
    // (names the kernel: ham_search_cross_kernel<B> / ham_search_cross_w2_kernel<B>)
    TA_HIP(w2 ? ham_search_cross_w2_launch(P, st) : ham_search_cross_launch(P, st));
    TA_HIP(ham_search_cross_finish_launch(P, st));
    return TA_OK;
}

extern "C" int ta_hamming_search_cross(const ta_strings *needles, size_t nn, const ta_strings *haystacks, size_t nh,
                                       uint32_t k,
                                       ta_search_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                       uint64_t *nearest_dev, ta_match *best_dev, uint32_t *per_haystack_dev, void *stream) {
    return ham_search_cross_run(needles, nn, haystacks, nh, k, 0u, SX_MAX_NEEDLE, hits_dev, count_dev, cap, nearest_dev, best_dev, per_haystack_dev,
                                stream);
}

extern "C" int ta_hamming_search_cross_with_opts(const ta_strings *needles, size_t nn, const ta_strings *haystacks, size_t nh,
                                                 uint32_t k, uint32_t flags,
                                                 ta_search_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                                 uint64_t *nearest_dev, ta_match *best_dev, uint32_t *per_haystack_dev, void *stream) {
    return ham_search_cross_run(needles, nn, haystacks, nh, k, flags, HSX2_MAX_NEEDLE, hits_dev, count_dev, cap, nearest_dev, best_dev,
                                per_haystack_dev, stream);
}
