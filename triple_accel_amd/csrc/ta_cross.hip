// ta_cross.hip -- ta_levenshtein_cross and ta_hamming_cross (include/triple_accel_amd.h): validation, the length
// bounds, the query tile and the launch of lev_cross.hip / ham_cross.hip.  Everything is enqueued on the caller's stream; with every length bound given (strided sides, or CSR max_len)
// there is no synchronisation and the call can be captured into a graph.  The shared host rules (cost check and scale, length bounds,
// measured maxima) and the scratch slot's name (SLOT_CROSS_CTL) are those of ta_internal.h; the query tile's rule is lev_plan.h's cross_qtile.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ta_internal.h"

namespace ta {

// the checks both entries share, in their order: counts, pointers and sizes, then the length bounds that are known without measuring
static int cross_check_args(const ta_strings *queries, size_t nq, const ta_strings *targets, size_t nt, const ta_cross_hit *hits_dev, size_t cap) {
    if ((uint64_t)nq >> 32 || (uint64_t)nt >> 32) { set_last_error_msg("2^32 or more queries / targets"); return TA_ERR_ARG; }
    if (nq && nt && (!queries->blob || !targets->blob)) { set_last_error_msg("null blob"); return TA_ERR_ARG; }
    if (cap && !hits_dev) { set_last_error_msg("cap > 0 with null hits_dev"); return TA_ERR_ARG; }
    if (cap > SIZE_MAX / sizeof(ta_cross_hit)) { set_last_error_msg("cap * sizeof(ta_cross_hit) overflows"); return TA_ERR_ARG; }
    if (side_bound_known(queries) && side_bound(queries) > 64) { set_last_error_msg("cross: a query longer than 64 bytes"); return TA_ERR_UNSUPPORTED; }
    if (side_bound_known(targets) && side_bound(targets) >> 32) { set_last_error_msg("cross: a target of 2^32 bytes or more"); return TA_ERR_UNSUPPORTED; }
    return device_ready() ? TA_OK : TA_ERR_HIP;
}

// the longest query and target (measure_max_lens: one synchronisation where a CSR side gives no max_len), under the same two limits
static int cross_max_lens(const ta_strings *qs, uint32_t nq, const ta_strings *ts, uint32_t nt, hipStream_t st, uint64_t *mq, uint64_t *mt) {
    unsigned long long *dst = nullptr;
    if (!side_bound_known(qs) || !side_bound_known(ts)) {
        Scratch &c = tls_scratch(SLOT_CROSS_CTL);
        if (int rc = c.ensure(64)) return rc;
        dst = (unsigned long long *)c.dev;
    }
    if (int rc = measure_max_lens(qs, nq, ts, nt, dst, st, mq, mt)) return rc;
    if (*mq > 64) { set_last_error_msg("cross: a query longer than 64 bytes"); return TA_ERR_UNSUPPORTED; }
    if (*mt >> 32) { set_last_error_msg("cross: a target of 2^32 bytes or more"); return TA_ERR_UNSUPPORTED; }
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
