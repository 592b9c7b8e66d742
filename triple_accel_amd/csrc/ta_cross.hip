// ta_cross.hip -- ta_levenshtein_cross and ta_hamming_cross (include/triple_accel_amd.h): validation, the length
// bounds, the query tile and the launch of lev_cross.hip / ham_cross.hip.  Everything is enqueued on the caller's stream; with every length bound given (strided sides, or CSR max_len)
// there is no synchronisation and the call can be captured into a graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ta_internal.h"

namespace ta {

static constexpr int CROSS_CTL = 30;

static StrView cross_view(const ta_strings *s) { return StrView{s->blob, s->off, s->stride, s->len}; }
static bool cross_bound_known(const ta_strings *s) { return !s->off || s->max_len; }
static uint64_t cross_bound(const ta_strings *s) { return s->off ? s->max_len : s->len; }

// the longest query and target: given (CSR max_len), implied (strided) or measured on the device (one synchronisation for both)
static int cross_max_lens(const ta_strings *qs, uint32_t nq, const ta_strings *ts, uint32_t nt, hipStream_t st, uint64_t *mq, uint64_t *mt) {
    *mq = cross_bound(qs);
    *mt = cross_bound(ts);
    const bool need_q = !cross_bound_known(qs), need_t = !cross_bound_known(ts);
    if (!need_q && !need_t) return TA_OK;
    Scratch &c = tls_scratch(CROSS_CTL);
    int rc = c.ensure(64);
    if (rc) return rc;
    unsigned long long *d = (unsigned long long *)c.dev;
    TA_HIP(fill_u32_launch((uint32_t *)d, 0u, 4, st));
    const StrView none = {nullptr, nullptr, 0, 0};
    if (need_q) TA_HIP(search_batch_maxlen_launch(cross_view(qs), none, nq, d, st));
    if (need_t) TA_HIP(search_batch_maxlen_launch(none, cross_view(ts), nt, d, st));
    unsigned long long host[2] = {0, 0};
    TA_HIP(hipMemcpyAsync(host, d, 16, hipMemcpyDeviceToHost, st));
    TA_HIP(hipStreamSynchronize(st));
    if (need_q) *mq = host[0];
    if (need_t) *mt = host[1];
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
    {                                                                              // EditCosts::new, src/levenshtein.rs:44-52
        ta_edit_costs t;
        if (ta_edit_costs_new(costs->mismatch_cost, costs->gap_cost, costs->start_gap_cost, costs->has_transpose, costs->transpose_cost, &t) != TA_OK)
            return TA_ERR_BAD_COSTS;
    }
    const bool trans = costs->has_transpose != 0;
    const uint32_t mc = costs->mismatch_cost, gc = costs->gap_cost, sg = costs->start_gap_cost, tc = costs->transpose_cost;
    uint32_t g = lev_unit_scale(mc, gc, sg, trans, tc);
    if (!g && mc == 1 && gc == 1 && sg == 0 && (!trans || tc == 1)) g = 1;        // LEVENSHTEIN_COSTS / RDAMERAU_COSTS
    if (!g) { set_last_error_msg("cross: unit-cost families and their multiples only"); return TA_ERR_UNSUPPORTED; }
    if ((uint64_t)nq >> 32 || (uint64_t)nt >> 32) { set_last_error_msg("2^32 or more queries / targets"); return TA_ERR_ARG; }
    if (nq && nt && (!queries->blob || !targets->blob)) { set_last_error_msg("null blob"); return TA_ERR_ARG; }
    if (cap && !hits_dev) { set_last_error_msg("cap > 0 with null hits_dev"); return TA_ERR_ARG; }
    if (cap > SIZE_MAX / sizeof(ta_cross_hit)) { set_last_error_msg("cap * sizeof(ta_cross_hit) overflows"); return TA_ERR_ARG; }
    if (cross_bound_known(queries) && cross_bound(queries) > 64) { set_last_error_msg("cross: a query longer than 64 bytes"); return TA_ERR_UNSUPPORTED; }
    if (cross_bound_known(targets) && cross_bound(targets) >> 32) { set_last_error_msg("cross: a target of 2^32 bytes or more"); return TA_ERR_UNSUPPORTED; }
    if (!device_ready()) return TA_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    int rc;
    if (nq == 0 || nt == 0) {
        if ((rc = cross_fill64(count_dev, 0u, 1, st))) return rc;
        if (nearest_dev && (rc = cross_fill64((unsigned long long *)nearest_dev, 0xFFFFFFFFu, nq, st))) return rc;
        return TA_OK;
    }
    uint64_t max_q = 0, max_t = 0;
    if ((rc = cross_max_lens(queries, (uint32_t)nq, targets, (uint32_t)nt, st, &max_q, &max_t))) return rc;
    if (max_q > 64) { set_last_error_msg("cross: a query longer than 64 bytes"); return TA_ERR_UNSUPPORTED; }
    if (max_t >> 32) { set_last_error_msg("cross: a target of 2^32 bytes or more"); return TA_ERR_UNSUPPORTED; }

    CrossParams P = {};
    P.q = cross_view(queries); P.t = cross_view(targets);
    P.nq = (uint32_t)nq; P.nt = (uint32_t)nt;
    P.k = k / g; P.g = g;
    P.hits = hits_dev; P.cap = cap; P.count = count_dev; P.nearest = (unsigned long long *)nearest_dev;
    // The query tile: a wavefront keeps its 64 targets' lengths, pointers and first 16 bytes across the tile, so a longer tile amortises
    // them further; a shorter one makes more wavefronts.  Long enough to leave about 16,384 wavefronts (8 per SIMD of 256 CUs, twice
    // over), within [CROSS_MIN_QTILE, 512], and never more than 65,535 tiles (the grid's y dimension).
    const uint64_t tgroups = ((uint64_t)nt + 63) / 64;
    uint64_t qtile = (nq * tgroups + 16383) / 16384;
    if (qtile < CROSS_MIN_QTILE) qtile = CROSS_MIN_QTILE;
    if (qtile > 512) qtile = 512;
    if (const int f = env_int("TA_CROSS_QTILE"); f > 0) qtile = (uint64_t)f;
    if ((nq + qtile - 1) / qtile > 65535) qtile = (nq + 65534) / 65535;
    P.qtile = (uint32_t)qtile;
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
    if ((uint64_t)nq >> 32 || (uint64_t)nt >> 32) { set_last_error_msg("2^32 or more queries / targets"); return TA_ERR_ARG; }
    if (nq && nt && (!queries->blob || !targets->blob)) { set_last_error_msg("null blob"); return TA_ERR_ARG; }
    if (cap && !hits_dev) { set_last_error_msg("cap > 0 with null hits_dev"); return TA_ERR_ARG; }
    if (cap > SIZE_MAX / sizeof(ta_cross_hit)) { set_last_error_msg("cap * sizeof(ta_cross_hit) overflows"); return TA_ERR_ARG; }
    if (cross_bound_known(queries) && cross_bound(queries) > 64) { set_last_error_msg("cross: a query longer than 64 bytes"); return TA_ERR_UNSUPPORTED; }
    if (cross_bound_known(targets) && cross_bound(targets) >> 32) { set_last_error_msg("cross: a target of 2^32 bytes or more"); return TA_ERR_UNSUPPORTED; }
    if (!device_ready()) return TA_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    int rc;
    if ((rc = cross_fill64(count_dev, 0u, 1, st))) return rc;
    if (nearest_dev && (rc = cross_fill64((unsigned long long *)nearest_dev, 0xFFFFFFFFu, nq, st))) return rc;
    if (per_query_dev && nq) TA_HIP(fill_u32_launch(per_query_dev, 0u, (uint32_t)nq, st));
    if (nq == 0 || nt == 0) return TA_OK;
    uint64_t max_q = 0, max_t = 0;
    if ((rc = cross_max_lens(queries, (uint32_t)nq, targets, (uint32_t)nt, st, &max_q, &max_t))) return rc;
    if (max_q > 64) { set_last_error_msg("cross: a query longer than 64 bytes"); return TA_ERR_UNSUPPORTED; }
    if (max_t >> 32) { set_last_error_msg("cross: a target of 2^32 bytes or more"); return TA_ERR_UNSUPPORTED; }

    const int nw = max_q <= 16 ? 4 : max_q <= 32 ? 8 : 16;
    const uint64_t chunk = 256u / (uint32_t)nw;                                    // queries staged at a time (ham_cross_body.h)
    HamCrossParams P = {};
    P.q = cross_view(queries); P.t = cross_view(targets);
    P.nq = (uint32_t)nq; P.nt = (uint32_t)nt;
    P.k8 = 8u * (k < 64u ? k : 64u) + 7u;                                          // (no string is longer than 64 bytes: k above that changes nothing)
    P.upper = flags & TA_CROSS_UPPER;
    P.hits = hits_dev; P.cap = cap; P.count = count_dev; P.nearest = (unsigned long long *)nearest_dev; P.per_query = per_query_dev;
    // The query tile, as ta_levenshtein_cross sizes it: a wavefront loads its 64 targets once per tile, so a longer tile amortises them
    // further and a shorter one makes more wavefronts.  About 16,384 wavefronts, whole staging chunks, at most 512 queries, and never
    // more than 65,535 tiles (the grid's y dimension).
    const uint64_t tgroups = ((uint64_t)nt + 63) / 64;
    uint64_t qtile = (nq * tgroups + 16383) / 16384;
    qtile = (qtile + chunk - 1) / chunk * chunk;
    if (qtile > 512) qtile = 512;
    if (const int f = env_int("TA_HCROSS_QTILE"); f > 0) qtile = (uint64_t)f;
    if ((nq + qtile - 1) / qtile > 65535) qtile = (nq + 65534) / 65535;
    P.qtile = (uint32_t)qtile;
    TA_HIP(ham_cross_launch(P, nw, st));
    return TA_OK;
}
