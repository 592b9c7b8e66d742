// ta_search_batch.hip -- ta_levenshtein_search_batch and ta_hamming_search_batch (include/triple_accel_amd.h):
// validation, route choice, thread scratch and the launches of lev_search_batch.hip / ham_search_batch.hip.  Everything is enqueued on
// the caller's stream; with every length bound given (strided sides, or CSR max_len) there is no synchronisation and the call can be
// captured into a graph.  The shared host rules (cost check, length bounds, measured maxima, length order) and the scratch slots' names
// (SLOT_SB_*) are those of ta_internal.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lev_search_batch_body.h"
#include "ta_internal.h"

namespace ta {

// the checks both entries share, in their order: pointers and sizes, then the length bounds that are known without measuring
static int sb_check_args(const ta_strings *needles, const ta_strings *haystacks, size_t n, int search_type, const ta_match *matches_dev,
                         const uint32_t *counts_dev, size_t cap) {
    if (!needles || !haystacks || (search_type != TA_SEARCH_ALL && search_type != TA_SEARCH_BEST) || n > 0xFFFFFFF0ull) {
        set_last_error_msg("bad search batch arguments");
        return TA_ERR_ARG;
    }
    if (n && (!needles->blob || !haystacks->blob || !counts_dev || (cap && !matches_dev))) { set_last_error_msg("null buffer"); return TA_ERR_ARG; }
    if (cap && n > SIZE_MAX / sizeof(ta_match) / cap) { set_last_error_msg("n * cap overflows"); return TA_ERR_ARG; }
    if (side_bound_known(needles) && side_bound(needles) > 0xFFFFu) { set_last_error_msg("needle longer than 65535 bytes"); return TA_ERR_ARG; }
    if (side_bound_known(haystacks) && side_bound(haystacks) >> 32) { set_last_error_msg("haystack of 2^32 bytes or more"); return TA_ERR_UNSUPPORTED; }
    return device_ready() ? TA_OK : TA_ERR_HIP;
}

// the longest needle and haystack (measure_max_lens: one synchronisation where a CSR side gives no max_len), under the same two limits
static int sb_max_lens(const ta_strings *nd, const ta_strings *hs, uint32_t n, hipStream_t st, uint64_t *mn, uint64_t *mh) {
    unsigned long long *dst = nullptr;
    if (!side_bound_known(nd) || !side_bound_known(hs)) {
        Scratch &c = tls_scratch(SLOT_SB_CTL);
        if (int rc = c.ensure(64)) return rc;
        dst = (unsigned long long *)c.dev + 2;
    }
    if (int rc = measure_max_lens(nd, n, hs, n, dst, st, mn, mh)) return rc;
    if (*mn > 0xFFFFu) { set_last_error_msg("needle longer than 65535 bytes"); return TA_ERR_ARG; }
    if (*mh >> 32) { set_last_error_msg("haystack of 2^32 bytes or more"); return TA_ERR_UNSUPPORTED; }
    return TA_OK;
}

// CSR haystacks: the pairs longest haystack first, so that a wavefront's lanes finish together (order_pairs with this file's own slots)
static int sb_order(const ta_strings *hs, size_t n, uint64_t max_h, hipStream_t st, const uint32_t **order) {
    if (!lev_wants_length_order(hs->off != nullptr, n, max_h)) return TA_OK;
    return order_pairs(hs, hs, (uint32_t)n, 0u, max_h, false, false, SLOT_SB_ORDER, SLOT_SB_BINS, st, order, nullptr);
}

}  // namespace ta

using namespace ta;

extern "C" {

int ta_levenshtein_search_batch(const ta_strings *needles, const ta_strings *haystacks, size_t n,
                                uint32_t k, int search_type, const ta_edit_costs *costs, int anchored,
                                ta_match *matches_dev, uint32_t *counts_dev, size_t cap, void *stream) {
    if (!costs) { set_last_error_msg("null costs"); return TA_ERR_ARG; }
    if (!costs_ok(costs) || ta_edit_costs_check_search(costs) != TA_OK) return TA_ERR_BAD_COSTS;   // EditCosts::new; :1965, for the whole batch
    int rc = sb_check_args(needles, haystacks, n, search_type, matches_dev, counts_dev, cap);
    if (rc) return rc;
    if (n == 0) return TA_OK;
    const bool shared = !needles->off && needles->stride == 0;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    uint64_t max_n = 0, max_h = 0;
    if ((rc = sb_max_lens(needles, haystacks, (uint32_t)n, st, &max_n, &max_h))) return rc;

    SearchBatchParams P = {};
    P.nd = view_of(needles); P.hs = view_of(haystacks);
    P.matches = matches_dev; P.counts = counts_dev; P.cap = cap; P.n = (uint32_t)n;
    P.k = k; P.mc = costs->mismatch_cost; P.gc = costs->gap_cost; P.sg = costs->start_gap_cost;
    P.tc = costs->has_transpose ? costs->transpose_cost : 0;
    P.anchored = anchored ? 1u : 0u; P.best = search_type == TA_SEARCH_BEST ? 1u : 0u;
    P.max_needle = (uint32_t)max_n;
    const bool trans = costs->has_transpose != 0;
    const bool unit = costs_unit(costs);
    // Route S: a shared needle of up to 64 bytes, the scan's threshold below its length (else every end is a candidate) -- the single-haystack
    // filter's conditions and threshold (ta_search.hip)
    const uint32_t kf = unit ? k : srch_filter_k(k, P.mc, P.gc, P.sg, trans, P.tc);
    const bool route_s = shared && max_n >= 1 && max_n <= 64 && !anchored && kf < max_n && !env_int("TA_SEARCH_BATCH_NO_SCAN");
    // the packed form needs N == every needle's length (a shared or strided side) and every cost and length within 16 bits over the
    // columns a lane visits -- the longest haystack's (lev_search_tile_packed, srch_anchored_packed_ok)
    const uint32_t unit_k = lev_sat_sub(k, P.sg) / P.gc;
    const uint64_t cols = anchored ? (max_h < max_n + unit_k ? max_h : max_n + unit_k) : max_h;
    bool packed = !needles->off && max_n >= 1 && max_n <= 32 && k <= 30000u && cols <= 60000u && !env_int("TA_SEARCH_BATCH_UNPACKED");
    if (anchored) packed = packed && srch_anchored_packed_ok(cols, (uint32_t)max_n, P.mc, P.gc, P.sg);

    uint32_t mem_lanes = 0;
    if (max_n > 32) {                  // memory-backed column: one per resident lane (256 CUs x 32 waves x 64), at most ~256 MB of them
        const uint64_t per_lane = 6ull * (max_n + 1) * 4ull;
        uint64_t lanes = (256ull << 20) / per_lane;
        if (lanes > 524288) lanes = 524288;
        if (lanes > n) lanes = n;
        if (lanes < 64) lanes = 64;
        lanes = (lanes + 255) / 256 * 256;
        Scratch &cs = tls_scratch(SLOT_SB_COL);
        if ((rc = cs.ensure((size_t)(per_lane * lanes)))) return rc;
        P.col = (uint32_t *)cs.dev;
        mem_lanes = (uint32_t)lanes;
    }
    if (route_s) {
        Scratch &ctl = tls_scratch(SLOT_SB_CTL), &ls = tls_scratch(SLOT_SB_LIST), &sp = tls_scratch(SLOT_SB_SPAN);
        if ((rc = ctl.ensure(64)) || (rc = ls.ensure((size_t)n * 4)) || (rc = sp.ensure((size_t)n * 8))) return rc;
        P.cand_count = (uint32_t *)ctl.dev;
        P.cand_list = (uint32_t *)ls.dev;
        P.span = (uint32_t *)sp.dev;
        P.kf = kf;
        P.halo = (uint32_t)max_n + kf + 2;
        TA_HIP(fill_u32_launch(P.cand_count, 0u, 1, st));
        TA_HIP(search_batch_scan_launch(P, trans, st));
        P.list = P.cand_list;
        P.n_list = P.cand_count;
        TA_HIP(search_batch_exact_launch(P, trans, packed, mem_lanes, st));
        set_last_kernel_name("lev_search_batch_scan_kernel<%d, %s>", max_n <= 32 ? 1 : 2, trans ? "true" : "false");
        return TA_OK;
    }
    if ((rc = sb_order(haystacks, n, max_h, st, &P.list))) return rc;
    TA_HIP(search_batch_exact_launch(P, trans, packed, mem_lanes, st));
    return TA_OK;
}

int ta_hamming_search_batch(const ta_strings *needles, const ta_strings *haystacks, size_t n,
                            uint32_t k, int search_type, ta_match *matches_dev, uint32_t *counts_dev, size_t cap, void *stream) {
    int rc = sb_check_args(needles, haystacks, n, search_type, matches_dev, counts_dev, cap);
    if (rc) return rc;
    if (n == 0) return TA_OK;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    uint64_t max_n = 0, max_h = 0;
    if ((rc = sb_max_lens(needles, haystacks, (uint32_t)n, st, &max_n, &max_h))) return rc;

    HamBatchParams P = {};
    P.nd = view_of(needles); P.hs = view_of(haystacks);
    P.matches = matches_dev; P.counts = counts_dev; P.cap = cap; P.n = (uint32_t)n;
    P.k = k; P.best = search_type == TA_SEARCH_BEST ? 1u : 0u;
    P.max_needle = (uint32_t)max_n;
    // the bit-sliced form: one needle for every pair, 1..32 bytes, k at most a quarter of its length (so k <= 8: at most four counter
    // planes).  A window that passes the counters is recounted from memory, so the form is kept to thresholds where such windows are
    // rare whatever the alphabet; beyond, the general route counts every window exactly in registers
    const bool shared = !needles->off && needles->stride == 0;
    const bool bits = shared && max_n >= 1 && max_n <= 32 && 4ull * k <= max_n && !env_int("TA_HSEARCH_BATCH_GENERAL");
    if ((rc = sb_order(haystacks, n, max_h, st, &P.list))) return rc;
    TA_HIP(ham_search_batch_launch(P, bits, st));
    return TA_OK;
}

}  // extern "C"
