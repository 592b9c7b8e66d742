// ta_search_batch.hip -- ta_levenshtein_search_batch and ta_hamming_search_batch (include/triple_accel_amd.h):
// validation, route choice, thread scratch and the launches of lev_search_batch.hip / ham_search_batch.hip.  Everything is enqueued on
// the caller's stream; with every length bound given (strided sides, or CSR max_len) there is no synchronisation and the call can be
// captured into a graph.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lev_search_batch_body.h"
#include "ta_internal.h"

namespace ta {

static constexpr int SB_ORDER = 23, SB_BINS = 24, SB_CTL = 25, SB_LIST = 26, SB_SPAN = 27, SB_COL = 28;

static StrView sb_view(const ta_strings *s) { return StrView{s->blob, s->off, s->stride, s->len}; }

// the longest needle and haystack: given (CSR max_len), implied (strided) or measured on the device (one synchronisation for both)
static int sb_max_lens(const ta_strings *nd, const ta_strings *hs, uint32_t n, hipStream_t st, uint64_t *mn, uint64_t *mh) {
    *mn = nd->off ? nd->max_len : nd->len;
    *mh = hs->off ? hs->max_len : hs->len;
    const bool need_n = nd->off && !nd->max_len, need_h = hs->off && !hs->max_len;
    if (!need_n && !need_h) return TA_OK;
    Scratch &c = tls_scratch(SB_CTL);
    int rc = c.ensure(64);
    if (rc) return rc;
    unsigned long long *d = (unsigned long long *)c.dev + 2;
    TA_HIP(fill_u32_launch((uint32_t *)d, 0u, 4, st));
    StrView vn = sb_view(nd), vh = sb_view(hs);
    if (!need_n) vn.off = nullptr;
    if (!need_h) vh.off = nullptr;
    TA_HIP(search_batch_maxlen_launch(vn, vh, n, d, st));
    unsigned long long host[2] = {0, 0};
    TA_HIP(hipMemcpyAsync(host, d, 16, hipMemcpyDeviceToHost, st));
    TA_HIP(hipStreamSynchronize(st));
    if (need_n) *mn = host[0];
    if (need_h) *mh = host[1];
    return TA_OK;
}

// the pairs longest haystack first (util_kernels.hip: length_order_launch), so that a wavefront's lanes finish together.  The histogram
// scratch must be zero on entry and a complete pass leaves it zero: `clean` says this thread's last pass was complete.
static int sb_order(const ta_strings *hs, uint32_t n, uint64_t max_h, hipStream_t st, const uint32_t **order) {
    static thread_local bool clean = false;
    Scratch &ord = tls_scratch(SB_ORDER), &bins = tls_scratch(SB_BINS);
    constexpr size_t BINS_BYTES = 2 * 1024 * 32 * 4;
    const bool fresh = bins.cap < BINS_BYTES || !clean;
    int rc;
    if ((rc = ord.ensure((size_t)n * 4)) || (rc = bins.ensure(BINS_BYTES))) return rc;
    if (fresh) TA_HIP(fill_u32_launch((uint32_t *)bins.dev, 0u, (uint32_t)(BINS_BYTES / 8), st));
    clean = false;
    const StrView v = sb_view(hs);
    TA_HIP(length_order_launch(v, v, nullptr, n, 0u, max_h, false, (uint32_t *)bins.dev, (uint32_t *)ord.dev, st));
    clean = true;
    *order = (const uint32_t *)ord.dev;
    return TA_OK;
}

}  // namespace ta

using namespace ta;

extern "C" {

int ta_levenshtein_search_batch(const ta_strings *needles, const ta_strings *haystacks, size_t n,
                                uint32_t k, int search_type, const ta_edit_costs *costs, int anchored,
                                ta_match *matches_dev, uint32_t *counts_dev, size_t cap, void *stream) {
    if (!costs) { set_last_error_msg("null costs"); return TA_ERR_ARG; }
    {                                                                              // EditCosts::new, src/levenshtein.rs:44-52
        ta_edit_costs t;
        if (ta_edit_costs_new(costs->mismatch_cost, costs->gap_cost, costs->start_gap_cost, costs->has_transpose, costs->transpose_cost, &t) != TA_OK)
            return TA_ERR_BAD_COSTS;
    }
    if (ta_edit_costs_check_search(costs) != TA_OK) return TA_ERR_BAD_COSTS;      // :1965, for the whole batch
    if (!needles || !haystacks || (search_type != TA_SEARCH_ALL && search_type != TA_SEARCH_BEST) || n > 0xFFFFFFF0ull) {
        set_last_error_msg("bad search batch arguments");
        return TA_ERR_ARG;
    }
    if (n && (!needles->blob || !haystacks->blob || !counts_dev || (cap && !matches_dev))) { set_last_error_msg("null buffer"); return TA_ERR_ARG; }
    if (cap && n > SIZE_MAX / sizeof(ta_match) / cap) { set_last_error_msg("n * cap overflows"); return TA_ERR_ARG; }
    const bool shared = !needles->off && needles->stride == 0;
    if ((!needles->off || needles->max_len) && (needles->off ? needles->max_len : needles->len) > 0xFFFFu) {
        set_last_error_msg("needle longer than 65535 bytes");
        return TA_ERR_ARG;
    }
    if ((!haystacks->off || haystacks->max_len) && (haystacks->off ? haystacks->max_len : haystacks->len) >> 32) {
        set_last_error_msg("haystack of 2^32 bytes or more");
        return TA_ERR_UNSUPPORTED;
    }
    if (!device_ready()) return TA_ERR_HIP;
    if (n == 0) return TA_OK;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    uint64_t max_n = 0, max_h = 0;
    int rc = sb_max_lens(needles, haystacks, (uint32_t)n, st, &max_n, &max_h);
    if (rc) return rc;
    if (max_n > 0xFFFFu) { set_last_error_msg("needle longer than 65535 bytes"); return TA_ERR_ARG; }
    if (max_h >> 32) { set_last_error_msg("haystack of 2^32 bytes or more"); return TA_ERR_UNSUPPORTED; }

    SearchBatchParams P = {};
    P.nd = sb_view(needles); P.hs = sb_view(haystacks);
    P.matches = matches_dev; P.counts = counts_dev; P.cap = cap; P.n = (uint32_t)n;
    P.k = k; P.mc = costs->mismatch_cost; P.gc = costs->gap_cost; P.sg = costs->start_gap_cost;
    P.tc = costs->has_transpose ? costs->transpose_cost : 0;
    P.anchored = anchored ? 1u : 0u; P.best = search_type == TA_SEARCH_BEST ? 1u : 0u;
    P.max_needle = (uint32_t)max_n;
    const bool trans = costs->has_transpose != 0;
    const bool unit = P.mc == 1 && P.gc == 1 && P.sg == 0 && (!trans || P.tc == 1);
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
        Scratch &cs = tls_scratch(SB_COL);
        if ((rc = cs.ensure((size_t)(per_lane * lanes)))) return rc;
        P.col = (uint32_t *)cs.dev;
        mem_lanes = (uint32_t)lanes;
    }
    if (route_s) {
        Scratch &ctl = tls_scratch(SB_CTL), &ls = tls_scratch(SB_LIST), &sp = tls_scratch(SB_SPAN);
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
    if (haystacks->off && n >= 4096 && max_h >= 16) {
        const uint32_t *order = nullptr;
        if ((rc = sb_order(haystacks, (uint32_t)n, max_h, st, &order))) return rc;
        P.list = order;
    }
    TA_HIP(search_batch_exact_launch(P, trans, packed, mem_lanes, st));
    return TA_OK;
}

int ta_hamming_search_batch(const ta_strings *needles, const ta_strings *haystacks, size_t n,
                            uint32_t k, int search_type, ta_match *matches_dev, uint32_t *counts_dev, size_t cap, void *stream) {
    if (!needles || !haystacks || (search_type != TA_SEARCH_ALL && search_type != TA_SEARCH_BEST) || n > 0xFFFFFFF0ull) {
        set_last_error_msg("bad search batch arguments");
        return TA_ERR_ARG;
    }
    if (n && (!needles->blob || !haystacks->blob || !counts_dev || (cap && !matches_dev))) { set_last_error_msg("null buffer"); return TA_ERR_ARG; }
    if (cap && n > SIZE_MAX / sizeof(ta_match) / cap) { set_last_error_msg("n * cap overflows"); return TA_ERR_ARG; }
    if ((!needles->off || needles->max_len) && (needles->off ? needles->max_len : needles->len) > 0xFFFFu) {
        set_last_error_msg("needle longer than 65535 bytes");
        return TA_ERR_ARG;
    }
    if ((!haystacks->off || haystacks->max_len) && (haystacks->off ? haystacks->max_len : haystacks->len) >> 32) {
        set_last_error_msg("haystack of 2^32 bytes or more");
        return TA_ERR_UNSUPPORTED;
    }
    if (!device_ready()) return TA_ERR_HIP;
    if (n == 0) return TA_OK;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    uint64_t max_n = 0, max_h = 0;
    int rc = sb_max_lens(needles, haystacks, (uint32_t)n, st, &max_n, &max_h);
    if (rc) return rc;
    if (max_n > 0xFFFFu) { set_last_error_msg("needle longer than 65535 bytes"); return TA_ERR_ARG; }
    if (max_h >> 32) { set_last_error_msg("haystack of 2^32 bytes or more"); return TA_ERR_UNSUPPORTED; }

    HamBatchParams P = {};
    P.nd = sb_view(needles); P.hs = sb_view(haystacks);
    P.matches = matches_dev; P.counts = counts_dev; P.cap = cap; P.n = (uint32_t)n;
    P.k = k; P.best = search_type == TA_SEARCH_BEST ? 1u : 0u;
    P.max_needle = (uint32_t)max_n;
    // the bit-sliced form: one needle for every pair, 1..32 bytes, k at most a quarter of its length (so k <= 8: at most four counter
    // planes).  A window that passes the counters is recounted from memory, so the form is kept to thresholds where such windows are
    // rare whatever the alphabet; beyond, the general route counts every window exactly in registers
    const bool shared = !needles->off && needles->stride == 0;
    const bool bits = shared && max_n >= 1 && max_n <= 32 && 4ull * k <= max_n && !env_int("TA_HSEARCH_BATCH_GENERAL");
    if (haystacks->off && n >= 4096 && max_h >= 16) {
        const uint32_t *order = nullptr;
        if ((rc = sb_order(haystacks, (uint32_t)n, max_h, st, &order))) return rc;
        P.list = order;
    }
    TA_HIP(ham_search_batch_launch(P, bits, st));
    return TA_OK;
}

}  // extern "C"
