// emu_search_batch.cpp -- host emulation driver of the search batch body (lev_search_batch_body.h).  TESTS ONLY: one pair as one
// lane of the batch kernels runs it -- the scan with a host-built match table, the span, then the exact pass with the online fold.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "emu_wave.h"
#include "lev_search_batch_body.h"

using namespace ta;

template <int N, bool TRANS>
static void exact_regs(const uint8_t *hay, const uint8_t *needle, uint32_t n, const SearchCosts &C, bool packed, uint64_t cb, uint64_t eb,
                       uint64_t ce, SearchBatchSink &sink) {
    uint8_t nd[N];
    for (int j = 0; j < N; j++) nd[j] = (uint32_t)j < n ? needle[j] : 0;       // (the kernels hold the needle in registers)
    if (packed) lev_search_batch_exact<N, TRANS, true>(hay, nd, n, C, cb, eb, ce, sink);
    else lev_search_batch_exact<N, TRANS, false>(hay, nd, n, C, cb, eb, ce, sink);
}

template <bool TRANS>
static void exact_packed(const uint8_t *hay, const uint8_t *needle, uint32_t n, const SearchCosts &C, uint64_t cb, uint64_t eb, uint64_t ce,
                         SearchBatchSink &sink) {
    switch (n) {
#define TA_N(x) case x: exact_regs<x, TRANS>(hay, needle, n, C, true, cb, eb, ce, sink); return;
        TA_N(1) TA_N(2) TA_N(3) TA_N(4) TA_N(5) TA_N(6) TA_N(7) TA_N(8) TA_N(9) TA_N(10) TA_N(11) TA_N(12)
        TA_N(13) TA_N(14) TA_N(15) TA_N(16) TA_N(17) TA_N(18) TA_N(19) TA_N(20) TA_N(21) TA_N(22) TA_N(23) TA_N(24)
        TA_N(25) TA_N(26) TA_N(27) TA_N(28) TA_N(29) TA_N(30) TA_N(31) TA_N(32)
#undef TA_N
    }
}

// One pair.  route_s: scan (kf) + span + exact, as lev_search_batch_scan_kernel and the listed exact pass; else the whole haystack.
// form: 0 register (N = 32, row test), 1 packed (N = n), 2 memory-backed column.  Returns the result's length; out gets min(count, cap).
// *first / *last: the scanned span (route_s).
extern "C" uint32_t emu_search_batch_pair(const uint8_t *needle, uint32_t n, const uint8_t *hay, uint64_t h, uint32_t k, int best,
                                          uint32_t mc, uint32_t gc, uint32_t sg, int has_t, uint32_t tc, int anchored, int route_s, uint32_t kf,
                                          int form, ta_match *out, uint64_t cap, uint64_t *first, uint64_t *last) {
    const SearchCosts C{k, mc, gc, sg, has_t ? tc : 0u, anchored ? 1u : 0u};
    SearchBatchSink sink;
    sink.init(out, cap, best != 0, k);
    *first = *last = 0;
    if (!lev_search_batch_prologue(n, h, C, sink)) return sink.count;
    uint64_t cb = 0, eb = 0, ce = lev_search_batch_cols(n, h, C);
    if (route_s) {
        uint64_t f = 0, l = 0;
        if (n <= 32) {
            uint32_t peq[256];
            for (uint32_t c = 0; c < 256; c++) peq[c] = lev_filter_peq(needle, n, c);
            auto lk = [&](uint32_t c, int) { return peq[c]; };
            if (has_t) lev_search_batch_scan<1, true>(hay, h, lk, n, kf, f, l);
            else lev_search_batch_scan<1, false>(hay, h, lk, n, kf, f, l);
        } else {
            uint32_t peq[256][2];
            for (uint32_t c = 0; c < 256; c++)
                for (uint32_t w = 0; w < 2; w++) peq[c][w] = lev_filter_peq_word(needle, n, 2, c, w);
            auto lk = [&](uint32_t c, int w) { return peq[c][w]; };
            if (has_t) lev_search_batch_scan<2, true>(hay, h, lk, n, kf, f, l);
            else lev_search_batch_scan<2, false>(hay, h, lk, n, kf, f, l);
        }
        *first = f; *last = l;
        if (!f) return sink.count;                 // (the scan kernel finishes the pair: the end == 0 match or nothing)
        lev_search_batch_span_cols(f, l, n + kf + 2, cb, eb, ce);
    }
    if (form == 2 || n > 32) {
        std::vector<uint32_t> col(6 * ((size_t)n + 1));
        lev_search_tile_mem(hay, needle, n, C, has_t != 0, col.data(), 1, cb, eb, ce,
                            [&sink](uint64_t end, uint32_t len, uint32_t cost) { sink.put(end - len, end, cost); });
    } else if (form == 1) {
        if (has_t) exact_packed<true>(hay, needle, n, C, cb, eb, ce, sink);
        else exact_packed<false>(hay, needle, n, C, cb, eb, ce, sink);
    } else {
        if (has_t) exact_regs<32, true>(hay, needle, n, C, false, cb, eb, ce, sink);
        else exact_regs<32, false>(hay, needle, n, C, false, cb, eb, ce, sink);
    }
    return sink.count;
}

// the online fold alone over a given hit list (increasing end): what SearchBatchSink keeps
extern "C" uint32_t emu_search_batch_fold(const ta_match *hits, uint64_t n_hits, uint32_t k, int best, ta_match *out, uint64_t cap) {
    SearchBatchSink sink;
    sink.init(out, cap, best != 0, k);
    for (uint64_t i = 0; i < n_hits; i++) sink.put(hits[i].start, hits[i].end, hits[i].k);
    return sink.count;
}

// the scan's threshold under any EditCosts (lev_unit_filter_k)
extern "C" uint32_t emu_search_batch_filter_k(uint32_t k, uint32_t mc, uint32_t gc, uint32_t sg, int has_t, uint32_t tc) {
    return srch_filter_k(k, mc, gc, sg, has_t != 0, tc);
}
