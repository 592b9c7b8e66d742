// lev_search_batch_body.h -- levenshtein_search over a BATCH of (needle, haystack) pairs, one lane per pair.
//
// Each pair's result is exactly ta_levenshtein_search_simd_with_opts(needle_i, haystack_i, ...): the end == 0 match
// (src/levenshtein.rs:1693-1706), the empty-needle answers (:1919-1963) and the Best fold (:1812-1835) happen here, per lane,
// with positions relative to the pair's haystack.  The recurrence itself is lev_search_body.h's tile functions run from a
// fresh column; the optional scan in front of it is lev_filter_body.h's unit-cost bit-parallel step.
// Plain per-lane code, no cross-lane traffic: tests run the same functions on the CPU.
#pragma once
#include <stdint.h>

#include "../../include/triple_accel_amd.h"
#include "lev_filter_body.h"
#include "lev_search_body.h"

namespace ta {

// One pair's result as the reference orders it (increasing end), written into its `cap` slots.  All mode keeps every hit.
// Best mode folds on the fly -- ta_search_fold_best with overlap_fold = 1 in one pass: a hit above the running threshold is
// dropped, a cheaper one restarts the list, an equally cheap one replaces the last kept match when it starts no later
// (:1812-1835), else it is appended.  count = the length of the whole result; only slots < cap are written.
struct SearchBatchSink {
    ta_match *out;
    uint64_t cap;
    uint32_t best, curr_k, count;
    uint64_t last_start;

    TA_HD void init(ta_match *o, uint64_t c, bool b, uint32_t k) {
        out = o; cap = c; best = b ? 1u : 0u; curr_k = k; count = 0; last_start = 0;
    }
    TA_HD void put(uint64_t start, uint64_t end, uint32_t cost) {
        uint32_t slot;
        if (best) {
            if (cost > curr_k) return;
            if (cost < curr_k) { curr_k = cost; count = 0; }
            if (count && start <= last_start) slot = count - 1;
            else slot = count++;
            last_start = start;
        } else {
            slot = count++;
        }
        if (slot < cap) out[slot] = ta_match{start, end, cost, 0u};
    }
};

// Everything of a pair that is not the recurrence: the empty needle (complete answer, returns false) or the end == 0 match
// (returns true: the caller runs the recurrence next).  n = needle length, h = haystack length.
TA_HD inline bool lev_search_batch_prologue(uint32_t n, uint64_t h, const SearchCosts &C, SearchBatchSink &sink) {
    if (n == 0) {                                                  // src/levenshtein.rs:1919-1963: no fold in either mode
        if (!C.anchored) return false;
        const uint32_t best = sink.best;
        sink.best = 0;
        sink.put(0, 0, 0);
        if (!best) {
            uint32_t cost = C.sg;
            for (uint64_t i = 0; i < h;) {
                i += 1;
                cost += C.gc;
                if (cost <= C.k) sink.put(0, i, cost); else break;
            }
        }
        sink.best = best;
        return false;
    }
    const uint32_t whole_gap = n * C.gc + C.sg;                    // :1693-1706 (u32 arithmetic, as the single-call form)
    if (whole_gap <= C.k) sink.put(0, 0, whole_gap);
    return true;
}

// Columns of the haystack a pair's search visits: an anchored search ends within needle_len + unit_k bytes (:1650-1658).
TA_HD inline uint64_t lev_search_batch_cols(uint32_t n, uint64_t h, const SearchCosts &C) {
    if (!C.anchored) return h;
    const uint32_t unit_k = (C.k > C.sg ? C.k - C.sg : 0u) / C.gc;
    const uint64_t lim = (uint64_t)n + unit_k;
    return lim < h ? lim : h;
}

// The exact recurrence over columns [col_begin, col_end), hits from column emit_begin on, into the sink.  `needle` is read
// with constant indices only (the caller keeps it in registers): rows past n are skipped by the register form's row test;
// the packed form needs N == n.
template <int N, bool TRANS, bool PACKED>
TA_HD inline void lev_search_batch_exact(const uint8_t *hay, const uint8_t *needle, uint32_t n, const SearchCosts &C,
                                         uint64_t col_begin, uint64_t emit_begin, uint64_t col_end, SearchBatchSink &sink) {
    auto emit = [&sink](uint64_t end, uint32_t len, uint32_t cost) { sink.put(end - len, end, cost); };
    if (PACKED) lev_search_tile_packed<N, TRANS>(hay, needle, n, C, col_begin, emit_begin, col_end, emit);
    else lev_search_tile<N, TRANS>(hay, needle, n, C, col_begin, emit_begin, col_end, emit);
}

// Every byte of hay[0..h) in order, f(i, byte): aligned dword loads inside the string, single bytes at its two ends -- nothing
// outside the string is read.
template <class F>
TA_HD inline void lev_search_batch_bytes(const uint8_t *hay, uint64_t h, F f) {
    uint64_t i = 0;
    const uint64_t head = (uint64_t)((4u - ((uintptr_t)hay & 3u)) & 3u);
    for (; i < h && i < head; i++) f(i, (uint32_t)hay[i]);
    for (; i + 4 <= h; i += 4) {
        const uint32_t w = *(const uint32_t *)(hay + i);
        f(i, w & 0xFFu); f(i + 1, (w >> 8) & 0xFFu); f(i + 2, (w >> 16) & 0xFFu); f(i + 3, w >> 24);
    }
    for (; i < h; i++) f(i, (uint32_t)hay[i]);
}

// The scan of Route S: the first and the last end (1-based, as Match.end) whose UNIT-cost semi-global score is <= kf -- a
// superset of the ends of every hit of cost <= k under the real costs when kf = srch_filter_k(...) (lev_search_body.h).
// first = 0 when there is none.  NWF = 1: needles of up to 32 bytes, peq(c) the match word of byte c;
// NWF = 2: up to 64 bytes, peq(c, w) word w.
template <int NWF, bool TRANS, class Peq>
TA_HD inline void lev_search_batch_scan(const uint8_t *hay, uint64_t h, Peq peq, uint32_t n, uint32_t kf, uint64_t &first, uint64_t &last) {
    first = 0; last = 0;
    if (NWF == 1) {
        FilterState s;
        lev_filter_reset(s, n);
        lev_search_batch_bytes(hay, h, [&](uint64_t i, uint32_t c) {
            if (lev_filter_step<TRANS>(s, peq(c, 0)) <= kf) { if (!first) first = i + 1; last = i + 1; }
        });
    } else {
        FilterStateN<2> s;
        lev_filter_reset_n<2>(s, n);
        lev_search_batch_bytes(hay, h, [&](uint64_t i, uint32_t c) {
            const uint32_t Eq[2] = {peq(c, 0), peq(c, 1)};
            if (lev_filter_step_n<2, TRANS>(s, Eq) <= kf) { if (!first) first = i + 1; last = i + 1; }
        });
    }
}

// The columns Route S's exact pass visits for a scanned span [first, last] of candidate ends: a fresh start `halo` =
// needle_len + kf + 2 columns before the first candidate makes every hit of cost <= k it reports exact (the tiled single
// search's argument, lev_search_body.h), and no hit ends outside the span.
TA_HD inline void lev_search_batch_span_cols(uint64_t first, uint64_t last, uint32_t halo, uint64_t &col_begin, uint64_t &emit_begin,
                                             uint64_t &col_end) {
    emit_begin = first - 1;
    col_begin = emit_begin > halo ? emit_begin - halo : 0;
    col_end = last;
}

}  // namespace ta
