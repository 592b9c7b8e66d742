// lev_search_cross_body.h -- levenshtein_search of EVERY needle of a panel in EVERY haystack of a batch (ta_levenshtein_search_cross,
// DESIGN.md 3.15): the lane mapping of the scan, the match table's columns, the per-needle rule, one pair's exact pass and the
// nearest / finish logic.
//
// The pair (needle p, haystack i) is answered exactly as ta_levenshtein_search_simd_with_opts(needle p, haystack i, k, Best, costs,
// anchored): the prologue, the recurrence and the online Best fold are lev_search_batch_body.h's, the scan step is
// lev_filter_body.h's.  What is new is the shape: the scan's LDS table peq[c * 64 + lane] holds 64 DIFFERENT needles' rows instead of
// 64 copies of one, so a wavefront scans one haystack (or 64 / G of them) against a whole group of needles at once.
// Plain per-lane code, no cross-lane traffic: tests run the same functions on the CPU.
#pragma once
#include <stdint.h>

#include "lev_search_batch_body.h"

namespace ta {

constexpr uint32_t SX_GROUP = 64;          // needles per group: the table's columns, the wavefront's lanes
constexpr uint32_t SX_WAVES = 8;           // wavefronts per scan workgroup (512 threads build one table)
constexpr uint32_t SX_MAX_NEEDLE = 32;     // the scan's word and the exact kernel's register form go no further
constexpr uint64_t SX_BUDGET = 256ull << 20;   // bytes of candidate records a sub-batch may need (SLOT_SB_COL's budget)

// One candidate of the scan, then (after the exact pass) its result, in place: a, b = the first and last candidate end (1-based), then
// R[0].start and R[0].end; k = TA_NONE until the exact pass finds a result, then R[0].k.
struct SxRec {
    uint32_t hay, needle, a, b, k;
};

// ---- the lane mapping.  A group of `size` needles (1..64) takes G = size rounded up to a power of two columns; lane l owns needle
// l mod G of the group and haystack slot l / G: 64 / G haystacks per wavefront.  A column without a needle (l mod G >= size) idles.
// group_size: the needles of a full group (SX_GROUP; the two-word routes' SX2_GROUP and HSX2_GROUP are 32: size 1..32, 64 / G >= 2).
TA_HD inline uint32_t sx_group_size(uint32_t nn, uint32_t group, uint32_t group_size = SX_GROUP) {
    const uint32_t left = nn - group * group_size;
    return left < group_size ? left : group_size;
}
TA_HD inline uint32_t sx_group_cols(uint32_t size) {
    uint32_t g = 1;
    while (g < size) g <<= 1;
    return g;
}
// the haystack (relative to the workgroup's first) of wavefront `wave`'s slot in iteration `it`: S = 64 / G slots per wavefront
TA_HD inline uint32_t sx_local_hay(uint32_t it, uint32_t wave, uint32_t S, uint32_t slot) { return (it * SX_WAVES + wave) * S + slot; }

// ---- the table.  Column l of row c = lev_filter_peq(needle of lane l, n, c): the wildcard rows below the needle in every row, the
// needle's own bits added row by row (sx_peq_bit into row needle[j]).  A needle the scan does not take, and a column without one: 0.
TA_HD inline uint32_t sx_peq_wild(uint32_t n) { return n < 32 ? ((1u << (32 - n)) - 1u) : 0u; }
TA_HD inline uint32_t sx_peq_bit(uint32_t n, uint32_t j) { return 1u << (32 - n + j); }

// ---- the per-needle rule.  The scan's threshold kf is a UNIT-cost one (k, or srch_filter_k under other costs).  With n == 0 or
// kf >= n every end passes it: the scan says nothing, the pair is a candidate over its whole haystack.  With kf < n a pair without a
// candidate end has NO result at all: the only match the scan cannot see is the end == 0 one (src/levenshtein.rs:1693-1706), which
// needs n gc + sg <= k -- an alignment of n gap characters, n unit edits, priced within k, so kf >= n (lev_unit_filter_k's argument).
TA_HD inline bool sx_scans(uint32_t n, uint32_t kf) { return n != 0 && kf < n; }

// One lane's scan of one haystack: the first and last end (1-based) whose unit-cost score is <= kf, first = 0 when there is none.
// peq(c) = the lane's column of row c.
template <bool TRANS, class Peq>
TA_HD inline void sx_scan_pair(const uint8_t *hay, uint64_t h, Peq peq, uint32_t n, uint32_t kf, uint32_t &first, uint32_t &last) {
    if (!sx_scans(n, kf)) { first = 1; last = (uint32_t)h; return; }
    first = 0; last = 0;
    FilterState s;
    lev_filter_reset(s, n);
    lev_search_batch_bytes(hay, h, [&](uint64_t i, uint32_t c) {
        if (lev_filter_step<TRANS>(s, peq(c)) <= kf) { if (!first) first = (uint32_t)i + 1; last = (uint32_t)i + 1; }
    });
}

// ---- the exact pass of one pair: R = the Best result, m = R[0], returns len(R) (0: no hit).  spans: over the scanned span [first, last]
// behind `halo` columns of context; else over the whole haystack or its anchored prefix.  The needle is held in N registers.
template <int N, bool TRANS, bool PACKED>
TA_HD inline uint32_t sx_exact_pair(const uint8_t *hay, uint64_t h, const uint8_t *np, uint32_t n, const SearchCosts &C, bool spans,
                                    uint32_t first, uint32_t last, uint32_t halo, ta_match &m) {
    SearchBatchSink sink;
    sink.init(&m, 1, true, C.k);
    if (lev_search_batch_prologue(n, h, C, sink)) {
        uint8_t needle[N];
#pragma unroll
        for (int j = 0; j < N; j++) needle[j] = (uint32_t)j < n ? np[j] : (uint8_t)0;
        uint64_t cb = 0, eb = 0, ce = lev_search_batch_cols(n, h, C);
        if (spans) lev_search_batch_span_cols(first, last, halo, cb, eb, ce);
        lev_search_batch_exact<N, TRANS, PACKED>(hay, needle, n, C, cb, eb, ce, sink);
    }
    return sink.count;
}

// ---- nearest and finish.  A haystack's nearest word is the smallest k << 32 | needle over its hits: the cheapest needle, the lowest
// index at equal cost.  A haystack meets every needle index once, so exactly one record carries the winning word: it writes best[i].
TA_HD inline uint64_t sx_word(uint32_t k, uint32_t needle) { return ((uint64_t)k << 32) | needle; }
TA_HD inline bool sx_wins(const SxRec &r, uint64_t nearest) { return r.k != TA_NONE && sx_word(r.k, r.needle) == nearest; }

// ---- the sub-batches.  The candidate list's worst case is nn records per haystack; the haystacks are taken `sub` at a time, in whole
// workgroups of `hpw` haystacks, so that the list stays within SX_BUDGET.  hpw: the table is built once per workgroup, so a workgroup
// takes as many haystacks as still leave about 2,048 workgroups (two per CU, four rounds); forced > 0: the sub-batch size of a test.
struct SxPlan {
    uint32_t groups, hpw, sub;
};
// group: the needles of one scan group (the two-word route's groups are 32 needles, lev_search_cross_w2_body.h).
inline SxPlan sx_plan(uint64_t nn, uint64_t nh, uint64_t forced, uint32_t group = SX_GROUP) {
    SxPlan p;
    p.groups = (uint32_t)((nn + group - 1) / group);
    uint64_t sub_max = SX_BUDGET / sizeof(SxRec) / (nn ? nn : 1);            // >= 204: nn <= 65,535
    if (forced && forced < sub_max) sub_max = forced;
    if (sub_max > nh) sub_max = nh;
    if (sub_max == 0) sub_max = 1;
    const uint64_t wgs = 2048 / (p.groups ? p.groups : 1) + 1;
    uint64_t hpw = (sub_max + wgs - 1) / wgs;
    if (hpw < SX_WAVES) hpw = SX_WAVES;
    if (hpw > sub_max) hpw = sub_max;
    p.hpw = (uint32_t)hpw;
    p.sub = (uint32_t)(sub_max >= nh ? nh : sub_max / hpw * hpw);              // (the last sub-batch alone may end in a partial workgroup)
    return p;
}

}  // namespace ta
