// lev_search_cross_w2_body.h -- the two-word route of ta_levenshtein_search_cross_with_opts: a panel whose longest
// needle is 33..64 bytes.  The lane mapping of the scan, the match table's columns, one pair's scan and one pair's exact pass.
//
// The shape is lev_search_cross_body.h's with every needle on TWO dwords: the scan's LDS table holds 32 columns of 2 words (64 KB, as
// the one-word table), a group is 32 needles, a wavefront scans 64 / G >= 2 haystacks per step.  The needle sits on the top n bits of
// the 64 (lev_filter_peq_word, nwf = 2): a needle of 33 bytes has one row in word 0, a needle of up to 32 bytes lives wholly in word 1
// under an all-wildcard word 0.  The scan step is lev_filter_step_n<2, TRANS>; the exact pass keeps the DP column in memory
// (lev_search_tile_mem, as lev_search_batch_mem_kernel).  The per-needle rule (sx_scans), the records (SxRec), the nearest word and the
// finish logic are lev_search_cross_body.h's, unchanged.
// Plain per-lane code, no cross-lane traffic: tests run the same functions on the CPU.
#pragma once
#include <stdint.h>

#include "lev_search_cross_body.h"

namespace ta {

constexpr uint32_t SX2_GROUP = 32;         // needles per group: the table's columns, half a wavefront
constexpr uint32_t SX2_MAX_NEEDLE = 64;    // two dwords of rows
constexpr uint32_t SX2_COL_WORDS = 6u * (SX2_MAX_NEEDLE + 1u);   // one lane's memory-backed column: 6 arrays of up to 65 elements
// the exact pass's resident lanes: their columns stay within SX_BUDGET (172,032 lanes of 1,560 bytes)
constexpr uint64_t SX2_MAX_LANES = SX_BUDGET / (SX2_COL_WORDS * 4u) / 256u * 256u;

// ---- the lane mapping.  A group of `size` needles (1..32: sx_group_size over SX2_GROUP) takes G = size rounded up to a power of two
// columns (sx_group_cols); lane l owns needle l mod G of the group and haystack slot l / G: 64 / G >= 2 haystacks per wavefront
// (sx_local_hay with S = 64 / G).  The table has one column per lane of a 32-lane half: lane l reads column l mod 32, which holds
// needle (l mod 32) mod G = l mod G.  (sx2_group_size: the rule under this route's name, as the host emulation spells it.)
TA_HD inline uint32_t sx2_group_size(uint32_t nn, uint32_t group) { return sx_group_size(nn, group, SX2_GROUP); }

// ---- the table.  Word w of column l of row c = lev_filter_peq_word(needle of column l, n, 2, c, w), at dword sx2_peq_at(c, l, w): the
// two words of a column lie side by side, so a lane takes both with one 8-byte read.  Built as the one-word table: the wildcard words in
// every row, then the needle's own bits row by row.  A needle the scan does not take, and a column without one: 0.
TA_HD inline uint32_t sx2_peq_at(uint32_t c, uint32_t column, uint32_t w) { return (c * SX2_GROUP + column) * 2u + w; }
TA_HD inline uint32_t sx2_peq_wild(uint32_t n, uint32_t w) {
    const uint32_t pad = 64u - n, lo = 32u * w;                     // wildcard rows: bits [0, pad) of the 64
    return pad >= lo + 32u ? 0xFFFFFFFFu : pad <= lo ? 0u : (1u << (pad - lo)) - 1u;
}
TA_HD inline uint32_t sx2_peq_bit(uint32_t n, uint32_t j, uint32_t &w) {   // needle byte j: bit 64 - n + j of the 64
    const uint32_t bit = 64u - n + j;
    w = bit >> 5;
    return 1u << (bit & 31u);
}

// One lane's scan of one haystack: the first and last end (1-based) whose unit-cost score is <= kf, first = 0 when there is none.
// peq(c, Eq) = the two words of the lane's column of row c.  A needle the scan does not take: a candidate over its whole haystack.
template <bool TRANS, class Peq>
TA_HD inline void sx2_scan_pair(const uint8_t *hay, uint64_t h, Peq peq, uint32_t n, uint32_t kf, uint32_t &first, uint32_t &last) {
    if (!sx_scans(n, kf)) { first = 1; last = (uint32_t)h; return; }
    first = 0; last = 0;
    FilterStateN<2> s;
    lev_filter_reset_n<2>(s, n);
    lev_search_batch_bytes(hay, h, [&](uint64_t i, uint32_t c) {
        uint32_t Eq[2];
        peq(c, Eq);
        if (lev_filter_step_n<2, TRANS>(s, Eq) <= kf) { if (!first) first = (uint32_t)i + 1; last = (uint32_t)i + 1; }
    });
}

// ---- the exact pass of one pair, as sx_exact_pair with the DP column in memory: element j of array a of this lane at
// col[(a * (n + 1) + j) * stride] (lev_search_tile_mem) -- `stride` = the resident lanes, so a wavefront's accesses coalesce.
template <bool TRANS>
TA_HD inline uint32_t sx2_exact_pair(const uint8_t *hay, uint64_t h, const uint8_t *np, uint32_t n, const SearchCosts &C, bool spans,
                                     uint32_t first, uint32_t last, uint32_t halo, uint32_t *col, uint64_t stride, ta_match &m) {
    SearchBatchSink sink;
    sink.init(&m, 1, true, C.k);
    if (lev_search_batch_prologue(n, h, C, sink)) {
        uint64_t cb = 0, eb = 0, ce = lev_search_batch_cols(n, h, C);
        if (spans) lev_search_batch_span_cols(first, last, halo, cb, eb, ce);
        lev_search_tile_mem(hay, np, n, C, TRANS, col, stride, cb, eb, ce,
                            [&sink](uint64_t end, uint32_t len, uint32_t cost) { sink.put(end - len, end, cost); });
    }
    return sink.count;
}

// the exact pass's resident lanes for up to `work` records: whole workgroups of 256, at most SX2_MAX_LANES
inline uint32_t sx2_exact_lanes(uint64_t work) {
    uint64_t lanes = (work + 255u) / 256u * 256u;
    if (lanes < 256u) lanes = 256u;
    return (uint32_t)(lanes < SX2_MAX_LANES ? lanes : SX2_MAX_LANES);
}

}  // namespace ta
