// ham_search_cross_body.h -- hamming_search of EVERY needle of a panel in EVERY haystack of a batch (ta_hamming_search_cross,
// DESIGN.md 3.16): the plane count, the mismatch table's columns, the byte walk with its fused NUL scan, one pair's scan with the online
// Best fold, the packed nearest word and the finish.
//
// The pair (needle p, haystack i) is answered exactly as ta_hamming_search_simd_with_opts(needle p, haystack i, k, Best)
// (src/hamming.rs:454-475, scalar text :96-146): needle_len > haystack_len and the empty needle give no hit, only then a 0x00 byte in the
// haystack is the NUL verdict; else the windows at the smallest mismatch count <= k, in increasing start, no overlap fold.  The lane
// mapping is lev_search_cross_body.h's (G columns per group, 64 / G haystack slots per wavefront), the counters are ham_bits_body.h's
// with per-lane bias words -- the lanes' needle lengths differ.  The scan is EXACT: the planes hold the mismatch count of the window that
// just completed, so there is no candidate list and no second pass.  Plain per-lane code, no cross-lane traffic (the one wave-uniform
// test is handed in by the caller): tests run the same functions on the CPU.
#pragma once
#include <stdint.h>

#include "ham_search_batch_body.h"
#include "lev_search_cross_body.h"

namespace ta {

// ---- the planes.  One threshold kc = min(k, longest needle) serves every lane: a window of a needle of n bytes has at most n
// mismatches, so k above the longest needle changes nothing, and a lane with n <= kc simply never overflows (every window is a
// candidate, the fold keeps the minimum).  B = the smallest plane count with 2^B - 1 >= kc: 1..6 for needles of up to 32 bytes
// (ham_bits_planes stops at 5: its callers keep k < n <= 32 and, on the batch route, 4 k <= n).
TA_HD inline uint32_t hsx_threshold(uint32_t k, uint32_t max_needle) { return k < max_needle ? k : max_needle; }
TA_HD inline int hsx_planes(uint32_t kc) {
    for (int B = 1; B <= 6; B++) if (((1u << B) - 1u) >= kc) return B;
    return 0;
}

// ---- the table.  Column l of row c = ham_bits_mis(needle of lane l, n, c): every row starts as "all n positions mismatch"
// (hsx_mis_full), needle byte j then clears its bit in row needle[j].  A column without a needle, or with n = 0 or n > 32: 0, never read.
TA_HD inline bool hsx_scans(uint32_t n) { return n >= 1u && n <= SX_MAX_NEEDLE; }
TA_HD inline uint32_t hsx_mis_full(uint32_t n) { return n >= 32u ? 0xFFFFFFFFu : ~((1u << (32u - n)) - 1u); }
TA_HD inline uint32_t hsx_mis_bit(uint32_t n, uint32_t j) { return 1u << (32u - n + j); }

// ---- the walk: lev_search_batch_bytes' loads (aligned dwords inside the string, single bytes at its two ends, nothing outside the
// string), but a load is handed over whole: word(i, w, nb) -- w holds the nb = 1 or 4 bytes i .. i + nb - 1 of the haystack -- so that the
// NUL scan runs per load, a dword's four table lookups are issued together and the rare path is tested once per load.  The next dword is
// loaded before the current one is worked on.
template <class FW>
TA_HD inline void hsx_words(const uint8_t *hay, uint32_t h, FW word) {
    uint32_t i = 0;
    const uint32_t head = (4u - (uint32_t)((uintptr_t)hay & 3u)) & 3u;
    for (; i < h && i < head; i++) word(i, (uint32_t)hay[i], 1u);
    uint32_t cur = h - i >= 4u ? *(const uint32_t *)(hay + i) : 0u;
    for (; h - i >= 4u; i += 4u) {
        const uint32_t nxt = *(const uint32_t *)(hay + (h - i >= 8u ? i + 4u : i));    // (unconditional: the last one loads its own dword again)
        word(i, cur, 4u);
        cur = nxt;
    }
    for (; i < h; i++) word(i, (uint32_t)hay[i], 1u);
}

// One pair's result: the smallest mismatch count d <= k (TA_NONE: no window), the first start at d, the number of windows at d, and
// whether the haystack holds a 0x00 byte.
struct HsxBest {
    uint32_t d, start, count;
    bool nul;
};

// the window that ends at byte `end` passed: its exact count is the planes' bit 31 minus the bias; the scalar routine's Best rule
// (src/hamming.rs:105-142) in one pass -- a cheaper window restarts the list, an equal one is counted
template <int B>
TA_HD inline void hsx_fold(const HamBitsState<B> &s, uint32_t base, uint32_t end, uint32_t n, HsxBest &r) {
    uint32_t v = 0;
#pragma unroll
    for (int p = 0; p < B; p++) v |= (s.P[p] >> 31) << p;
    const uint32_t d = v - base;
    if (d < r.d) { r.d = d; r.start = end + 1u - n; r.count = 1u; }
    else if (d == r.d) r.count++;
}

// One lane's scan of one haystack; needs 1 <= n <= 32, n <= h, kc <= 2^B - 1.  mis(w, b) = the lane's column of row (byte b of w);
// any(p): true when p holds on some lane of the wavefront (the host: p itself) -- the common step is the counter update alone.
// Bit 31 of OV clear: the window that ends at this byte has at most kc mismatches (and n bytes have been consumed: ham_bits_reset).  The
// four states of a dword stay in registers until the one test behind them.
template <int B, class Mis, class Any>
TA_HD inline void hsx_scan_pair(const uint8_t *hay, uint32_t h, Mis mis, uint32_t n, uint32_t kc, Any any, HsxBest &r) {
    HamBitsState<B> st;
    ham_bits_reset<B>(st, n);
    uint32_t bias[B];
    ham_bits_bias<B>(kc, n, bias);
    const uint32_t base = ((1u << B) - 1u) - kc;
    uint32_t nul = 0;
    r.d = TA_NONE; r.start = 0; r.count = 0;
    hsx_words(hay, h, [&](uint32_t i, uint32_t w, uint32_t nb) {
        nul |= ham_zero_bytes(w, nb);
        if (nb == 4u) {
            const uint32_t m0 = mis(w, 0), m1 = mis(w, 1), m2 = mis(w, 2), m3 = mis(w, 3);
            HamBitsState<B> s0 = st;
            const uint32_t o0 = ham_bits_step<B>(s0, m0, bias);
            HamBitsState<B> s1 = s0;
            const uint32_t o1 = ham_bits_step<B>(s1, m1, bias);
            HamBitsState<B> s2 = s1;
            const uint32_t o2 = ham_bits_step<B>(s2, m2, bias);
            st = s2;
            const uint32_t o3 = ham_bits_step<B>(st, m3, bias);
            if (any(((o0 & o1 & o2 & o3) >> 31) == 0u)) {
                if (!(o0 >> 31)) hsx_fold<B>(s0, base, i, n, r);
                if (!(o1 >> 31)) hsx_fold<B>(s1, base, i + 1u, n, r);
                if (!(o2 >> 31)) hsx_fold<B>(s2, base, i + 2u, n, r);
                if (!(o3 >> 31)) hsx_fold<B>(st, base, i + 3u, n, r);
            }
        } else {
            const bool pass = (ham_bits_step<B>(st, mis(w, 0), bias) >> 31) == 0u;
            if (any(pass)) {
                if (pass) hsx_fold<B>(st, base, i, n, r);
            }
        }
    });
    r.nul = nul != 0u;
}

// ---- nearest and finish.  A haystack's packed word is the smallest d << 48 | needle << 32 | start over its hits (d needs 6 bits, the
// needle index 16, the start 32): ordered by (d, needle) -- a haystack meets every needle index once -- and carrying the winner's start.
TA_HD inline uint64_t hsx_word(uint32_t d, uint32_t needle, uint32_t start) { return ((uint64_t)d << 48) | ((uint64_t)needle << 32) | start; }
TA_HD inline uint32_t hsx_word_needle(uint64_t w) { return (uint32_t)(w >> 32) & 0xFFFFu; }
TA_HD inline uint64_t hsx_nearest(uint64_t w) { return w == ~0ull ? ~0ull : ((w >> 48) << 32) | hsx_word_needle(w); }
TA_HD inline ta_match hsx_best(uint64_t w, uint32_t needle_len) {
    if (w == ~0ull) return ta_match{0, 0, TA_NONE, 0u};
    const uint64_t start = w & 0xFFFFFFFFull;
    return ta_match{start, start + needle_len, (uint32_t)(w >> 48), 0u};
}

// ---- the append.  A wavefront stages its records in LDS, a step's hits in ballot order behind those of the steps before, and flushes the
// stage -- one add to the counter, the records behind it -- when the next step's hits would not fit, and at its end.
constexpr uint32_t HSX_STAGE = 64;

// ---- haystacks per workgroup.  The table is built once per workgroup, so a workgroup takes as many haystacks as still leave about 2,048
// workgroups (lev_search_cross_body.h: sx_plan), and at least min_hpw: one full step of its eight wavefronts -- SX_WAVES over groups of
// SX_GROUP needles, 2 SX_WAVES over the two-word route's groups of HSX2_GROUP (two haystacks per wavefront); forced > 0: a test's value.
inline uint32_t hsx_hpw(uint64_t nn, uint64_t nh, uint64_t forced, uint32_t group_size = SX_GROUP, uint32_t min_hpw = SX_WAVES) {
    const uint64_t groups = (nn + group_size - 1) / group_size;
    const uint64_t wgs = 2048 / (groups ? groups : 1) + 1;
    uint64_t hpw = forced ? forced : (nh + wgs - 1) / wgs;
    if (!forced && hpw < min_hpw) hpw = min_hpw;
    if (hpw > nh) hpw = nh;
    return (uint32_t)(hpw ? hpw : 1);
}

}  // namespace ta
