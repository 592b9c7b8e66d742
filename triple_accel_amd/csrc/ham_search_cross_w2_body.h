// ham_search_cross_w2_body.h -- the two-word route of ta_hamming_search_cross_with_opts: a panel whose longest needle is
// 33..64 bytes.  The plane count, the lane mapping, the mismatch table's columns and one pair's scan with the online Best fold.
//
// The shape is ham_search_cross_body.h's with every needle on TWO dwords (ham_bits2_body.h): the LDS table holds 32 columns of 2 words
// (64 KB, as the one-word table), a group is 32 needles, a wavefront scans 64 / G >= 2 haystacks per step.  The needle sits on the top
// n bits of the 64: a needle of 33 bytes has one position in the low word, a needle of up to 32 bytes lives wholly in the high word
// under an all-zero low word.  The per-pair rule (hsx_scans up to 64 bytes), the walk (hsx_words), the Best triple (HsxBest), the packed
// word, the stage and the finish are ham_search_cross_body.h's, unchanged.  The scan stays EXACT: no candidate list, no second pass.
// Plain per-lane code, no cross-lane traffic (the one wave-uniform test is handed in by the caller): tests run the same functions on
// the CPU.
#pragma once
#include <stdint.h>

#include "ham_bits2_body.h"
#include "ham_search_cross_body.h"

namespace ta {

constexpr uint32_t HSX2_GROUP = 32;        // needles per group: the table's columns, half a wavefront
constexpr uint32_t HSX2_MAX_NEEDLE = 64;   // two dwords of positions

// ---- the planes.  kc = min(k, longest needle) (hsx_threshold) now reaches 64: B = the smallest plane count with 2^B - 1 >= kc, 1..7.
TA_HD inline int hsx2_planes(uint32_t kc) { return kc <= HSX2_MAX_NEEDLE ? ham_bits2_planes(kc) : 0; }

// ---- the lane mapping.  A group of `size` needles (1..32: sx_group_size over HSX2_GROUP) takes G = size rounded up to a power of two
// columns (sx_group_cols); lane l owns needle l mod G of the group and haystack slot l / G: 64 / G >= 2 haystacks per wavefront
// (sx_local_hay with S = 64 / G).  The table has one column per lane of a 32-lane half: lane l reads column l mod 32, which holds
// needle (l mod 32) mod G = l mod G.  (hsx2_group_size: the rule under this route's name, as the host emulation spells it.)
TA_HD inline uint32_t hsx2_group_size(uint32_t nn, uint32_t group) { return sx_group_size(nn, group, HSX2_GROUP); }

// ---- the table.  Word w of column l of row c = word w of ham_bits2_mis(needle of column l, n, c), at dword hsx2_mis_at(c, l, w): the
// two words of a column lie side by side, so a lane takes both with one 8-byte read at byte c * 256 + l * 8.  Built as the one-word
// table, per dword of the pair: every row starts as "all n positions mismatch" (hsx2_mis_full), needle byte j then clears its bit in
// row needle[j].  A column without a needle, or with n = 0 or n > 64: 0, never read.
TA_HD inline bool hsx2_scans(uint32_t n) { return n >= 1u && n <= HSX2_MAX_NEEDLE; }
TA_HD inline uint32_t hsx2_mis_at(uint32_t c, uint32_t column, uint32_t w) { return (c * HSX2_GROUP + column) * 2u + w; }
TA_HD inline uint32_t hsx2_mis_full(uint32_t n, uint32_t w) {
    const HamBits2Word f = ham_bits2_split(ham_bits2_span(n));
    return w ? f.hi : f.lo;
}
TA_HD inline uint32_t hsx2_mis_bit(uint32_t n, uint32_t j, uint32_t &w) {   // needle byte j: bit 64 - n + j of the 64
    const uint32_t bit = 64u - n + j;
    w = bit >> 5;
    return 1u << (bit & 31u);
}

// the window that ends at byte `end` passed: its exact count is bit 63 of the planes minus the bias -- the high words alone
template <int B>
TA_HD inline void hsx2_fold(const uint32_t (&hi)[B], uint32_t base, uint32_t end, uint32_t n, HsxBest &r) {
    const uint32_t d = ham_bits2_count<B>(hi) - base;
    if (d < r.d) { r.d = d; r.start = end + 1u - n; r.count = 1u; }
    else if (d == r.d) r.count++;
}

// One lane's scan of one haystack; needs 1 <= n <= 64, n <= h, kc <= 2^B - 1.  mis(w, b) = the lane's two words of row (byte b of w);
// any(p): true when p holds on some lane of the wavefront (the host: p itself).  hsx_scan_pair's step on two words; of the four states
// of a dword only the high words -- what the fold reads -- stay in registers until the one test behind them.
template <int B, class Mis, class Any>
TA_HD inline void hsx2_scan_pair(const uint8_t *hay, uint32_t h, Mis mis, uint32_t n, uint32_t kc, Any any, HsxBest &r) {
    HamBits2State<B> st;
    ham_bits2_reset<B>(st, n);
    HamBits2Word bias[B];
    ham_bits2_bias<B>(kc, n, bias);
    const uint32_t base = ((1u << B) - 1u) - kc;
    uint32_t nul = 0;
    r.d = TA_NONE; r.start = 0; r.count = 0;
    hsx_words(hay, h, [&](uint32_t i, uint32_t w, uint32_t nb) {
        nul |= ham_zero_bytes(w, nb);
        if (nb == 4u) {
            const HamBits2Word m0 = mis(w, 0), m1 = mis(w, 1), m2 = mis(w, 2), m3 = mis(w, 3);
            uint32_t t0[B], t1[B], t2[B], t3[B];
            const uint32_t o0 = ham_bits2_step<B>(st, m0, bias);
            ham_bits2_top<B>(st, t0);
            const uint32_t o1 = ham_bits2_step<B>(st, m1, bias);
            ham_bits2_top<B>(st, t1);
            const uint32_t o2 = ham_bits2_step<B>(st, m2, bias);
            ham_bits2_top<B>(st, t2);
            const uint32_t o3 = ham_bits2_step<B>(st, m3, bias);
            if (any(((o0 & o1 & o2 & o3) >> 31) == 0u)) {
                ham_bits2_top<B>(st, t3);
                if (!(o0 >> 31)) hsx2_fold<B>(t0, base, i, n, r);
                if (!(o1 >> 31)) hsx2_fold<B>(t1, base, i + 1u, n, r);
                if (!(o2 >> 31)) hsx2_fold<B>(t2, base, i + 2u, n, r);
                if (!(o3 >> 31)) hsx2_fold<B>(t3, base, i + 3u, n, r);
            }
        } else {
            const bool pass = (ham_bits2_step<B>(st, mis(w, 0), bias) >> 31) == 0u;
            if (any(pass)) {
                uint32_t t[B];
                ham_bits2_top<B>(st, t);
                if (pass) hsx2_fold<B>(t, base, i, n, r);
            }
        }
    });
    r.nul = nul != 0u;
}

// ---- haystacks per workgroup: hsx_hpw over groups of HSX2_GROUP needles, at least HSX2_MIN_HPW -- one full step of the eight
// wavefronts, two haystacks each.
constexpr uint32_t HSX2_MIN_HPW = 2u * SX_WAVES;
inline uint32_t hsx2_hpw(uint64_t nn, uint64_t nh, uint64_t forced) { return hsx_hpw(nn, nh, forced, HSX2_GROUP, HSX2_MIN_HPW); }

}  // namespace ta
