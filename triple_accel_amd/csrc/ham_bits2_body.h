// ham_bits2_body.h -- the bit-sliced mismatch counters of ham_bits_body.h on 64 positions: needles of up to 64 bytes.
//
// Contract as ham_bits_body.h (src/hamming.rs:454-554): mismatches(p) <= k for every offset p in [0, h - n].
//
// A plane is 64 positions wide, held as two dwords {lo, hi}.  Needle position j sits on bit 64 - n + j of the 64, so a needle of
// n <= 32 bytes lives wholly in `hi` -- its `lo` words (table, bias, planes) stay zero and its answers are ham_bits_body.h's bit for
// bit.  A haystack byte c costs, per plane b,
//     s_b = (P_b << 1) | bias_b      the shift by one crosses the word boundary: hi = hi << 1 | lo >> 31 (one v_alignbit_b32)
//     P_b = s_b ^ carry_b,  carry_{b+1} = s_b & carry_b,  carry_0 = Mis[c]     the ripple add runs over the PLANES, position by position:
//                                    it never crosses the word boundary
//     OV = (OV << 1) | carry_B
// and bit 63 of OV (bit 31 of OV.hi) is the verdict of the alignment that just completed; bit 63 of the planes is its counter
// (ham_bits2_count).  7 B + 4 instructions + the lookup per byte against the one-word form's 3 B + 2.  Plain per-lane code, nothing of
// any one caller in it: the tests run the same functions on the CPU.
#pragma once
#include <stdint.h>

#include "wave.h"

namespace ta {

struct HamBits2Word { uint32_t lo, hi; };

TA_HD inline HamBits2Word ham_bits2_split(uint64_t v) { return HamBits2Word{(uint32_t)v, (uint32_t)(v >> 32)}; }
// the needle's positions: bits 64 - n .. 63 (n = 0: none)
TA_HD inline uint64_t ham_bits2_span(uint32_t n) { return n >= 64u ? ~0ull : n == 0u ? 0ull : ~((1ull << (64u - n)) - 1ull); }

// planes needed for threshold k (2^B - 1 >= k, k <= 64): 1..7; 0: k too large
TA_HD inline int ham_bits2_planes(uint32_t k) {
    for (int B = 1; B <= 7; B++) if (((1u << B) - 1u) >= k) return B;
    return 0;
}
// Mis[c]: bit 64 - n + j = needle[j] != c
TA_HD inline HamBits2Word ham_bits2_mis(const uint8_t *needle, uint32_t n, uint32_t c) {
    uint64_t m = 0;
    for (uint32_t j = 0; j < n; j++)
        if ((uint32_t)needle[j] != c) m |= 1ull << (64u - n + j);
    return ham_bits2_split(m);
}
template <int B> struct HamBits2State { HamBits2Word P[B], OV; };
template <int B> TA_HD inline void ham_bits2_reset(HamBits2State<B> &s, uint32_t n) {
#pragma unroll
    for (int b = 0; b < B; b++) s.P[b] = HamBits2Word{0u, 0u};
    // the alignments "in flight" at a scan's start are nobody's: overflowed (the bits below the needle's stay zero -- a new alignment's
    // overflow bit is shifted in from there)
    s.OV = ham_bits2_split(ham_bits2_span(n));
}
// bias_b: bit b of 2^B - 1 - k on the entry position, bit 64 - n
template <int B> TA_HD inline void ham_bits2_bias(uint32_t k, uint32_t n, HamBits2Word (&bias)[B]) {
    const uint32_t v = ((1u << B) - 1u) - k;
#pragma unroll
    for (int b = 0; b < B; b++) bias[b] = ham_bits2_split((uint64_t)((v >> b) & 1u) << (64u - n));
}
// one haystack byte; returns OV.hi (bit 31: the alignment that ends at this byte has MORE than k mismatches)
template <int B>
TA_HD inline __attribute__((always_inline)) uint32_t ham_bits2_step(HamBits2State<B> &s, HamBits2Word mis, const HamBits2Word (&bias)[B]) {
    HamBits2Word carry = mis;
#pragma unroll
    for (int b = 0; b < B; b++) {
        const uint32_t thi = ((s.P[b].hi << 1) | (s.P[b].lo >> 31)) | bias[b].hi;
        const uint32_t tlo = (s.P[b].lo << 1) | bias[b].lo;
        s.P[b].hi = thi ^ carry.hi; s.P[b].lo = tlo ^ carry.lo;
        carry.hi = thi & carry.hi; carry.lo = tlo & carry.lo;
    }
    s.OV.hi = ((s.OV.hi << 1) | (s.OV.lo >> 31)) | carry.hi;
    s.OV.lo = (s.OV.lo << 1) | carry.lo;
    return s.OV.hi;
}
// the counter of the alignment that just completed (bit 63 of every plane), bias included: mismatches + 2^B - 1 - k.  Only the `hi`
// words are read: a caller that keeps a state for later keeps those alone.
template <int B> TA_HD inline uint32_t ham_bits2_count(const uint32_t (&hi)[B]) {
    uint32_t v = 0;
#pragma unroll
    for (int p = 0; p < B; p++) v |= (hi[p] >> 31) << p;
    return v;
}
template <int B> TA_HD inline void ham_bits2_top(const HamBits2State<B> &s, uint32_t (&hi)[B]) {
#pragma unroll
    for (int p = 0; p < B; p++) hi[p] = s.P[p].hi;
}

}  // namespace ta
