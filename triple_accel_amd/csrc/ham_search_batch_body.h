// ham_search_batch_body.h -- hamming_search over a BATCH of (needle, haystack) pairs, one lane per pair.
//
// Each pair's result is exactly ta_hamming_search_simd_with_opts(needle_i, haystack_i, k, search_type) (src/hamming.rs:454-475, scalar
// text :96-146): needle_len > haystack_len and the empty needle give an empty result, only then a NUL byte anywhere in the haystack is the
// NUL verdict (TA_NONE in the pair's count); else every offset p in [0, h - n] with at most k mismatches, in increasing p, Best keeping the
// windows at the smallest count.  Three forms of the scan, each a function that returns the pair's count word:
//   ham_batch_pair_regs<NW>  any needle of up to 4 NW bytes: the needle in NW dwords, a sliding window of NW + 1 haystack dwords, four
//                            offsets per loaded dword, xor + v_perm + v_bcnt per needle dword (ham_swar_body.h's compare)
//   ham_batch_pair_mem       any needle: both sides read from memory, a window abandoned above the running threshold
//   ham_batch_pair_bits<B>   a needle of up to 32 bytes with k < n: ham_bits_body.h's bit-sliced counters, one table lookup and 3 B + 2
//                            instructions per haystack byte; a window that passes is recounted a dword at a time.  The host takes this
//                            form only where such windows are rare (4 k <= n): the recount's loads follow the previous hit's store
// The NUL scan rides on the haystack words each form loads anyway.  Plain per-lane code, no cross-lane traffic: the tests run the same
// functions on the CPU.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/triple_accel_amd.h"
#include "ham_bits_body.h"
#include "ham_swar_body.h"
#include "wave.h"

namespace ta {

// One pair's result in the reference's order (increasing start), written into its `cap` slots.  All mode keeps every window of at most k
// mismatches.  Best mode is the scalar routine's rule (src/hamming.rs:105-142) in one pass: the threshold starts at k, a window above it
// is dropped, a cheaper one lowers it and restarts the list, an equal one is appended -- ta_search_fold_best with overlap_fold = 0.
// count = the length of the whole result; only slots < cap are written.
struct HamBatchSink {
    ta_match *out;
    uint64_t cap;
    uint32_t best, curr_k, count, n;

    TA_HD void init(ta_match *o, uint64_t c, bool b, uint32_t k, uint32_t needle_len) {
        out = o; cap = c; best = b ? 1u : 0u; curr_k = k; count = 0; n = needle_len;
    }
    TA_HD void put(uint32_t start, uint32_t cnt) {
        if (cnt > curr_k) return;
        if (best && cnt < curr_k) { curr_k = cnt; count = 0; }
        const uint32_t slot = count++;
        if (slot < cap) out[slot] = ta_match{(uint64_t)start, (uint64_t)start + n, cnt, 0u};
    }
};

// a dword / four dwords at any byte address
TA_HD inline uint32_t ham_ld32(const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t __attribute__((aligned(1))) u32u;
    return *(const u32u *)p;
#else
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}
struct HamQ { uint32_t w[4]; };
TA_HD inline HamQ ham_ld128(const uint8_t *p) {
    HamQ q;
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));
    const u32x4u v = *(const u32x4u *)p;
    q.w[0] = v.x; q.w[1] = v.y; q.w[2] = v.z; q.w[3] = v.w;
#else
    memcpy(q.w, p, 16);
#endif
    return q;
}
// non-zero exactly when one of the dword's low `valid` bytes (1..4, or more: all four) is 0x00
TA_HD inline uint32_t ham_zero_bytes(uint32_t w, uint32_t valid) {
    if (valid < 4u) w |= 0xFFFFFFFFu << (8u * valid);
    return (w - 0x01010101u) & ~w & 0x80808080u;
}
// the pairs the reference answers before it looks at a byte (src/hamming.rs:455-461)
TA_HD inline bool ham_batch_trivial(uint64_t n, uint64_t h) { return n > h || n == 0; }

// ---- register form -----------------------------------------------------------------------------------------------------------
// the needle as the window compare wants it: msk[j] covers the needle's bytes of dword j, nd12[j] = those bytes ^ 0x0C (ham_ne12: a byte
// of (window & msk) ^ nd12 is 12 exactly where window and needle agree, and in every byte past the needle's end)
template <int NW>
TA_HD inline void ham_batch_needle(const uint8_t *np, uint32_t n, uint32_t (&nd12)[NW], uint32_t (&msk)[NW]) {
#pragma unroll
    for (int j = 0; j < NW; j++) {
        const uint32_t lo = 4u * (uint32_t)j;
        const uint32_t valid = n > lo ? (n - lo < 4u ? n - lo : 4u) : 0u;
        const uint32_t m = valid >= 4u ? 0xFFFFFFFFu : ((1u << (8u * valid)) - 1u);
        const uint32_t v = valid ? ham_ld32(np + lo) : 0u;         // (up to 3 bytes past the needle: the blob's slack)
        msk[j] = m;
        nd12[j] = (v & m) ^ 0x0C0C0C0Cu;
    }
}
// EIGHT TIMES the mismatches of the window that starts R bytes into w[0]
template <int NW, int R>
TA_HD inline uint32_t ham_batch_count8(const uint32_t (&w)[NW + 1], const uint32_t (&nd12)[NW], const uint32_t (&msk)[NW]) {
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < NW; j++) c += ham_popc(ham_ne12((ham_window<R>(w[j + 1], w[j]) & msk[j]) ^ nd12[j]));
    return c;
}

template <int NW>
TA_HD inline uint32_t ham_batch_pair_regs(const uint8_t *np, uint64_t nl, const uint8_t *hay, uint64_t hl, uint32_t k, bool best,
                                          ta_match *out, uint64_t cap) {
    if (ham_batch_trivial(nl, hl)) return 0u;
    const uint32_t n = nl < 4u * (uint32_t)NW ? (uint32_t)nl : 4u * (uint32_t)NW, h = (uint32_t)hl;   // (the caller's bound: no clamp in a valid call)
    HamBatchSink sink;
    sink.init(out, cap, best, k, n);
    uint32_t nd12[NW], msk[NW];
    ham_batch_needle<NW>(np, n, nd12, msk);
    uint32_t nul = 0;
    // dword d of the haystack (up to 3 bytes past its end: slack; nothing further), its own bytes checked for NUL.  Every byte of the
    // haystack is in some window, so every dword below h is loaded once.
    auto load = [&](uint32_t d) -> uint32_t {
        const uint32_t b = 4u * d;
        if (b >= h) return 0u;
        const uint32_t v = ham_ld32(hay + b);
        nul |= ham_zero_bytes(v, h - b);
        return v;
    };
    uint32_t w[NW + 1];
#pragma unroll
    for (int i = 0; i < NW; i++) w[i] = load((uint32_t)i);
    const uint32_t last = h - n;
    uint32_t nxt = load((uint32_t)NW);
    for (uint32_t g = 0; 4u * g <= last; g++) {                    // offsets 4 g .. 4 g + 3
        w[NW] = nxt;
        nxt = load(g + (uint32_t)NW + 1u);                         // one dword ahead of its use
        const uint32_t p = 4u * g;
        const uint32_t c0 = ham_batch_count8<NW, 0>(w, nd12, msk), c1 = ham_batch_count8<NW, 1>(w, nd12, msk),
                       c2 = ham_batch_count8<NW, 2>(w, nd12, msk), c3 = ham_batch_count8<NW, 3>(w, nd12, msk);
        sink.put(p, c0 >> 3);
        if (p + 1u <= last) sink.put(p + 1u, c1 >> 3);
        if (p + 2u <= last) sink.put(p + 2u, c2 >> 3);
        if (p + 3u <= last) sink.put(p + 3u, c3 >> 3);
#pragma unroll
        for (int i = 0; i < NW; i++) w[i] = w[i + 1];
    }
    return nul ? TA_NONE : sink.count;
}

// ---- memory form ---------------------------------------------------------------------------------------------------------------
// EIGHT TIMES the mismatches of the n-byte window `win` against the needle, both read a dword at a time (up to 3 bytes past each: slack);
// gives up -- any value above 8 limit + 7 -- once the count passes `limit`
TA_HD inline uint32_t ham_batch_count8_mem(const uint8_t *win, const uint8_t *np, uint32_t n, uint32_t limit) {
    const uint32_t full = n >> 2, tail = n & 3u;
    uint32_t c8 = 0;
    for (uint32_t j = 0; j < full; j++) {
        c8 += ham_popc(ham_ne12(ham_ld32(win + 4u * j) ^ ham_ld32(np + 4u * j) ^ 0x0C0C0C0Cu));
        if ((c8 >> 3) > limit) return c8;
    }
    if (tail) {
        const uint32_t m = (1u << (8u * tail)) - 1u;
        c8 += ham_popc(ham_ne12(((ham_ld32(win + 4u * full) ^ ham_ld32(np + 4u * full)) & m) ^ 0x0C0C0C0Cu));
    }
    return c8;
}

TA_HD inline uint32_t ham_batch_pair_mem(const uint8_t *np, uint64_t nl, const uint8_t *hay, uint64_t hl, uint32_t k, bool best,
                                         ta_match *out, uint64_t cap) {
    if (ham_batch_trivial(nl, hl)) return 0u;
    const uint32_t n = (uint32_t)nl, h = (uint32_t)hl;
    HamBatchSink sink;
    sink.init(out, cap, best, k, n);
    uint32_t nul = 0;
    for (uint32_t b = 0; b < h; b += 4u) nul |= ham_zero_bytes(ham_ld32(hay + b), h - b);
    if (nul) return TA_NONE;
    const uint32_t last = h - n;
    for (uint32_t p = 0; p <= last; p++) sink.put(p, ham_batch_count8_mem(hay + p, np, n, sink.curr_k) >> 3);
    return sink.count;
}

// ---- bit-sliced form -----------------------------------------------------------------------------------------------------------
// mis(word, b) = Mis[byte b of word] (ham_bits_mis of the needle).  Needs 1 <= n <= 32, k < n, B = ham_bits_planes(k).
template <int B, class Mis>
TA_HD inline uint32_t ham_batch_pair_bits(const uint8_t *np, uint32_t n, const uint8_t *hay, uint64_t hl, uint32_t k, bool best, Mis mis,
                                          ta_match *out, uint64_t cap) {
    if (ham_batch_trivial(n, hl)) return 0u;
    const uint32_t h = (uint32_t)hl;
    HamBatchSink sink;
    sink.init(out, cap, best, k, n);
    HamBitsState<B> st;
    ham_bits_reset<B>(st, n);
    uint32_t bias[B];
    ham_bits_bias<B>(k, n, bias);
    uint32_t nul = 0;
    HamQ cur = ham_ld128(hay), nxt = cur;                          // 16 bytes per load (the last one up to 15 bytes into the slack)
    for (uint32_t i = 0; i < h; i += 16u) {
        if (i + 16u < h) nxt = ham_ld128(hay + i + 16u);           // one block ahead, issued before this block's match stores
        const uint32_t valid = h - i < 16u ? h - i : 16u;
        uint32_t acc = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (4u * (uint32_t)q < valid) nul |= ham_zero_bytes(cur.w[q], valid - 4u * (uint32_t)q);
#pragma unroll
            for (int b = 0; b < 4; b++) acc = (acc << 1) | (ham_bits_step<B>(st, mis(cur.w[q], b), bias) >> 31);
        }
        // bit 15 - t: the window that ENDS at byte i + t has more than k mismatches
        uint32_t hits = ~acc & 0xFFFFu & ~((1u << (16u - valid)) - 1u);
        while (hits) {                                             // rare; increasing t
            const uint32_t t = 15u - (31u - (uint32_t)__builtin_clz(hits));
            hits &= ~(1u << (15u - t));
            const uint32_t x = i + t;
            if (x < n - 1u) continue;                              // (no window ends there)
            const uint32_t pos = x - (n - 1u);
            sink.put(pos, ham_batch_count8_mem(hay + pos, np, n, 0xFFFFFFFFu) >> 3);
        }
        cur = nxt;
    }
    return nul ? TA_NONE : sink.count;
}

}  // namespace ta
