// sym_compact_body.h -- per-pair symbol compaction of a batch of 32-bit token sequences (ta_tokens.hip).
//
// The edit-distance kernels only ever compare an item of `a` with an item of `b` (the transposition term too: a[i-1] == b[j],
// a[i] == b[j-1]).  Any per-pair code map with  a[i] == b[j]  <=>  ca[i] == cb[j]  therefore gives the same distance and the same
// edit script, edit for edit.  This body writes such a map as BYTES, one wavefront per pair, so the byte kernels run unchanged:
//
//   shorter side s of at most 255 items: code_s[i] = the first index i' with s[i'] == s[i]; an item x of the other side t gets the
//     first index i with s[i] == x, or 255.  Both sides' codes of a common item are its first index in s (<= 254); 255 only occurs on
//     t.  s is held in registers (up to four VGPRs per lane) and broadcast item by item (v_readlane).
//   shorter side of more than 255 items: an open-addressing hash table of s's distinct items (global scratch, one table per
//     wavefront), items of t found in it mark their slot; the marked slots are numbered 0.. in slot order.  Common items get that
//     number, items on one side only get 254 (a) or 255 (b).  More than 254 distinct common items: the pair goes on the overflow
//     list (its codes are not written; the caller answers it with 32-bit items).
//
// Orientation stays as given: only the side the coding refers to swaps (AGap / BGap depend on which side is `a`).
// Memory writes and atomics are vector (or LDS) operations only.  Written against the wave policy W (wave.h) plus the few operations
// of SymOps<W> below, so the host emulation (tests) runs the same body.
#pragma once
#include <stdint.h>

#include "wave.h"

namespace ta {

struct SymCompactParams {
    const uint32_t *a_data, *b_data;     // device; items of pair i: data[off[i] .. off[i+1]) or data[i * stride .. + len)
    const uint64_t *a_off, *b_off;       // CSR element offsets (n + 1) or nullptr
    uint64_t a_stride, a_len, b_stride, b_len;   // strided form
    uint8_t *ca, *cb;                    // codes: CSR at the caller's element offsets, strided with byte stride = len
    uint32_t n;
    uint64_t *table;                     // long pairs: per wavefront table_cap entries (0 = empty, else 1 << 32 | item)
    uint32_t *flags;                     //   and as many u32 (0: not common, else code + 1)
    uint32_t table_cap;                  // power of two >= 2 x the longest shorter side of a long pair (>= 64), 0: no long pairs
    uint32_t *ovf_list, *ovf_count;      // pairs with more than 254 distinct common items
};

constexpr uint32_t SYM_SHORT_MAX = 255;   // shorter sides up to this many items take the first-index coding

template <class W> struct SymOps;

#if defined(__HIPCC__)
template <> struct SymOps<DevWave> {
    using U32 = uint32_t;
    using Bool = bool;
    static __device__ __forceinline__ uint32_t readlane(U32 v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
    static __device__ __forceinline__ void store_u8(uint8_t *p, U32 idx, U32 v, Bool pred) { if (pred) p[idx] = (uint8_t)v; }
    static __device__ __forceinline__ void fence() { __threadfence(); }
    // slot h holds x after this (claimed now or before): 64-bit compare-and-swap on global memory
    static __device__ __forceinline__ Bool claim(uint64_t *tab, U32 h, U32 x, Bool pred) {
        if (!pred) return false;
        const unsigned long long key = (1ull << 32) | x;
        const unsigned long long old = atomicCAS((unsigned long long *)(tab + h), 0ull, key);
        return old == 0ull || old == key;
    }
    static __device__ __forceinline__ Bool holds(const uint64_t *tab, U32 h, U32 x, Bool pred, Bool &empty) {
        const uint64_t e = pred ? tab[h] : 0ull;
        empty = pred && e == 0ull;
        return pred && e == ((1ull << 32) | x);
    }
    static __device__ __forceinline__ void store_u64(uint64_t *p, U32 idx, uint64_t v, Bool pred) { if (pred) p[idx] = v; }
    static __device__ __forceinline__ uint64_t ballot(Bool c) { return __builtin_amdgcn_ballot_w64(c); }
    static __device__ __forceinline__ U32 bits_below(uint64_t m) {        // set bits of m in the lanes below this one
        return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    }
    static __device__ __forceinline__ void append(uint32_t *list, uint32_t *count, uint32_t v) {
        if (DevWave::lane() == 0) list[atomicAdd(count, 1u)] = v;
    }
};
#endif

template <class W> struct SymCompact {
    using U32 = typename W::U32;
    using Bool = typename W::Bool;
    using X = SymOps<W>;

    static TA_HD void side(const SymCompactParams &P, uint32_t i, bool is_a, const uint32_t *&p, uint32_t &len, uint8_t *&out) {
        const uint64_t *off = is_a ? P.a_off : P.b_off;
        const uint32_t *d = is_a ? P.a_data : P.b_data;
        uint8_t *c = is_a ? P.ca : P.cb;
        if (off) {
            const uint64_t o0 = off[i];
            p = d + o0; len = (uint32_t)(off[i + 1] - o0); out = c + o0;
        } else {
            const uint64_t st = is_a ? P.a_stride : P.b_stride, l = is_a ? P.a_len : P.b_len;
            p = d + (uint64_t)i * st; len = (uint32_t)l; out = c + (uint64_t)i * l;
        }
    }

    // codes of one side against s held in sreg (the first index of the item in s, or 255)
    static TA_HD void code_first(const U32 (&sreg)[4], uint32_t ls, const uint32_t *p, uint32_t len, uint8_t *out) {
        const U32 lane = W::lane();
        for (uint32_t base = 0; base < len; base += 64) {
            const U32 idx = lane + W::splat(base);
            const Bool valid = idx < W::splat(len);
            const U32 x = W::load_u32(p, idx, valid, 0u);
            U32 code = W::splat(255u);
#pragma unroll
            for (int r = 3; r >= 0; r--) {
                if ((uint32_t)r * 64u >= ls) continue;
                const uint32_t hi = ls - (uint32_t)r * 64u > 64u ? 63u : ls - (uint32_t)r * 64u - 1u;
                for (int l = (int)hi; l >= 0; l--) {                        // descending: the first index wins
                    const uint32_t sv = X::readlane(sreg[r], (uint32_t)l);
                    code = W::sel(x == W::splat(sv), W::splat((uint32_t)r * 64u + (uint32_t)l), code);
                }
            }
            X::store_u8(out, idx, code, valid);
        }
    }

    static TA_HD U32 hash(const U32 &x, uint32_t bits) { return (x * W::splat(2654435761u)) >> (int)(32u - bits); }

    // the slot of x (probing from its hash); found = false where the probe met an empty slot first
    static TA_HD U32 find(const uint64_t *tab, uint32_t mask, uint32_t bits, const U32 &x, const Bool &valid, Bool &found) {
        U32 h = hash(x, bits);
        Bool active = valid;
        found = W::bfalse();
        for (uint32_t probe = 0; probe <= mask && W::any(active); probe++) {
            Bool empty;
            const Bool hit = X::holds(tab, h, x, active, empty);
            found = found | hit;
            active = active & !(hit | empty);
            h = W::sel(active, (h + W::splat(1u)) & W::splat(mask), h);
        }
        return h;
    }

    static TA_HD void run(const SymCompactParams &P, uint32_t wave, uint32_t n_waves) {
        const U32 lane = W::lane();
        for (uint32_t i = wave; i < P.n; i += n_waves) {
            const uint32_t *ap, *bp;
            uint32_t la, lb;
            uint8_t *oa, *ob;
            side(P, i, true, ap, la, oa);
            side(P, i, false, bp, lb, ob);
            const bool s_is_a = la <= lb;
            const uint32_t *sp = s_is_a ? ap : bp, *tp = s_is_a ? bp : ap;
            const uint32_t ls = s_is_a ? la : lb, lt = s_is_a ? lb : la;
            uint8_t *os = s_is_a ? oa : ob, *ot = s_is_a ? ob : oa;
            if (ls <= SYM_SHORT_MAX) {
                U32 sreg[4];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const U32 idx = lane + W::splat((uint32_t)r * 64u);
                    sreg[r] = W::load_u32(sp, idx, idx < W::splat(ls), 0u);
                }
                code_first(sreg, ls, sp, ls, os);
                code_first(sreg, ls, tp, lt, ot);
                continue;
            }
            // long pair: hash table of s's distinct items
            uint32_t bits = 6;
            while ((1u << bits) < 2u * ls) bits++;
            const uint32_t T = 1u << bits, mask = T - 1u;
            uint64_t *tab = P.table + (uint64_t)wave * P.table_cap;
            uint32_t *fl = P.flags + (uint64_t)wave * P.table_cap;
            for (uint32_t base = 0; base < T; base += 64) {
                const U32 idx = lane + W::splat(base);
                X::store_u64(tab, idx, 0ull, idx == idx);
                W::store_u32(fl, idx, W::splat(0u), idx == idx);
            }
            X::fence();
            for (uint32_t base = 0; base < ls; base += 64) {             // insert s
                const U32 idx = lane + W::splat(base);
                const Bool valid = idx < W::splat(ls);
                const U32 x = W::load_u32(sp, idx, valid, 0u);
                U32 h = hash(x, bits);
                Bool active = valid;
                while (W::any(active)) {
                    const Bool done = X::claim(tab, h, x, active);
                    active = active & !done;
                    h = W::sel(active, (h + W::splat(1u)) & W::splat(mask), h);
                }
            }
            X::fence();
            for (uint32_t base = 0; base < lt; base += 64) {             // mark the items t shares
                const U32 idx = lane + W::splat(base);
                const Bool valid = idx < W::splat(lt);
                const U32 x = W::load_u32(tp, idx, valid, 0u);
                Bool found;
                const U32 h = find(tab, mask, bits, x, valid, found);
                W::store_u32(fl, h, W::splat(1u), found);
            }
            X::fence();
            uint32_t common = 0;                                          // number the marked slots in slot order
            for (uint32_t base = 0; base < T; base += 64) {
                const U32 idx = lane + W::splat(base);
                const Bool f = W::load_u32(fl, idx, idx == idx, 0u) != W::splat(0u);
                const uint64_t m = X::ballot(f);
                const U32 code = W::splat(common) + X::bits_below(m);
                W::store_u32(fl, idx, W::sel(f, code + W::splat(1u), W::splat(0u)), idx == idx);
                common += (uint32_t)__builtin_popcountll(m);
            }
            X::fence();
            if (common > 254u) {
                X::append(P.ovf_list, P.ovf_count, i);
                continue;
            }
            for (int sd = 0; sd < 2; sd++) {
                const uint32_t *p = sd ? tp : sp;
                const uint32_t len = sd ? lt : ls;
                uint8_t *o = sd ? ot : os;
                const bool is_a = (sd == 0) == s_is_a;
                for (uint32_t base = 0; base < len; base += 64) {
                    const U32 idx = lane + W::splat(base);
                    const Bool valid = idx < W::splat(len);
                    const U32 x = W::load_u32(p, idx, valid, 0u);
                    Bool found;
                    const U32 h = find(tab, mask, bits, x, valid, found);
                    const U32 c = W::load_u32(fl, h, found, 0u);
                    const U32 code = W::sel(c != W::splat(0u), c - W::splat(1u), W::splat(is_a ? 254u : 255u));
                    X::store_u8(o, idx, code, valid);
                }
            }
        }
    }
};

}  // namespace ta
