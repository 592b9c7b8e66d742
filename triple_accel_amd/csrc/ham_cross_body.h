// ham_cross_body.h -- a chunk of queries against the 64 targets of a wavefront, Hamming distance: the inner steps of
// ta_hamming_cross, "every query against every target within k mismatches".
//
// Lane t owns one target and keeps it in NW dwords of registers (NW = 4, 8 or 16: strings of up to 16, 32 or 64 bytes, chosen from the
// longest query), every byte at or past its end zero; a target longer than 4 NW bytes can match no query and is not loaded at all.  The
// queries come a chunk at a time through the wavefront's own slice of LDS: lane L loads piece L % (NW / 4) of query L / (NW / 4) -- 16
// bytes -- zeroes the bytes past the query's end, XORs 0x0C into every byte and stores it; the piece-0 lanes also store the query's
// length.  Every lane then reads a query's dwords and its length at ONE address (a broadcast: no bank conflict) and a dword of the
// compare is v_xor, v_perm (wave.h ne12: 0x00 where target and query byte agree, 0xFF elsewhere) and v_bcnt with its accumulate operand,
// as in ham_swar_body.h.  The zero pads of both sides compare equal, so there is no tail mask in the loop; cnt = 8 x the mismatches.
//
// A pair is a hit with distance d exactly when both strings have the same length and hamming(query, target) = d <= k
// (src/hamming.rs:390; the reference panics on unequal lengths, ta_hamming_batch answers TA_NONE: here such a pair is never a hit).  A
// query whose length no live lane shares costs no compare.  Bytes are opaque: 0x00 and 0x0C are ordinary symbols -- a pad byte is only
// ever compared with a pad byte, because the lengths are equal.
#pragma once
#include <stdint.h>

#include "wave.h"

namespace ta {

template <class W, int NW>
struct HamCross {
    static_assert(NW == 4 || NW == 8 || NW == 16, "strings of up to 16, 32 or 64 bytes");
    static constexpr uint32_t MAX_LEN = 4u * NW;                 // bytes a lane holds of its target = the longest query
    static constexpr uint32_t PIECES = NW / 4u;                  // 16-byte pieces per string
    static constexpr uint32_t CHUNK = 64u / PIECES;              // queries staged at a time
    static constexpr uint32_t LEN_OFF = 1024u;                   // the chunk's lengths, one dword per query, behind its 1 KB of bytes
    static constexpr uint32_t LDS_BYTES = LEN_OFF + 4u * CHUNK;  // per wavefront
    using U32 = typename W::U32;
    using Bool = typename W::Bool;
    using Ptr = typename W::Ptr;
    using Q = typename W::Q;

    // the bytes of the dword at byte `base` of a string of `len` bytes that belong to the string, as a mask
    static TA_HD inline U32 keep_mask(U32 len, uint32_t base) {
        const U32 here = W::sel(len > base, len - base, W::splat(0));
        return W::sel(here >= 4u, W::splat(0xFFFFFFFFu), W::shlv(W::splat(1), (here & 3u) * 8u) - 1u);
    }

    // once per tile: the lane's target in registers.  usable = live and short enough to match a query; the others hold zeros and never hit
    static TA_HD inline Bool load_target(Ptr tp, U32 tl, Bool live, U32 (&t)[NW]) {
        const Bool usable = W::land(live, tl <= MAX_LEN);
#pragma unroll
        for (uint32_t p = 0; p < PIECES; p++) {
            // 16 bytes (up to 15 past the target's end: the blob's slack), none where the piece starts at or past the end
            const Q piece = W::gload16(W::ptr_add(tp, W::splat(16u * p)), W::land(usable, tl > 16u * p));
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) t[4 * p + j] = W::qword(piece, (int)j) & keep_mask(tl, 16u * p + 4u * j);
        }
        return usable;
    }

    // queries q0 .. q0 + n (n <= CHUNK) of `qs` into the wavefront's slice: bytes of query i at 4 NW i, its length at LEN_OFF + 4 i
    static TA_HD inline void stage(uint8_t *lds, const StrView &qs, uint32_t q0, uint32_t n) {
        const U32 lane = W::lane();
        const U32 qi = W::udiv(lane, PIECES), pc = lane - qi * PIECES;
        const Bool valid = qi < n;
        Ptr qp;
        U32 ql;
        W::load_str(qs, qi + q0, valid, qp, ql);
        const U32 start = pc * 16u;
        const Q piece = W::gload16(W::ptr_add(qp, start), W::land(valid, ql > start));
        const U32 rest = W::sel(ql > start, ql - start, W::splat(0));   // bytes of the query from this piece on
        W::lds_wave_sync();                                        // (the last chunk's reads lie before these writes)
#pragma unroll
        for (uint32_t j = 0; j < 4; j++)
            W::lds_write32p(lds, lane * 16u + 4u * j, (W::qword(piece, (int)j) & keep_mask(rest, 4u * j)) ^ 0x0C0C0C0Cu, valid);
        W::lds_write32p(lds, qi * 4u + LEN_OFF, ql, W::land(valid, pc == 0u));
        W::lds_wave_sync();
    }

    // Query i of the staged chunk against the 64 targets.  k8 = 8 min(k, 64) + 7.  hit / d: the lanes within k and their mismatch counts.
    // Returns false when no usable lane has the query's length: the query then cost one LDS read and no compare.
    static TA_HD inline bool compare(const uint8_t *lds, uint32_t i, const U32 (&t)[NW], U32 tl, Bool usable, uint32_t k8, Bool &hit, U32 &d) {
        const U32 m = W::lds_read32(lds, W::splat(LEN_OFF + 4u * i));
        const Bool same = W::land(usable, tl == m);
        hit = W::bfalse();
        d = W::splat(0);
        if (!W::any(same)) return false;
        U32 cnt = W::splat(0);
#pragma unroll
        for (uint32_t p = 0; p < PIECES; p++) {
            // (wave-uniform: past the end of every lane that can hit both sides hold pads only)
            if (p && !W::any(W::land(same, tl > 16u * p))) break;
#pragma unroll
            for (uint32_t j = 0; j < 4; j += 2) {
                U32 q0, q1;
                W::lds_read64(lds, W::splat(MAX_LEN * i + 16u * p + 4u * j), q0, q1);
                cnt = W::bcnt(W::ne12(t[4 * p + j] ^ q0), cnt);
                cnt = W::bcnt(W::ne12(t[4 * p + j + 1] ^ q1), cnt);
            }
        }
        hit = W::land(same, cnt <= k8);
        d = cnt >> 3;
        return true;
    }
};

}  // namespace ta
