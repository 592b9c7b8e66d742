// ham_long_body.h -- the mismatch count of one SLICE of a long pair, one wavefront: the inner steps of ham_long_kernel,
// "hamming of long strings, every pair sliced across the chip".
//
// A pair is cut into slices of S bytes (S a multiple of 1,024); a wavefront is handed the n <= S bytes of one slice of a and of b -- at
// ANY and different byte alignments -- and returns the number of positions where they differ.  A trip is TRIP = 4 KiB of each string:
// lane L loads the 16 bytes at 16 L of each of the trip's four 1 KiB quarters, of a and of b -- eight unconditional, unaligned 16-byte
// loads in straight-line code, all issued before the first one is consumed (a wavefront keeps 8 KiB in flight).  A dword of the compare
// is v_xor (with 0x0C folded in), v_perm (wave.h ne12: 0x00 where the bytes agree, 0xFF elsewhere) and v_bcnt with its accumulate
// operand, as in ham_cross_body.h: cnt = 8 x the mismatches.
//
// Nothing outside [0, n) is ever read, so nothing outside it can reach the count: the whole trips lie inside the slice, the last
// n % 4,096 bytes go through four PREDICATED 16-byte loads (a piece is loaded only where all 16 bytes belong to the slice; the lanes
// without one hold zeros on both sides, which compare equal), and the last n % 16 bytes are loaded one byte per lane.  The entry
// therefore needs no read slack behind the strings (ta_hamming_dev takes bare device pointers).
#pragma once
#include <stdint.h>

#include "wave.h"

namespace ta {

template <class W>
struct HamLong {
    static constexpr uint32_t QUARTER = 1024u;                   // bytes a wavefront's 64 lanes cover with one 16-byte load each
    static constexpr uint32_t LOADS = 4u;                        // 16-byte loads of each string a lane has in flight
    static constexpr uint32_t TRIP = LOADS * QUARTER;
    using U32 = typename W::U32;
    using Bool = typename W::Bool;
    using Ptr = typename W::Ptr;
    using Q = typename W::Q;

    // cnt + 8 x the differing bytes of two 16-byte pieces
    static TA_HD inline U32 piece(const Q &x, const Q &y, U32 cnt) {
#pragma unroll
        for (int j = 0; j < 4; j++) cnt = W::bcnt(W::ne12(W::qword(x, j) ^ W::qword(y, j) ^ 0x0C0C0C0Cu), cnt);
        return cnt;
    }

    // the number of i < n with a[i] != b[i]; a, b and n are wave-uniform, n <= 2^28
    static TA_HD inline uint32_t slice(const uint8_t *a, const uint8_t *b, uint32_t n) {
        const U32 lane16 = W::lane() * 16u;
        U32 cnt = W::splat(0);
        uint32_t off = 0;
        for (; n - off >= TRIP; off += TRIP) {
            const Ptr pa = W::ptr_add(W::ptr_splat(a + off), lane16), pb = W::ptr_add(W::ptr_splat(b + off), lane16);
            const Q x0 = W::gload16_all(pa), x1 = W::gload16_all(W::ptr_add(pa, W::splat(QUARTER))),
                    x2 = W::gload16_all(W::ptr_add(pa, W::splat(2u * QUARTER))), x3 = W::gload16_all(W::ptr_add(pa, W::splat(3u * QUARTER)));
            const Q y0 = W::gload16_all(pb), y1 = W::gload16_all(W::ptr_add(pb, W::splat(QUARTER))),
                    y2 = W::gload16_all(W::ptr_add(pb, W::splat(2u * QUARTER))), y3 = W::gload16_all(W::ptr_add(pb, W::splat(3u * QUARTER)));
            cnt = piece(x0, y0, cnt);
            cnt = piece(x1, y1, cnt);
            cnt = piece(x2, y2, cnt);
            cnt = piece(x3, y3, cnt);
        }
        if (off < n) {
            // the last n - off < TRIP bytes: the 16-byte pieces that lie inside the slice ...
            const uint32_t rest = n - off;
            const Ptr pa = W::ptr_add(W::ptr_splat(a + off), lane16), pb = W::ptr_add(W::ptr_splat(b + off), lane16);
            Q x[LOADS], y[LOADS];
#pragma unroll
            for (uint32_t u = 0; u < LOADS; u++) {
                const Bool whole = lane16 + (u * QUARTER + 16u) <= rest;
                x[u] = W::gload16(W::ptr_add(pa, W::splat(u * QUARTER)), whole);
                y[u] = W::gload16(W::ptr_add(pb, W::splat(u * QUARTER)), whole);
            }
#pragma unroll
            for (uint32_t u = 0; u < LOADS; u++) cnt = piece(x[u], y[u], cnt);
            // ... and the n % 16 bytes behind them, one per lane
            const uint32_t odd = n & 15u;
            if (odd) {
                const U32 lane = W::lane();
                const Bool in = lane < odd;
                const uint32_t at = n - odd;
                const U32 xb = W::gload_u8(W::ptr_add(W::ptr_splat(a + at), lane), in), yb = W::gload_u8(W::ptr_add(W::ptr_splat(b + at), lane), in);
                cnt = cnt + W::sel(xb != yb, W::splat(8), W::splat(0));
            }
        }
        return W::wave_sum(cnt >> 3);
    }
};

}  // namespace ta
