// lev_cross_win_body.h -- ONE query of up to 256 bytes against the 64 targets of a wavefront, unit-cost Levenshtein / restricted Damerau
// under a threshold k: the inner step of ta_levenshtein_cross_with_opts for queries of 65 .. 256 bytes.
//
// The frame is lev_cross_body.h's: lane t owns one target, the query lies along the rows, its match vectors are a table in the
// wavefront's slice of LDS (256 rows of NB = 8 dwords at a stride of 9, row c = the rows of the query that hold byte c), a column costs each lane one
// lookup with its own target byte, the score is followed down the column's last row, and the length prefilter answers the pairs whose
// lengths are more than k apart.  What is new is that a lane holds only a WINDOW of the column: under a threshold k only the rows within
// k of the diagonal can lie on a path of cost <= k, and all 64 lanes stand at the same column, so the 32-row blocks that hold those rows
// are the same for every lane.  The window is the WW blocks [lo, lo + WW) with lo wave-uniform; every register index is a constant.
//
//   nb = ceil(m / 32) blocks.  Before the piece of 16 columns that starts at 0-based column j0:
//       lo = min(nb - 1, NB - WW, max(0, j0 - k) / 32)
//   and while the held lo is smaller the window SLIDES: every array moves down one register, the top register starts as a block does
//   at column 0 (Pv = ~0, Mv = 0, D0p = ~0, Eqp = 0), and when block lo + WW - 1 exists the score moves down to its last row
//   (+ 32, or + m - 32 (nb - 1) for the query's last block).  WW >= (2 k + 15) / 32 + 2 makes the window hold rows
//   j0 + 1 - k .. j0 + 16 + k; when that reaches NB the window is the whole column and never moves (win_ww).
//   The bound NB - WW keeps every table read inside the row: a window that would hang over the table's end stays where it is, which
//   only holds MORE rows below.  Blocks at and above nb read zeros and compute rows that nothing reads (carries only travel upwards).
//
//   A column is lev_cross_body.h's over the WW words; at the window's first word the addc chain starts with carry 0, Phs takes in-bit 1,
//   Mhs and the transposition shift take in-bit 0 -- row 0's rules, applied at the window's top.  The score takes the Ph / Mh bit of the
//   last live block's bottom row: bit 31, or bit (m - 1) & 31 once that block is the query's last.
//
// Exact: the row above the window is taken as +1 per column and an entering block as score + 1, + 2, ... down its rows; both are costs
// of real edit paths, so every computed cell is an upper bound of the true one, and a cell of value <= k has an optimal path inside
// the band, which the window holds: it is exact.  By the prefilter |m - len(t)| <= k, so at a lane's last column row m is inside the
// window and the query's last block is the window's last live one.
//
// The table is all zero between queries: a query clears exactly the slots it set, so the table is zeroed once per wavefront.
#pragma once
#include <stdint.h>

#include "wave.h"

namespace ta {

constexpr uint32_t WIN_NB = 8;                                   // blocks of 32 rows: queries of up to 256 bytes
constexpr uint32_t WIN_MAX_QUERY = 32u * WIN_NB;
// dwords from one table row to the next: 9.  Packed rows (8) put bytes that agree modulo 4 on the same banks -- C and G for one; the odd
// stride spreads them.  It costs 9 KB of LDS per wavefront instead of 8 (four wavefronts per SIMD instead of five) and measured 3.5 - 4 %
// faster on ACGT reads all the same (-DTA_WIN_ROW_DWORDS=8 builds the packed table).
#ifndef TA_WIN_ROW_DWORDS
#define TA_WIN_ROW_DWORDS 9
#endif
constexpr uint32_t WIN_ROW_DWORDS = TA_WIN_ROW_DWORDS;
static_assert(WIN_ROW_DWORDS == WIN_NB || WIN_ROW_DWORDS == WIN_NB + 1, "row stride");

// the smallest instantiated window for unit threshold k: 2 for k <= 8, 3 for k <= 24, 4 for k <= 40, else the whole column
static inline TA_HD int win_ww(uint32_t k) {
    const uint64_t need = (2ull * k + 15u) / 32u + 2u;
    return need <= 2 ? 2 : need <= 3 ? 3 : need <= 4 ? 4 : (int)WIN_NB;
}

template <class W, int WW, bool TRANS>
struct LevCrossWin {
    static_assert(WW == 2 || WW == 3 || WW == 4 || WW == (int)WIN_NB, "window widths");
    static constexpr uint32_t NB = WIN_NB;
    static constexpr uint32_t MAX_QUERY = WIN_MAX_QUERY;
    static constexpr uint32_t ROW = 4u * WIN_ROW_DWORDS;         // bytes from a table row to the next
    static constexpr uint32_t LDS_BYTES = 256u * ROW;            // per wavefront
    static constexpr uint32_t MAX_LO = NB - (uint32_t)WW;
    using U32 = typename W::U32;
    using Bool = typename W::Bool;
    using Ptr = typename W::Ptr;
    using Q = typename W::Q;

    // once per wavefront, before its first query
    static TA_HD inline void clear(uint8_t *lds) {
        const U32 lane_off = W::lane() * 4u;
#pragma unroll
        for (uint32_t e = 0; e < LDS_BYTES; e += 256u) W::lds_write32(lds, lane_off + e, W::splat(0));
        W::lds_wave_sync();
    }

    static TA_HD inline Q first_piece(Ptr tp, U32 tl, Bool live) { return W::gload16(tp, W::land(live, tl > 0u)); }

    // rows of block b of a query of m bytes in nb blocks
    static TA_HD inline uint32_t block_rows(uint32_t b, uint32_t nb, uint32_t m) { return b + 1u == nb ? m - 32u * (nb - 1u) : 32u; }

    // The 64 answers of query qp[0 .. m) (m <= MAX_QUERY), unit threshold k with win_ww(k) <= WW: LevCross::query's contract.
    static TA_HD inline bool query(uint8_t *lds, const uint8_t *qp, uint32_t m, Ptr tp, U32 tl, Bool live, const Q &first, uint32_t k,
                                   U32 &res, Bool &skip) {
        const U32 lane = W::lane();
        const U32 none = W::splat(0xFFFFFFFFu);
        const U32 diff = W::sel(tl > m, tl - m, W::splat(m) - tl);
        skip = W::land(live, diff > k);                           // src/levenshtein.rs:426-428
        const Bool work = W::land(live, !(diff > k));
        res = none;
        if (!W::any(work)) return false;
        if (m == 0) {                                            // one gap run: len(t), within k by the prefilter
            res = W::sel(work, tl, none);
            return true;
        }
        // ---- the query's table: in round r lane i sets bit (64 r + i) & 31 of dword (64 r + i) >> 5 of row q[64 r + i]
        U32 slot[4];
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            if (64u * r >= m) break;
            const U32 i = lane + 64u * r;
            const Bool mine = i < m;
            const U32 qb = W::gload_u8(W::ptr_add(W::ptr_splat(qp), i), mine);
            slot[r] = qb * ROW + (i >> 5) * 4u;
            W::lds_or32(lds, slot[r], W::shlv(W::splat(1), lane & 31u), mine);
        }
        W::lds_wave_sync();

        const U32 tle = W::sel(work, tl, W::splat(0));            // columns whose score counts
        const uint32_t cols = W::wave_max(tle);
        const uint32_t nb = (m + 31u) >> 5;
        U32 Pv[WW], Mv[WW], D0p[WW], Eqp[WW];
#pragma unroll
        for (int w = 0; w < WW; w++) {
            Pv[w] = W::splat(0xFFFFFFFFu); Mv[w] = W::splat(0);  // column 0: D grows by 1 per row
            D0p[w] = W::splat(0xFFFFFFFFu); Eqp[w] = W::splat(0);
        }
        uint32_t lo = 0;
        U32 score = W::splat(m < 32u * (uint32_t)WW ? m : 32u * (uint32_t)WW);   // the initial window's last row
        for (uint32_t j0 = 0; j0 < cols; j0 += 16u) {
            uint32_t want = j0 > k ? (j0 - k) >> 5 : 0u;
            if (want > nb - 1u) want = nb - 1u;
            if (want > MAX_LO) want = MAX_LO;
            if (lo < want) {                                      // (a piece is 16 columns: want grows by at most one block)
                lo++;
#pragma unroll
                for (int w = 0; w + 1 < WW; w++) { Pv[w] = Pv[w + 1]; Mv[w] = Mv[w + 1]; D0p[w] = D0p[w + 1]; Eqp[w] = Eqp[w + 1]; }
                Pv[WW - 1] = W::splat(0xFFFFFFFFu); Mv[WW - 1] = W::splat(0);
                D0p[WW - 1] = W::splat(0xFFFFFFFFu); Eqp[WW - 1] = W::splat(0);
                const uint32_t in_block = lo + (uint32_t)WW - 1u;
                if (in_block < nb) score = score + W::splat(block_rows(in_block, nb, m));
            }
            const uint32_t live_w = nb - lo < (uint32_t)WW ? nb - lo : (uint32_t)WW;   // the window's live words: 1 .. WW
            const uint32_t sb = lo + live_w == nb ? (m - 1u) & 31u : 31u;             // the score's row in the last of them
            const uint32_t row_off = 4u * lo;
            // 16 target bytes (up to 15 past the target's end: the blob's slack); a lane past its end reads nothing and looks up row 0
            const Q piece = j0 ? W::gload16(W::ptr_add(tp, W::splat(j0)), W::splat(j0) < tle) : first;
            const U32 w4[4] = {W::qword(piece, 0), W::qword(piece, 1), W::qword(piece, 2), W::qword(piece, 3)};
#pragma unroll
            for (int r = 0; r < 16; r++) {
                if (r == 8 && j0 + 8u >= cols) break;             // (wave-uniform: the second half of the piece holds no live column)
                const U32 c = W::byte_of(w4[r >> 2], r & 3);
                const U32 at = c * ROW + row_off;
                U32 Eq[WW], D0[WW], Ph[WW], Mh[WW];
#pragma unroll
                for (int w = 0; w + 1 < WW; w += 2) W::lds_read64(lds, at + 4u * (uint32_t)w, Eq[w], Eq[w + 1]);
                if (WW & 1) Eq[WW - 1] = W::lds_read32(lds, at + 4u * (uint32_t)(WW - 1));
                Bool carry = W::bfalse();
#pragma unroll
                for (int w = 0; w < WW; w++) {
                    U32 s;
                    W::addc(Eq[w] & Pv[w], Pv[w], carry, s, carry);
                    D0[w] = ((s ^ Pv[w]) | Eq[w]) | Mv[w];
                }
                if (TRANS) {                                      // D0 |= ((~D0_prev & Eq) << 1) & Eq_prev  (src/levenshtein.rs:517-525)
                    U32 X[WW];
#pragma unroll
                    for (int w = 0; w < WW; w++) X[w] = ~D0p[w] & Eq[w];
#pragma unroll
                    for (int w = 0; w < WW; w++) D0[w] = D0[w] | (W::template alignbit<31>(X[w], w ? X[w - 1] : W::splat(0)) & Eqp[w]);
                }
#pragma unroll
                for (int w = 0; w < WW; w++) {
                    Ph[w] = Mv[w] | ~(D0[w] | Pv[w]);
                    Mh[w] = D0[w] & Pv[w];
                }
                U32 ph = Ph[0], mh = Mh[0];                       // of the last live word (live_w is wave-uniform)
#pragma unroll
                for (int w = 1; w < WW; w++)
                    if ((uint32_t)w < live_w) { ph = Ph[w]; mh = Mh[w]; }
                const Bool in = W::splat(j0 + (uint32_t)r) < tle;
                const U32 up = W::shr_u(ph, sb) & 1u, down = W::shr_u(mh, sb) & 1u;
                score = score + W::sel(in, up, W::splat(0)) - W::sel(in, down, W::splat(0));
#pragma unroll
                for (int w = 0; w < WW; w++) {
                    const U32 Phs = W::template alignbit<31>(Ph[w], w ? Ph[w - 1] : W::splat(0x80000000u));   // the row above the window: +1 per column
                    const U32 Mhs = W::template alignbit<31>(Mh[w], w ? Mh[w - 1] : W::splat(0));
                    Pv[w] = Mhs | ~(D0[w] | Phs);
                    Mv[w] = Phs & D0[w];
                    if (TRANS) { D0p[w] = D0[w]; Eqp[w] = Eq[w]; }
                }
            }
        }
        // the slots this query set, back to zero
        W::lds_wave_sync();
#pragma unroll
        for (uint32_t r = 0; r < 4; r++) {
            if (64u * r >= m) break;
            W::lds_write32p(lds, slot[r], W::splat(0), (lane + 64u * r) < m);
        }
        W::lds_wave_sync();
        res = W::sel(W::land(work, score <= k), score, none);    // src/levenshtein.rs:539-541
        return true;
    }
};

}  // namespace ta
