// lev_cross_body.h -- ONE query against the 64 targets of a wavefront, unit-cost Levenshtein / restricted Damerau:
// the inner step of ta_levenshtein_cross, "every query against every target within k".
//
// Lane t owns one target.  The query (m <= 32 NW bytes, NW = 1 or 2) lies along the rows of every lane's matrix, so its match vectors are
// the same for all 64 lanes: a table of 256 rows of NW dwords in the wavefront's slice of LDS, row c = the rows of the query that hold
// byte c, built once per query with one ds_or_b32 per query byte.  A column then costs each lane ONE lookup with its own target byte --
// no byte-test tree, and no cross-lane traffic at all: the whole column (Pv / Mv, Myers 1999 in Hyyro's D0 form, as lev_widebits_body.h
// :60-100) sits in the lane's registers, the +1 of row 0 carries in at bit 0, TRANS adds Hyyro's transposition term.  The score is
// followed at the query's last row: it starts at m (column 0) and takes the Ph / Mh bit of row m of every column; a lane whose target has
// ended keeps computing (garbage, unread) with its score frozen.
//
// A pair is a hit with distance d exactly when levenshtein_simd_k_with_opts(query, target, k, false, costs) is Some(d)
// (src/levenshtein.rs:714-720; None above k :539-541, and for lengths more than k apart :426-428).  That last test is the prefilter: such
// a pair is None without any column work, and a query that no live lane of the wavefront can match is skipped whole (no table either).
//
// The table is all zero between queries: a query clears exactly the rows it set, so the 256 NW dwords are zeroed once per wavefront.
#pragma once
#include <stdint.h>

#include "wave.h"

namespace ta {

template <class W, int NW, bool TRANS>
struct LevCross {
    static_assert(NW == 1 || NW == 2, "queries of up to 32 or 64 bytes");
    static constexpr uint32_t MAX_QUERY = 32u * NW;
    static constexpr uint32_t ROW = 4u * NW;                     // bytes per table row
    static constexpr uint32_t LDS_BYTES = 256u * ROW;            // per wavefront
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

    // what a lane keeps of its target across the queries of a tile: its first 16 bytes (a barcode never loads again)
    static TA_HD inline Q first_piece(Ptr tp, U32 tl, Bool live) { return W::gload16(tp, W::land(live, tl > 0u)); }

    // The 64 answers of query qp[0 .. m) (m <= MAX_QUERY), unit threshold k: the distance, or 0xFFFFFFFF for None and for lanes that are
    // not live.  tp / tl: each lane's target; first = first_piece of it.  `skip` gets the lanes the length prefilter answered;
    // returns false when it answered every live lane, the query then having cost no table and no column.
    static TA_HD inline bool query(uint8_t *lds, const uint8_t *qp, uint32_t m, Ptr tp, U32 tl, Bool live, const Q &first, uint32_t k,
                                   U32 &res, Bool &skip) {
        const U32 lane = W::lane();
        const U32 none = W::splat(0xFFFFFFFFu);
        const U32 diff = W::sel(tl > m, tl - m, W::splat(m) - tl);
        skip = W::land(live, diff > k);                           // :426-428
        const Bool work = W::land(live, !(diff > k));
        res = none;
        if (!W::any(work)) return false;
        if (m == 0) {                                            // one gap run: len(t), within k by the prefilter
            res = W::sel(work, tl, none);
            return true;
        }
        // ---- the query's table: lane i sets bit i of row q[i]
        const Bool mine = lane < m;
        const U32 qb = W::gload_u8(W::ptr_add(W::ptr_splat(qp), lane), mine);
        const U32 slot = qb * ROW + (NW == 2 ? (lane >> 5) * 4u : W::splat(0));
        W::lds_or32(lds, slot, W::shlv(W::splat(1), lane & 31u), mine);
        W::lds_wave_sync();

        const U32 tle = W::sel(work, tl, W::splat(0));            // columns whose score counts
        const uint32_t cols = W::wave_max(tle);
        const uint32_t top = (m - 1u) >> 5, sb = (m - 1u) & 31u;  // the query's last row: word and bit
        U32 Pv[NW], Mv[NW], D0p[NW], Eqp[NW];
#pragma unroll
        for (int q = 0; q < NW; q++) {
            Pv[q] = W::splat(0xFFFFFFFFu); Mv[q] = W::splat(0);  // column 0: D grows by 1 per row
            D0p[q] = W::splat(0xFFFFFFFFu); Eqp[q] = W::splat(0);
        }
        U32 score = W::splat(m);
        for (uint32_t j0 = 0; j0 < cols; j0 += 16u) {
            // 16 target bytes (up to 15 past the target's end: the blob's slack); a lane past its end reads nothing and looks up row 0
            const Q piece = j0 ? W::gload16(W::ptr_add(tp, W::splat(j0)), W::splat(j0) < tle) : first;
            const U32 w4[4] = {W::qword(piece, 0), W::qword(piece, 1), W::qword(piece, 2), W::qword(piece, 3)};
#pragma unroll
            for (int r = 0; r < 16; r++) {
                if (r == 8 && j0 + 8u >= cols) break;             // (wave-uniform: the second half of the piece holds no live column)
                const U32 c = W::byte_of(w4[r >> 2], r & 3);
                U32 Eq[NW], D0[NW], Ph[NW], Mh[NW];
                if (NW == 2) W::lds_read64(lds, c * ROW, Eq[0], Eq[NW - 1]);
                else Eq[0] = W::lds_read32(lds, c * ROW);
                Bool carry = W::bfalse();
#pragma unroll
                for (int q = 0; q < NW; q++) {
                    U32 s;
                    W::addc(Eq[q] & Pv[q], Pv[q], carry, s, carry);
                    D0[q] = ((s ^ Pv[q]) | Eq[q]) | Mv[q];
                }
                if (TRANS) {                                      // D0 |= ((~D0_prev & Eq) << 1) & Eq_prev  (src/levenshtein.rs:517-525)
                    U32 X[NW];
#pragma unroll
                    for (int q = 0; q < NW; q++) X[q] = ~D0p[q] & Eq[q];
#pragma unroll
                    for (int q = 0; q < NW; q++) D0[q] = D0[q] | (W::template alignbit<31>(X[q], q ? X[q - 1] : W::splat(0)) & Eqp[q]);
                }
#pragma unroll
                for (int q = 0; q < NW; q++) {
                    Ph[q] = Mv[q] | ~(D0[q] | Pv[q]);
                    Mh[q] = D0[q] & Pv[q];
                }
                const Bool in = W::splat(j0 + (uint32_t)r) < tle;
                const U32 up = W::shr_u(top ? Ph[NW - 1] : Ph[0], sb) & 1u, down = W::shr_u(top ? Mh[NW - 1] : Mh[0], sb) & 1u;
                score = score + W::sel(in, up, W::splat(0)) - W::sel(in, down, W::splat(0));
#pragma unroll
                for (int q = 0; q < NW; q++) {
                    const U32 Phs = W::template alignbit<31>(Ph[q], q ? Ph[q - 1] : W::splat(0x80000000u));   // row 0: D[0][j] - D[0][j-1] = +1
                    const U32 Mhs = W::template alignbit<31>(Mh[q], q ? Mh[q - 1] : W::splat(0));
                    Pv[q] = Mhs | ~(D0[q] | Phs);
                    Mv[q] = Phs & D0[q];
                    if (TRANS) { D0p[q] = D0[q]; Eqp[q] = Eq[q]; }
                }
            }
        }
        // the rows this query set, back to zero
        W::lds_wave_sync();
        W::lds_write32p(lds, slot, W::splat(0), mine);
        W::lds_wave_sync();
        res = W::sel(W::land(work, score <= k), score, none);    // :539-541
        return true;
    }
};

}  // namespace ta
