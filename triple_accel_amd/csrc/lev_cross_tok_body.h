// lev_cross_tok_body.h -- ONE query of 32-bit tokens against the 64 token targets of a wavefront, unit-cost Levenshtein / restricted
// Damerau: the inner step of ta_levenshtein_cross_tokens.
//
// The column, the score at the query's last row, the length prefilter, the m == 0 answer and the frozen score of a lane whose target has
// ended are LevCross<W, NW, TRANS>::query's (lev_cross_body.h).  Two things differ: where Eq comes from, and how a target is fetched.
//
// Eq.  A token has 2^32 values, so the query's match vectors cannot be a table with a row per value.  They sit in a hash table of H slots
// in the wavefront's slice of LDS, a slot = one key dword and NW mask dwords.  Lane i holds q[i]; its mask -- the rows j with q[j] == q[i]
// -- is formed in the wavefront (readlane + compare, m steps).  The lanes then insert without atomics, in rounds: an unplaced lane whose
// probe slot is empty (mask == 0: a placed mask is never zero, lane i's holds bit i) writes its key, one of the competing writers wins,
// every lane reads the key back, a lane that finds its own token writes its mask and is placed (lanes with the same token walk the same
// slots in the same rounds and write the same mask), the others go on to the next slot.  A round places the tokens of every slot that was
// tried, a lane only ever steps over slots taken by other tokens, of which there are at most 63: at most 64 rounds.  A column looks its
// token up by the same probe: the key matches (Eq = the mask), or the slot is empty (Eq = 0).  Every probe loop is bounded by H
// iterations whatever the table holds.
//
// The table is all zero between queries: every lane zeroes the slot it ended on, so the H slots are cleared once per wavefront.
//
// The fetch.  Nothing outside a sequence's items is read: 16-byte pieces are loaded only where all four items lie inside the target.  The
// last 1 .. 3 items of a target of four or more come from the piece that ENDS at the target's end, shifted; a target of fewer than four
// items is read byte by byte, once per wavefront (first_piece).
#pragma once
#include <stdint.h>

#include "wave.h"

namespace ta {

template <class W, int NW, bool TRANS>
struct LevCrossTok {
    static_assert(NW == 1 || NW == 2, "queries of up to 32 or 64 tokens");
    static constexpr uint32_t MAX_QUERY = 32u * NW;
    static constexpr uint32_t LOG2H = 8, H = 1u << LOG2H;        // slots: load <= 64 / 256
    static constexpr uint32_t SLOT = 4u * (1u + NW);             // bytes per slot: the key, then the mask
    static constexpr uint32_t LDS_BYTES = H * SLOT;              // per wavefront
    using U32 = typename W::U32;
    using Bool = typename W::Bool;
    using Ptr = typename W::Ptr;
    using Q = typename W::Q;

    // the slot a token's probe starts at (any fixed function does: correctness does not depend on it)
    static TA_HD inline U32 home(U32 x) { return (x * W::splat(0x9E3779B1u)) >> (int)(32u - LOG2H); }
    static TA_HD inline U32 next(U32 slot) { return (slot + W::splat(1)) & W::splat(H - 1u); }

    // once per wavefront, before its first query
    static TA_HD inline void clear(uint8_t *lds) {
        const U32 lane_off = W::lane() * 4u;
#pragma unroll
        for (uint32_t e = 0; e < LDS_BYTES; e += 256u) W::lds_write32(lds, lane_off + e, W::splat(0));
        W::lds_wave_sync();
    }

    // one item from its four bytes (targets of fewer than four items only)
    static TA_HD inline U32 item_by_bytes(Ptr tp, uint32_t i, Bool pred) {
        U32 x = W::splat(0);
#pragma unroll
        for (uint32_t b = 0; b < 4u; b++) x = x | (W::gload_u8(W::ptr_add(tp, W::splat(4u * i + b)), pred) << (int)(8u * b));
        return x;
    }

    // what a lane keeps of its target across the queries of a tile: its first four items
    struct First { U32 x[4]; };
    static TA_HD inline First first_piece(Ptr tp, U32 tl, Bool live) {
        const Q q = W::gload16(tp, W::land(live, tl >= 4u));       // (zeros elsewhere)
        First f;
#pragma unroll
        for (int r = 0; r < 4; r++) f.x[r] = W::qword(q, r);
        const Bool few = W::land(live, tl < 4u);
        if (W::any(W::land(few, tl > 0u))) {
#pragma unroll
            for (uint32_t r = 0; r < 3u; r++) f.x[r] = f.x[r] | item_by_bytes(tp, r, W::land(few, tl > r));
        }
        return f;
    }

    // The 64 answers of query qp[0 .. m) (m <= MAX_QUERY), unit threshold k: the distance, or 0xFFFFFFFF for None and for lanes that are
    // not live.  tp / tl: each lane's target (tl items from the byte address tp); first = first_piece of it.  `skip` gets the lanes the
    // length prefilter answered; returns false when it answered every live lane, the query then having cost no table and no column.
    static TA_HD inline bool query(uint8_t *lds, const uint32_t *qp, uint32_t m, Ptr tp, U32 tl, Bool live, const First &first, uint32_t k,
                                   U32 &res, Bool &skip) {
        const U32 lane = W::lane();
        const U32 none = W::splat(0xFFFFFFFFu);
        const U32 diff = W::sel(tl > m, tl - m, W::splat(m) - tl);
        skip = W::land(live, diff > k);
        const Bool work = W::land(live, !(diff > k));
        res = none;
        if (!W::any(work)) return false;
        if (m == 0) {                                            // one gap run: len(t), within k by the prefilter
            res = W::sel(work, tl, none);
            return true;
        }
        // ---- lane i's mask: the rows that hold q[i]
        const Bool mine = lane < m;
        const U32 qv = W::load_u32(qp, lane, mine, 0u);
        U32 mk[NW];
#pragma unroll
        for (int w = 0; w < NW; w++) {
            mk[w] = W::splat(0);
            const uint32_t hi = m < 32u * (uint32_t)(w + 1) ? m : 32u * (uint32_t)(w + 1);
            for (uint32_t j = 32u * (uint32_t)w; j < hi; j++)
                mk[w] = mk[w] | W::sel(qv == W::splat(W::readlane(qv, j)), W::splat(1u << (j & 31u)), W::splat(0));
        }
        // ---- insertion in rounds (no atomics): see the head of the file
        U32 slot = home(qv);
        {
            Bool unplaced = mine;
            for (uint32_t round = 0; round < H && W::any(unplaced); round++) {
                const U32 at = slot * SLOT;
                U32 held[NW];
                if (NW == 2) W::lds_read64(lds, at + 4u, held[0], held[NW - 1]);
                else held[0] = W::lds_read32(lds, at + 4u);
                const Bool empty = (NW == 2 ? held[0] | held[NW - 1] : held[0]) == 0u;
                W::lds_write32p(lds, at, qv, W::land(unplaced, empty));
                W::lds_wave_sync();
                const Bool own = W::land(unplaced, W::lds_read32(lds, at) == qv);
#pragma unroll
                for (int w = 0; w < NW; w++) W::lds_write32p(lds, at + 4u + 4u * (uint32_t)w, mk[w], own);
                W::lds_wave_sync();
                unplaced = W::land(unplaced, !own);
                slot = W::sel(unplaced, next(slot), slot);
            }
        }

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
        for (uint32_t j0 = 0; j0 < cols; j0 += 4u) {
            // four items: the piece at j0 where it lies inside the target, else (the target's last 1 .. 3 items) the piece that ends at its
            // end, shifted down; a lane past its end reads nothing
            U32 x[4];
            if (j0 == 0) {
#pragma unroll
                for (int r = 0; r < 4; r++) x[r] = first.x[r];
            } else {
                const U32 left = tle - W::umin(tle, W::splat(j0));                      // items from j0 on
                const Bool whole = left >= 4u, tail = W::land(left > 0u, left < 4u);
                const U32 from = W::sel(whole, W::splat(j0), tle - W::umin(tle, W::splat(4)));   // (a tail lane: tle >= j0 + 1 >= 5)
                // (a target may hold 2^30 items and more: the byte offset 4 from does not fit 32 bits -- four pointer steps of `from`)
                const Ptr at = W::ptr_add(W::ptr_add(W::ptr_add(W::ptr_add(tp, from), from), from), from);
                const Q piece = W::gload16(at, left > 0u);
                const U32 p0 = W::qword(piece, 0), p1 = W::qword(piece, 1), p2 = W::qword(piece, 2), p3 = W::qword(piece, 3);
                const Bool l1 = W::land(tail, left == 1u), l2 = W::land(tail, left == 2u), l3 = W::land(tail, left == 3u);
                x[0] = W::sel(l1, p3, W::sel(l2, p2, W::sel(l3, p1, p0)));
                x[1] = W::sel(l2, p3, W::sel(l3, p2, p1));
                x[2] = W::sel(l3, p3, p2);
                x[3] = p3;
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                if (r && j0 + (uint32_t)r >= cols) break;         // (wave-uniform: no live column from here on)
                const Bool in = W::splat(j0 + (uint32_t)r) < tle;
                // ---- Eq: the mask of x[r]'s slot, 0 when the probe reaches an empty one
                U32 Eq[NW], D0[NW], Ph[NW], Mh[NW];
#pragma unroll
                for (int q = 0; q < NW; q++) Eq[q] = W::splat(0);
                {
                    U32 at = home(x[r]) * SLOT;
                    Bool pend = in;
                    for (uint32_t probe = 0; probe < H; probe++) {
                        U32 key, held[NW];
                        W::lds_read64(lds, at, key, held[0]);
                        if (NW == 2) held[NW - 1] = W::lds_read32(lds, at + 8u);
                        const Bool empty = (NW == 2 ? held[0] | held[NW - 1] : held[0]) == 0u;
                        const Bool found = W::land(pend, W::land(!empty, key == x[r]));
#pragma unroll
                        for (int q = 0; q < NW; q++) Eq[q] = W::sel(found, held[q], Eq[q]);
                        pend = W::land(pend, W::land(!empty, !found));
                        if (!W::any(pend)) break;
                        at = W::sel(at == W::splat((H - 1u) * SLOT), W::splat(0), at + SLOT);
                    }
                }
                Bool carry = W::bfalse();
#pragma unroll
                for (int q = 0; q < NW; q++) {
                    U32 s;
                    W::addc(Eq[q] & Pv[q], Pv[q], carry, s, carry);
                    D0[q] = ((s ^ Pv[q]) | Eq[q]) | Mv[q];
                }
                if (TRANS) {                                      // D0 |= ((~D0_prev & Eq) << 1) & Eq_prev
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
        // the slots this query took, back to zero
        W::lds_wave_sync();
        {
            const U32 at = slot * SLOT;
#pragma unroll
            for (uint32_t e = 0; e < SLOT; e += 4u) W::lds_write32p(lds, at + e, W::splat(0), mine);
        }
        W::lds_wave_sync();
        res = W::sel(W::land(work, score <= k), score, none);
        return true;
    }
};

}  // namespace ta
