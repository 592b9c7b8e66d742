// lev_cross_walk.h -- what a wavefront of lev_cross_kernel / lev_cross_win_kernel does: its 64 targets against a
// tile of P.qtile queries, one call of the body B (lev_cross_body.h or lev_cross_win_body.h) per query.
//
// The lanes that hit are counted with a ballot: one atomic on the 64-bit counter per wavefront and query (and one on the query's own
// count where the caller asks for it), every hitting lane writes its record at base + its prefix count while that is below cap.
// Nearest: the smallest distance of the wavefront, its lowest target, one 64-bit atomicMin per wavefront and query.  Under
// TA_CROSS_UPPER only the pairs with target > query count, and, as in ham_cross.hip, a wavefront stops its tile at the query that
// reaches its last live target and leaves at once when the tile starts there.  Nothing of size nq x nt exists anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ta_internal.h"
#include "wave.h"

namespace ta {

// What a wavefront does with the 64 answers of query q (res: the unit distance of the lane's target t, 0xFFFFFFFF for no hit): the epilogue
// of every walk (below; lev_cross_tok.hip)
template <bool OPTS>
__device__ __forceinline__ void lev_cross_emit(const CrossParams &P, uint32_t q, uint32_t t, uint32_t lane, uint32_t res, bool upper) {
    bool hit = res != 0xFFFFFFFFu;
    if (upper) hit = hit && t > q;
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
    unsigned long long base = 0;
    if (lane == leader) {
        base = atomicAdd(P.count, (unsigned long long)__popcll(mask));
        if (OPTS && P.per_query) atomicAdd(P.per_query + q, (uint32_t)__popcll(mask));
    }
    base = ((unsigned long long)__builtin_amdgcn_readlane((uint32_t)(base >> 32), leader) << 32) |
           __builtin_amdgcn_readlane((uint32_t)base, leader);
    const unsigned long long idx = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    const uint32_t d = res * P.g;                                  // (g d <= k: no overflow)
    if (hit && idx < P.cap) P.hits[idx] = ta_cross_hit{q, t, d, 0u};
    if (P.nearest) {
        const uint32_t dmin = ~DevWave::wave_max(hit ? ~res : 0u);
        const unsigned long long best = __ballot(hit && res == dmin);
        if (lane == (uint32_t)__ffsll((long long)best) - 1u) atomicMin(P.nearest + q, ((unsigned long long)d << 32) | t);
    }
}

// OPTS: the call asks for TA_CROSS_UPPER or the per-query counts; without it the walk is ta_levenshtein_cross's as it always was
template <class B, bool OPTS>
__device__ __forceinline__ void lev_cross_walk(const CrossParams &P, uint8_t *tables) {
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t t0 = ((uint64_t)blockIdx.x * 4u + wave) * 64u;
    if (t0 >= P.nt) return;                                        // (no workgroup barrier below: a wavefront may leave)
    const bool upper = OPTS && (P.flags & TA_CROSS_UPPER) != 0;
    const uint64_t q0 = (uint64_t)blockIdx.y * P.qtile;
    uint64_t q1 = q0 + P.qtile < P.nq ? q0 + P.qtile : P.nq;
    if (upper) {                                                   // only queries below the wavefront's last live target
        const uint64_t last = t0 + 63u < P.nt ? t0 + 63u : (uint64_t)P.nt - 1u;
        if (q1 > last) q1 = last;
        if (q0 >= q1) return;
    }
    uint8_t *lds = tables + wave * B::LDS_BYTES;
    const uint32_t lane = DevWave::lane();
    const uint32_t t = (uint32_t)t0 + lane;
    const bool live = t < P.nt;
    const uint8_t *tp;
    uint32_t tl;
    DevWave::load_str(P.t, t, live, tp, tl);
    B::clear(lds);
    const Q128 first = B::first_piece(tp, tl, live);
    for (uint32_t q = (uint32_t)q0; q < (uint32_t)q1; q++) {
        const uint8_t *qp;
        uint64_t m64;
        if (P.q.off) {
            const uint64_t o0 = P.q.off[q], o1 = P.q.off[q + 1];
            qp = P.q.blob + o0;
            m64 = o1 - o0;
        } else {
            qp = P.q.blob + (uint64_t)q * P.q.stride;
            m64 = P.q.len;
        }
        const uint32_t m = m64 < B::MAX_QUERY ? (uint32_t)m64 : B::MAX_QUERY;   // (the caller's bound: no clamp in a valid call)
        uint32_t res;
        bool skip;
        if (!B::query(lds, qp, m, tp, tl, live, first, P.k, res, skip)) continue;
        lev_cross_emit<OPTS>(P, q, t, lane, res, upper);
    }
}

}  // namespace ta
