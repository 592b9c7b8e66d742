// lev_cross_tok.hip -- gfx950 kernel of ta_levenshtein_cross_tokens: every query of 32-bit tokens against every target within k
// (DESIGN.md 3.20).
//
// lev_cross.hip's shape: one lane per target, 64 targets per wavefront, four wavefronts per workgroup; a wavefront walks a tile of
// P.qtile queries with lev_cross_tok_body.h (the query's match vectors in a hash table in the wavefront's own 2 / 3 KB of LDS, the column
// in the lane's registers).  The walk below differs from lev_cross_walk.h's only in what a sequence is -- items of four bytes behind
// ELEMENT offsets -- and hands the 64 answers of a query to the same epilogue (lev_cross_emit): the count, the records, nearest, the
// per-query count, TA_CROSS_UPPER.  Nothing of size nq x nt exists anywhere.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "lev_cross_tok_body.h"
#include "lev_cross_walk.h"
#include "ta_internal.h"

namespace ta {

// P.q / P.t: StrView over the items (blob = the first item; off, stride and len in ELEMENTS)
template <class B, bool OPTS>
__device__ __forceinline__ void lev_cross_tok_walk(const CrossParams &P, uint8_t *tables) {
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
    const uint8_t *tp = P.t.blob;
    uint32_t tl = 0;
    if (live) {
        if (P.t.off) {
            const uint64_t o0 = P.t.off[t], o1 = P.t.off[t + 1];
            tp = P.t.blob + 4u * o0;
            tl = (uint32_t)(o1 - o0);
        } else {
            tp = P.t.blob + 4u * ((uint64_t)t * P.t.stride);
            tl = (uint32_t)P.t.len;
        }
    }
    B::clear(lds);
    const typename B::First first = B::first_piece(tp, tl, live);
    for (uint32_t q = (uint32_t)q0; q < (uint32_t)q1; q++) {
        const uint32_t *qp;
        uint64_t m64;
        if (P.q.off) {
            const uint64_t o0 = P.q.off[q], o1 = P.q.off[q + 1];
            qp = (const uint32_t *)P.q.blob + o0;
            m64 = o1 - o0;
        } else {
            qp = (const uint32_t *)P.q.blob + (uint64_t)q * P.q.stride;
            m64 = P.q.len;
        }
        const uint32_t m = m64 < B::MAX_QUERY ? (uint32_t)m64 : B::MAX_QUERY;   // (the caller's bound: no clamp in a valid call)
        uint32_t res;
        bool skip;
        if (!B::query(lds, qp, m, tp, tl, live, first, P.k, res, skip)) continue;
        lev_cross_emit<OPTS>(P, q, t, lane, res, upper);
    }
}

template <int NW, bool TRANS, bool OPTS = false>
__global__ __launch_bounds__(256) void lev_cross_tok_kernel(CrossParams P) {
    using B = LevCrossTok<DevWave, NW, TRANS>;
    __shared__ __attribute__((aligned(16))) uint8_t tables[4u * B::LDS_BYTES];
    lev_cross_tok_walk<B, OPTS>(P, tables);
}

template <int NW, bool OPTS>
static void cross_tok_launch(const CrossParams &P, bool trans, dim3 grid, dim3 block, hipStream_t st) {
    if (trans) hipLaunchKernelGGL((lev_cross_tok_kernel<NW, true, OPTS>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((lev_cross_tok_kernel<NW, false, OPTS>), grid, block, 0, st, P);
}

hipError_t lev_cross_tok_launch(const CrossParams &P, int nw, bool trans, hipStream_t st) {
    if (P.nq == 0 || P.nt == 0) return hipSuccess;
    if (P.qtile == 0 || (nw != 1 && nw != 2)) return hipErrorInvalidValue;
    const uint32_t tgroups = (uint32_t)(((uint64_t)P.nt + 63u) / 64u);
    const uint64_t qtiles = ((uint64_t)P.nq + P.qtile - 1u) / P.qtile;
    if (qtiles > 65535u) return hipErrorInvalidValue;
    const dim3 grid((tgroups + 3u) / 4u, (uint32_t)qtiles), block(256);
    set_last_kernel_name("lev_cross_tok_kernel<%d, %s>", nw, trans ? "true" : "false");
    const bool opts = P.flags != 0 || P.per_query != nullptr;
    if (nw == 1) {
        if (opts) cross_tok_launch<1, true>(P, trans, grid, block, st);
        else cross_tok_launch<1, false>(P, trans, grid, block, st);
    } else {
        if (opts) cross_tok_launch<2, true>(P, trans, grid, block, st);
        else cross_tok_launch<2, false>(P, trans, grid, block, st);
    }
    return hipGetLastError();
}

}  // namespace ta
