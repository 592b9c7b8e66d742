// lev_cross.hip -- gfx950 kernel of ta_levenshtein_cross: every query against every target within k.
//
// One lane per target, 64 targets per wavefront, four wavefronts per workgroup; a wavefront walks a tile of P.qtile queries with
// lev_cross_body.h (the query's match vectors as a table in the wavefront's own 1 / 2 KB of LDS, the column in the lane's registers).
// The lanes that hit are counted with a ballot: one atomic on the 64-bit counter per wavefront and query, every hitting lane writes its
// record at base + its prefix count while that is below cap.  Nearest: the smallest distance of the wavefront, its lowest target, one
// 64-bit atomicMin per wavefront and query.  Nothing of size nq x nt exists anywhere.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "lev_cross_body.h"
#include "ta_internal.h"

namespace ta {

template <int NW, bool TRANS>
__global__ __launch_bounds__(256) void lev_cross_kernel(CrossParams P) {
    using B = LevCross<DevWave, NW, TRANS>;
    __shared__ __attribute__((aligned(16))) uint8_t tables[4u * B::LDS_BYTES];
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t t0 = ((uint64_t)blockIdx.x * 4u + wave) * 64u;
    if (t0 >= P.nt) return;                                        // (no workgroup barrier below: a wavefront may leave)
    uint8_t *lds = tables + wave * B::LDS_BYTES;
    const uint32_t lane = DevWave::lane();
    const uint32_t t = (uint32_t)t0 + lane;
    const bool live = t < P.nt;
    const uint8_t *tp;
    uint32_t tl;
    DevWave::load_str(P.t, t, live, tp, tl);
    B::clear(lds);
    const Q128 first = B::first_piece(tp, tl, live);
    const uint64_t q0 = (uint64_t)blockIdx.y * P.qtile;
    const uint32_t q1 = (uint32_t)(q0 + P.qtile < P.nq ? q0 + P.qtile : P.nq);
    for (uint32_t q = (uint32_t)q0; q < q1; q++) {
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
        const bool hit = res != 0xFFFFFFFFu;
        const unsigned long long mask = __ballot(hit);
        if (!mask) continue;
        const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(P.count, (unsigned long long)__popcll(mask));
        base = ((unsigned long long)__builtin_amdgcn_readlane((uint32_t)(base >> 32), leader) << 32) |
               __builtin_amdgcn_readlane((uint32_t)base, leader);
        const unsigned long long idx = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        const uint32_t d = res * P.g;                              // (g d <= k: no overflow)
        if (hit && idx < P.cap) P.hits[idx] = ta_cross_hit{q, t, d, 0u};
        if (P.nearest) {
            const uint32_t dmin = ~DevWave::wave_max(hit ? ~res : 0u);
            const unsigned long long best = __ballot(hit && res == dmin);
            if (lane == (uint32_t)__ffsll((long long)best) - 1u) atomicMin(P.nearest + q, ((unsigned long long)d << 32) | t);
        }
    }
}

hipError_t lev_cross_launch(const CrossParams &P, int nw, bool trans, hipStream_t st) {
    if (P.nq == 0 || P.nt == 0) return hipSuccess;
    if (P.qtile == 0 || (nw != 1 && nw != 2)) return hipErrorInvalidValue;
    const uint32_t tgroups = (uint32_t)(((uint64_t)P.nt + 63u) / 64u);
    const uint64_t qtiles = ((uint64_t)P.nq + P.qtile - 1u) / P.qtile;
    if (qtiles > 65535u) return hipErrorInvalidValue;
    const dim3 grid((tgroups + 3u) / 4u, (uint32_t)qtiles), block(256);
    set_last_kernel_name("lev_cross_kernel<%d, %s>", nw, trans ? "true" : "false");
    if (nw == 1) {
        if (trans) hipLaunchKernelGGL((lev_cross_kernel<1, true>), grid, block, 0, st, P);
        else hipLaunchKernelGGL((lev_cross_kernel<1, false>), grid, block, 0, st, P);
    } else {
        if (trans) hipLaunchKernelGGL((lev_cross_kernel<2, true>), grid, block, 0, st, P);
        else hipLaunchKernelGGL((lev_cross_kernel<2, false>), grid, block, 0, st, P);
    }
    return hipGetLastError();
}

}  // namespace ta
