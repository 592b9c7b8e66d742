// ham_cross.hip -- gfx950 kernel of ta_hamming_cross: every query against every target within k mismatches.
//
// One lane per target, 64 targets per wavefront, four wavefronts per workgroup; a wavefront loads its targets into registers once and
// walks a tile of P.qtile queries with ham_cross_body.h, a chunk of 256 / NW queries staged through its own 1.25 KB of LDS at a time.
// Hits, count and nearest are lev_cross.hip's sequence: a ballot of the hitting lanes, one atomic on the 64-bit counter per wavefront
// and query, every hitting lane writes its record at base + its prefix count while that is below cap, one 64-bit atomicMin for the
// wavefront's nearest; the per-query count is one more atomicAdd of the ballot's popcount by the same leader.  Under TA_CROSS_UPPER a
// wavefront stops its tile at the query that reaches its last target (the later ones have no target above them: no staging, no
// compare) and leaves at once when the tile starts there.  Nothing of size nq x nt exists anywhere.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ham_cross_body.h"
#include "ta_internal.h"

namespace ta {

template <int NW>
__global__ __launch_bounds__(256) void ham_cross_kernel(HamCrossParams P) {
    using B = HamCross<DevWave, NW>;
    __shared__ __attribute__((aligned(16))) uint8_t slices[4u * B::LDS_BYTES];
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t t0 = ((uint64_t)blockIdx.x * 4u + wave) * 64u;
    if (t0 >= P.nt) return;                                        // (no workgroup barrier below: a wavefront may leave)
    const uint64_t q0 = (uint64_t)blockIdx.y * P.qtile;
    uint64_t q1 = q0 + P.qtile < P.nq ? q0 + P.qtile : P.nq;
    if (P.upper) {                                                 // only queries below the wavefront's last live target
        const uint64_t last = t0 + 63u < P.nt ? t0 + 63u : (uint64_t)P.nt - 1u;
        if (q1 > last) q1 = last;
    }
    if (q0 >= q1) return;
    uint8_t *lds = slices + wave * B::LDS_BYTES;
    const uint32_t lane = DevWave::lane();
    const uint32_t t = (uint32_t)t0 + lane;
    const bool live = t < P.nt;
    const uint8_t *tp;
    uint32_t tl;
    DevWave::load_str(P.t, t, live, tp, tl);
    uint32_t tw[NW];
    const bool usable = B::load_target(tp, tl, live, tw);
    for (uint64_t c0 = q0; c0 < q1; c0 += B::CHUNK) {
        const uint32_t n = q1 - c0 < B::CHUNK ? (uint32_t)(q1 - c0) : B::CHUNK;
        B::stage(lds, P.q, (uint32_t)c0, n);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t q = (uint32_t)c0 + i;
            bool hit;
            uint32_t d;
            if (!B::compare(lds, i, tw, tl, usable, P.k8, hit, d)) continue;
            if (P.upper) hit = hit && t > q;
            const unsigned long long mask = __ballot(hit);
            if (!mask) continue;
            const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
            unsigned long long base = 0;
            if (lane == leader) {
                base = atomicAdd(P.count, (unsigned long long)__popcll(mask));
                if (P.per_query) atomicAdd(P.per_query + q, (uint32_t)__popcll(mask));
            }
            base = ((unsigned long long)__builtin_amdgcn_readlane((uint32_t)(base >> 32), leader) << 32) |
                   __builtin_amdgcn_readlane((uint32_t)base, leader);
            const unsigned long long idx = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (hit && idx < P.cap) P.hits[idx] = ta_cross_hit{q, t, d, 0u};
            if (P.nearest) {
                const uint32_t dmin = ~DevWave::wave_max(hit ? ~d : 0u);
                const unsigned long long best = __ballot(hit && d == dmin);
                if (lane == (uint32_t)__ffsll((long long)best) - 1u) atomicMin(P.nearest + q, ((unsigned long long)d << 32) | t);
            }
        }
    }
}

hipError_t ham_cross_launch(const HamCrossParams &P, int nw, hipStream_t st) {
    if (P.nq == 0 || P.nt == 0) return hipSuccess;
    if (P.qtile == 0 || (nw != 4 && nw != 8 && nw != 16)) return hipErrorInvalidValue;
    const uint32_t tgroups = (uint32_t)(((uint64_t)P.nt + 63u) / 64u);
    const uint64_t qtiles = ((uint64_t)P.nq + P.qtile - 1u) / P.qtile;
    if (qtiles > 65535u) return hipErrorInvalidValue;
    const dim3 grid((tgroups + 3u) / 4u, (uint32_t)qtiles), block(256);
    set_last_kernel_name("ham_cross_kernel<%d>", nw);
    if (nw == 4) hipLaunchKernelGGL((ham_cross_kernel<4>), grid, block, 0, st, P);
    else if (nw == 8) hipLaunchKernelGGL((ham_cross_kernel<8>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((ham_cross_kernel<16>), grid, block, 0, st, P);
    return hipGetLastError();
}

}  // namespace ta
