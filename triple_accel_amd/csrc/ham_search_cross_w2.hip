// ham_search_cross_w2.hip -- gfx950 kernel of ta_hamming_search_cross_with_opts's two-word route: a panel whose longest needle is 33..64
// bytes, every needle in every haystack, substitutions only.  The finish kernel is ham_search_cross.hip's: it reads a
// needle's length from the needle side and does not care how long it is.
//
// Scan: a workgroup of 512 threads builds ONE group's mismatch table in LDS -- 256 rows of 32 columns of 2 words, 64 KB as the one-word
// table, so two workgroups share a CU's 160 KB: four wavefronts per SIMD -- and its eight wavefronts then walk the workgroup's
// haystacks, 64 / G >= 2 of them per wavefront and step.  Lane l reads column l mod 32 (needle l mod G of the group: the columns repeat
// the group's needles where G < 32), both words with ONE ds_read_b64 at byte c * 256 + (l mod 32) * 8 (the address is one v_perm of the
// haystack dword).  The bank argument: ds_read_b64 serves a 32-lane half per pass and banks dwords modulo 64; the lanes of a half read 32
// different columns, so their 64 dwords are banks 2 (l mod 32) + {0, 1} of ONE 256-byte row each -- every bank once, whatever the
// haystacks' bytes c are and however many slots (haystacks) a half holds.  Lanes l and l + 32 share a column but sit in different
// halves: they never meet.  The build's stores and atomics run once per workgroup.
// The two-word counters give the exact mismatch count of every window within the threshold, folded into the lane's Best triple on the
// spot.  Lane ownership, the walk, the stage, its flush, the per-haystack count and the packed word are search_cross_dev.h's
// (hsx_walk_emit), shared with ham_search_cross.hip.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ham_search_cross_w2_body.h"
#include "lds_tab64.h"
#include "search_cross_dev.h"
#include "ta_internal.h"

namespace ta {

template <int B>
__global__ __launch_bounds__(512) void ham_search_cross_w2_kernel(HamSearchCrossParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t mis[256 * HSX2_GROUP * 2];
    __shared__ ta_search_cross_hit stage[SX_WAVES][HSX_STAGE];                    // 12 KB: 76 KB per workgroup, two workgroups per CU
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t column = lane & (HSX2_GROUP - 1u), half = lane >> 5;
    const SxLane L = sx_lane(P.nd, P.nn, blockIdx.y, HSX2_GROUP, HSX2_MAX_NEEDLE + 1u);   // (max_len bounds every needle: 65 in no valid call)
    const uint32_t n = L.n;
    const bool scans = L.has_needle && hsx2_scans(n);
    // the table: lanes l and l + 32 own one column (the same needle), word l / 32 of it each.  Wavefront w fills rows 32 w .. 32 w + 31
    // with "every position mismatches", then (behind a barrier) needle byte j clears its bit, byte j by half-wavefront j mod 16 -- two
    // bytes of one needle may name the same row: an LDS atomic
    const uint32_t full = scans ? hsx2_mis_full(n, half) : 0u;
#pragma unroll 8
    for (uint32_t c = wave * 32u; c < wave * 32u + 32u; c++) mis[hsx2_mis_at(c, column, half)] = full;
    __syncthreads();
    if (scans)
        for (uint32_t j = wave * 2u + half; j < n; j += 2u * SX_WAVES) {
            uint32_t w;
            const uint32_t bit = hsx2_mis_bit(n, j, w);
            atomicAnd(&mis[hsx2_mis_at((uint32_t)L.np[j], column, w)], ~bit);
        }
    __syncthreads();

    const uint32_t lane_off = column * 8u;
    auto lookup = [&](uint32_t w, int b) -> HamBits2Word {                        // both words of the column: one ds_read_b64
        const u32x2 v = tab64_lookup<u32x2>(mis, lane_off, w, b);
        return HamBits2Word{v.x, v.y};
    };
    hsx_walk_emit(P, L, scans, stage[wave], [&](const uint8_t *hay, uint32_t h, auto any, HsxBest &r) {
        hsx2_scan_pair<B>(hay, h, lookup, n, P.kc, any, r);
    });
}

hipError_t ham_search_cross_w2_launch(const HamSearchCrossParams &P, hipStream_t st) {
    if (P.nh == 0 || P.nn == 0 || P.hpw == 0) return hipSuccess;
    const uint32_t groups = (P.nn + HSX2_GROUP - 1) / HSX2_GROUP;
    if (groups > 65535u) return hipErrorInvalidValue;
    const int planes = hsx2_planes(P.kc);
    const dim3 grid((P.nh + P.hpw - 1) / P.hpw, groups), block(512);
    set_last_kernel_name("ham_search_cross_w2_kernel<%d>", planes);
    switch (planes) {
        case 1: hipLaunchKernelGGL(ham_search_cross_w2_kernel<1>, grid, block, 0, st, P); break;
        case 2: hipLaunchKernelGGL(ham_search_cross_w2_kernel<2>, grid, block, 0, st, P); break;
        case 3: hipLaunchKernelGGL(ham_search_cross_w2_kernel<3>, grid, block, 0, st, P); break;
        case 4: hipLaunchKernelGGL(ham_search_cross_w2_kernel<4>, grid, block, 0, st, P); break;
        case 5: hipLaunchKernelGGL(ham_search_cross_w2_kernel<5>, grid, block, 0, st, P); break;
        case 6: hipLaunchKernelGGL(ham_search_cross_w2_kernel<6>, grid, block, 0, st, P); break;
        case 7: hipLaunchKernelGGL(ham_search_cross_w2_kernel<7>, grid, block, 0, st, P); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ta
