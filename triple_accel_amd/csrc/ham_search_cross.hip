// ham_search_cross.hip -- gfx950 kernels of ta_hamming_search_cross: every needle of a panel in every haystack, substitutions only
// (DESIGN.md 3.16).
//
// Scan: a workgroup of 512 threads builds ONE group's mismatch table mis[256][64] in LDS -- column l the rows of needle l mod G of the
// group -- and its eight wavefronts then walk the workgroup's haystacks, 64 / G of them per wavefront and step: every lane of a slot
// reads the same haystack bytes and looks its own column up (mis[c * 64 + lane]: no two lanes of a 32-lane half share a bank whatever the
// bytes are; the address is one v_perm of the haystack dword).  The bit-sliced counters give the exact mismatch count of every window
// within the threshold, folded into the lane's Best triple on the spot.  At the end of a haystack a lane with a hit puts its record into
// its wavefront's stage in LDS (flushed with one atomic per 64 records), bumps the haystack's count and folds its packed word into the
// haystack's minimum.  Lane ownership, the walk and that tail (hsx_walk_emit) are search_cross_dev.h's, shared with
// ham_search_cross_w2.hip.
// Finish: one lane per haystack unpacks the word into nearest[i] and best[i].
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ham_search_cross_body.h"
#include "lds_tab64.h"
#include "search_cross_dev.h"
#include "ta_internal.h"

namespace ta {

template <int B>
__global__ __launch_bounds__(512) void ham_search_cross_kernel(HamSearchCrossParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t mis[256 * SX_GROUP];
    __shared__ ta_search_cross_hit stage[SX_WAVES][HSX_STAGE];                    // 12 KB: 76 KB per workgroup, two workgroups per CU
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const SxLane L = sx_lane(P.nd, P.nn, blockIdx.y, SX_GROUP, SX_MAX_NEEDLE + 1u);   // (max_len bounds every needle: 33 in no valid call)
    const uint32_t n = L.n;
    const bool scans = L.has_needle && hsx_scans(n);
    // the table: wavefront w fills rows 32 w .. 32 w + 31 of its lanes' columns with "every position mismatches", then (behind a barrier)
    // needle byte j clears its bit, byte j by wavefront j mod 8 -- two bytes of one needle may name the same row: an LDS atomic
    const uint32_t full = scans ? hsx_mis_full(n) : 0u;
#pragma unroll 8
    for (uint32_t c = wave * 32u; c < wave * 32u + 32u; c++) mis[c * SX_GROUP + lane] = full;
    __syncthreads();
    if (scans)
        for (uint32_t j = wave; j < n; j += SX_WAVES) atomicAnd(&mis[(uint32_t)L.np[j] * SX_GROUP + lane], ~hsx_mis_bit(n, j));
    __syncthreads();

    const uint32_t lane_off = lane * 4u;
    auto lookup = [&](uint32_t w, int b) -> uint32_t { return tab64_lookup(mis, lane_off, w, b); };
    hsx_walk_emit(P, L, scans, stage[wave], [&](const uint8_t *hay, uint32_t h, auto any, HsxBest &r) {
        hsx_scan_pair<B>(hay, h, lookup, n, P.kc, any, r);
    });
}

__global__ __launch_bounds__(256) void ham_search_cross_finish_kernel(HamSearchCrossParams P) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.nh) return;
    const uint64_t w = P.packed[i];
    if (P.nearest) P.nearest[i] = hsx_nearest(w);
    if (P.best) {
        uint64_t nl = 0;
        if (w != ~0ull) {
            const uint8_t *np;
            dev_str(P.nd, hsx_word_needle(w), np, nl);
        }
        P.best[i] = hsx_best(w, (uint32_t)nl);
    }
}

hipError_t ham_search_cross_launch(const HamSearchCrossParams &P, hipStream_t st) {
    if (P.nh == 0 || P.nn == 0 || P.hpw == 0) return hipSuccess;
    const uint32_t groups = (P.nn + SX_GROUP - 1) / SX_GROUP;
    if (groups > 65535u) return hipErrorInvalidValue;
    const int planes = hsx_planes(P.kc);
    const dim3 grid((P.nh + P.hpw - 1) / P.hpw, groups), block(512);
    set_last_kernel_name("ham_search_cross_kernel<%d>", planes);
    switch (planes) {
        case 1: hipLaunchKernelGGL(ham_search_cross_kernel<1>, grid, block, 0, st, P); break;
        case 2: hipLaunchKernelGGL(ham_search_cross_kernel<2>, grid, block, 0, st, P); break;
        case 3: hipLaunchKernelGGL(ham_search_cross_kernel<3>, grid, block, 0, st, P); break;
        case 4: hipLaunchKernelGGL(ham_search_cross_kernel<4>, grid, block, 0, st, P); break;
        case 5: hipLaunchKernelGGL(ham_search_cross_kernel<5>, grid, block, 0, st, P); break;
        case 6: hipLaunchKernelGGL(ham_search_cross_kernel<6>, grid, block, 0, st, P); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t ham_search_cross_finish_launch(const HamSearchCrossParams &P, hipStream_t st) {
    if (P.nh == 0 || !P.packed || (!P.nearest && !P.best)) return hipSuccess;
    hipLaunchKernelGGL(ham_search_cross_finish_kernel, dim3((P.nh + 255u) / 256u), dim3(256), 0, st, P);
    return hipGetLastError();
}

}  // namespace ta
