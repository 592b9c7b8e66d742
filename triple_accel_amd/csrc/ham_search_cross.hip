// ham_search_cross.hip -- gfx950 kernels of ta_hamming_search_cross: every needle of a panel in every haystack, substitutions only
// (DESIGN.md 3.16).
//
// Scan: a workgroup of 512 threads builds ONE group's mismatch table mis[256][64] in LDS -- column l the rows of needle l mod G of the
// group -- and its eight wavefronts then walk the workgroup's haystacks, 64 / G of them per wavefront and step: every lane of a slot
// reads the same haystack bytes and looks its own column up (mis[c * 64 + lane]: no two lanes of a 32-lane half share a bank whatever the
// bytes are; the address is one v_perm of the haystack dword).  The bit-sliced counters give the exact mismatch count of every window
// within the threshold, folded into the lane's Best triple on the spot.  At the end of a haystack a lane with a hit puts its record into
// its wavefront's stage in LDS (flushed with one atomic per 64 records), bumps the haystack's count and folds its packed word into the
// haystack's minimum.
// Finish: one lane per haystack unpacks the word into nearest[i] and best[i].
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ham_search_cross_body.h"
#include "ta_internal.h"

namespace ta {

__device__ __forceinline__ void hsx_str(const StrView &s, uint32_t i, const uint8_t *&p, uint64_t &len) {
    if (s.off) {
        const uint64_t o0 = s.off[i], o1 = s.off[i + 1];
        p = s.blob + o0;
        len = o1 - o0;
    } else {
        p = s.blob + (uint64_t)i * s.stride;
        len = s.len;
    }
}

template <int B>
__global__ __launch_bounds__(512) void ham_search_cross_kernel(HamSearchCrossParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t mis[256 * SX_GROUP];
    __shared__ ta_search_cross_hit stage[SX_WAVES][HSX_STAGE];                    // 12 KB: 76 KB per workgroup, two workgroups per CU
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t g0 = blockIdx.y * SX_GROUP;
    const uint32_t size = sx_group_size(P.nn, blockIdx.y), G = sx_group_cols(size), S = SX_GROUP / G;
    const uint32_t col = lane & (G - 1u), slot = lane / G;
    const bool has_needle = col < size;
    const uint32_t needle = g0 + col;
    const uint8_t *np = nullptr;
    uint32_t n = 0;
    if (has_needle) {
        uint64_t nl;
        hsx_str(P.nd, needle, np, nl);
        n = nl < (uint64_t)SX_MAX_NEEDLE + 1u ? (uint32_t)nl : SX_MAX_NEEDLE + 1u;   // (max_len bounds every needle: 33 in no valid call)
    }
    const bool scans = has_needle && hsx_scans(n);
    // the table: wavefront w fills rows 32 w .. 32 w + 31 of its lanes' columns with "every position mismatches", then (behind a barrier)
    // needle byte j clears its bit, byte j by wavefront j mod 8 -- two bytes of one needle may name the same row: an LDS atomic
    const uint32_t full = scans ? hsx_mis_full(n) : 0u;
#pragma unroll 8
    for (uint32_t c = wave * 32u; c < wave * 32u + 32u; c++) mis[c * SX_GROUP + lane] = full;
    __syncthreads();
    if (scans)
        for (uint32_t j = wave; j < n; j += SX_WAVES) atomicAnd(&mis[(uint32_t)np[j] * SX_GROUP + lane], ~hsx_mis_bit(n, j));
    __syncthreads();

    const uint32_t lane_off = lane * 4u;
    auto lookup = [&](uint32_t w, int b) -> uint32_t {                            // byte b of w << 8 | lane * 4
        const uint32_t a = __builtin_amdgcn_perm(w, lane_off, 0x0C0C0000u | ((4u + (uint32_t)b) << 8));
        return *(const uint32_t *)((const uint8_t *)mis + a);
    };
    auto any = [](bool p) -> bool { return __ballot(p) != 0ull; };
    // the wavefront's staged records go out: ONE add to the counter for up to 64 records (one add per wavefront and step made a million
    // returning atomics on one address of a million haystacks with a hit each: they serialise at the memory side)
    auto flush = [&](uint32_t cnt) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(P.count, (unsigned long long)cnt);
        base = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)base);
        if (lane < cnt && base + lane < P.cap) P.hits[base + lane] = stage[wave][lane];
        __builtin_amdgcn_wave_barrier();
    };
    uint32_t staged = 0;                                                          // records in the wavefront's stage (wavefront-uniform)

    const uint64_t wg0 = (uint64_t)blockIdx.x * P.hpw;                            // the workgroup's haystacks: [wg0, wg1)
    const uint64_t wg1 = wg0 + P.hpw < P.nh ? wg0 + P.hpw : P.nh;
    for (uint32_t it = 0;; it++) {
        if (wg0 + sx_local_hay(it, wave, S, 0) >= wg1) break;                    // (wavefront-uniform: the ballot below sees every lane)
        const uint64_t hi = wg0 + sx_local_hay(it, wave, S, slot);
        HsxBest r = {TA_NONE, 0u, 0u, false};
        bool live = false;                                                       // 1 <= n <= h: the pairs the reference looks at
        if (scans && hi < wg1) {
            const uint8_t *hay;
            uint64_t h;
            hsx_str(P.hs, (uint32_t)hi, hay, h);
            live = (uint64_t)n <= h;
            if (live) hsx_scan_pair<B>(hay, (uint32_t)h, lookup, n, P.kc, any, r);
        }
        const bool hit = live && !r.nul && r.count != 0u;
        if (live && r.nul && P.per_haystack) P.per_haystack[hi] = TA_NONE;       // (every lane of the haystack stores the same word)
        const unsigned long long mask = __ballot(hit);
        if (!mask) continue;
        const uint32_t hits_now = (uint32_t)__popcll(mask);
        if (staged + hits_now > HSX_STAGE) { flush(staged); staged = 0; }          // (wavefront-uniform)
        if (hit) {
            stage[wave][staged + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] =
                ta_search_cross_hit{(uint32_t)hi, needle, r.start, r.start + n, r.d, r.count};
            if (P.per_haystack) atomicAdd(P.per_haystack + hi, 1u);
            if (P.packed) atomicMin(P.packed + hi, (unsigned long long)hsx_word(r.d, needle, r.start));
        }
        staged += hits_now;
    }
    if (staged) flush(staged);
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
            hsx_str(P.nd, hsx_word_needle(w), np, nl);
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
