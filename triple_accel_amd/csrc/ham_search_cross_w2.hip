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
// spot; the stage, its flush, the per-haystack count and the packed word are ham_search_cross_kernel's.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ham_search_cross_w2_body.h"
#include "ta_internal.h"

namespace ta {

__device__ __forceinline__ void hsx2_str(const StrView &s, uint32_t i, const uint8_t *&p, uint64_t &len) {
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
__global__ __launch_bounds__(512) void ham_search_cross_w2_kernel(HamSearchCrossParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t mis[256 * HSX2_GROUP * 2];
    __shared__ ta_search_cross_hit stage[SX_WAVES][HSX_STAGE];                    // 12 KB: 76 KB per workgroup, two workgroups per CU
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t g0 = blockIdx.y * HSX2_GROUP;
    const uint32_t size = hsx2_group_size(P.nn, blockIdx.y), G = sx_group_cols(size), S = 64u / G;
    const uint32_t col = lane & (G - 1u), slot = lane / G, column = lane & (HSX2_GROUP - 1u), half = lane >> 5;
    const bool has_needle = col < size;
    const uint32_t needle = g0 + col;
    const uint8_t *np = nullptr;
    uint32_t n = 0;
    if (has_needle) {
        uint64_t nl;
        hsx2_str(P.nd, needle, np, nl);
        n = nl < (uint64_t)HSX2_MAX_NEEDLE + 1u ? (uint32_t)nl : HSX2_MAX_NEEDLE + 1u;   // (max_len bounds every needle: 65 in no valid call)
    }
    const bool scans = has_needle && hsx2_scans(n);
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
            atomicAnd(&mis[hsx2_mis_at((uint32_t)np[j], column, w)], ~bit);
        }
    __syncthreads();

    const uint32_t lane_off = column * 8u;
    auto lookup = [&](uint32_t w, int b) -> HamBits2Word {                        // byte b of w << 8 | column * 8
        const uint32_t a = __builtin_amdgcn_perm(w, lane_off, 0x0C0C0000u | ((4u + (uint32_t)b) << 8));
        const u32x2 v = *(const u32x2 *)((const uint8_t *)mis + a);
        return HamBits2Word{v.x, v.y};
    };
    auto any = [](bool p) -> bool { return __ballot(p) != 0ull; };
    // the wavefront's staged records go out: ONE add to the counter for up to 64 records
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
            hsx2_str(P.hs, (uint32_t)hi, hay, h);
            live = (uint64_t)n <= h;
            if (live) hsx2_scan_pair<B>(hay, (uint32_t)h, lookup, n, P.kc, any, r);
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
