// search_cross_dev.h -- what the panel search kernels share (lev_search_cross.hip, lev_search_cross_w2.hip, ham_search_cross.hip,
// ham_search_cross_w2.hip): which needle and haystack slot a lane owns, the walk of a workgroup over
// its haystacks, and what happens to a pair's result -- the Levenshtein scan's candidate append, the Levenshtein exact kernels' hit
// epilogue, the Hamming kernels' staged append.  A kernel builds its table in LDS, defines the lookup and makes one call.
// (lev_search_cross_w2_scan_kernel keeps its own copy of the ownership, walk and append: it measured slower with these.)
// Device-only: wavefront ballots and atomics.  The per-lane rules stay in the body headers, which the host emulations compile
// (tests/emu_search_cross*, tests/emu_hsearch_cross*: their own re-statements of these loops, on purpose).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_str.h"
#include "ham_search_cross_body.h"
#include "ta_internal.h"

namespace ta {

// ---- lane ownership.  Of a group of `size` needles in G columns (sx_group_size, sx_group_cols) lane l owns column l mod G and haystack
// slot l / G of the S = 64 / G its wavefront takes per step; a column without a needle (has_needle false: n = 0, np = nullptr) idles.
struct SxLane {
    uint32_t col, slot, S;
    uint32_t needle;               // the column's needle of the panel
    const uint8_t *np;
    uint32_t n;                    // its length, clamped
    bool has_needle;
};

// group: the workgroup's (blockIdx.y) of group_size needles each.  clamp: max_len bounds every needle, so a valid call never clamps -- the
// Levenshtein scans pass their longest needle, the Hamming kernels one more: a length their per-needle rule turns away.
__device__ __forceinline__ SxLane sx_lane(const StrView &nd, uint32_t nn, uint32_t group, uint32_t group_size, uint32_t clamp) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t size = sx_group_size(nn, group, group_size), G = sx_group_cols(size);
    SxLane L;
    L.S = 64u / G;
    L.col = lane & (G - 1u);
    L.slot = lane / G;
    L.has_needle = L.col < size;
    L.needle = group * group_size + L.col;
    L.np = nullptr;
    L.n = 0;
    if (L.has_needle) {
        uint64_t nl;
        dev_str(nd, L.needle, L.np, nl);
        L.n = nl < (uint64_t)clamp ? (uint32_t)nl : clamp;
    }
    return L;
}

// ---- the walk.  Workgroup blockIdx.x takes the haystacks [wg0, wg1): hpw of [h0, h1); each of its eight wavefronts takes S of them per
// step (sx_local_hay).  step(hi, inside): the lane's haystack of this step, and whether it is one of the workgroup's.
template <class Step>
__device__ __forceinline__ void sx_walk(uint32_t h0, uint32_t h1, uint32_t hpw, uint32_t S, uint32_t slot, Step step) {
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t wg0 = (uint64_t)h0 + (uint64_t)blockIdx.x * hpw;
    const uint64_t wg1 = wg0 + hpw < h1 ? wg0 + hpw : h1;
    for (uint32_t it = 0;; it++) {
        if (wg0 + sx_local_hay(it, wave, S, 0) >= wg1) break;                    // (wavefront-uniform: the ballots in step see every lane)
        const uint64_t hi = wg0 + sx_local_hay(it, wave, S, slot);
        step(hi, hi < wg1);
    }
}

// ---- the Levenshtein scan: pair(hay, h, first, last) scans one haystack against the lane's needle; a pair with a candidate end
// (first != 0) goes to the candidate list, one atomic per wavefront and step.
template <class Pair>
__device__ __forceinline__ void sx_scan_walk(const SearchCrossParams &P, const SxLane &L, Pair pair) {
    const uint32_t lane = threadIdx.x & 63u;
    sx_walk(P.h0, P.h1, P.hpw, L.S, L.slot, [&](uint64_t hi, bool inside) {
        const bool valid = L.has_needle && inside;
        uint32_t first = 0, last = 0;
        if (valid) {
            const uint8_t *hay;
            uint64_t h;
            dev_str(P.hs, (uint32_t)hi, hay, h);
            pair(hay, h, first, last);
        }
        const bool cand = valid && first != 0;
        const unsigned long long mask = __ballot(cand);
        if (mask) {
            const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(P.n_rec, (uint32_t)__popcll(mask));
            base = (uint32_t)__shfl((int)base, (int)leader);
            if (cand) P.rec[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = SxRec{(uint32_t)hi, L.needle, first, last, TA_NONE};
        }
    });
}

// ---- the Levenshtein exact kernels' epilogue, every lane of the wavefront: a live lane's record takes its result in place (R[0] = m,
// k = TA_NONE without one); a hit (n_matches != 0) is counted and appended, one atomic per wavefront, and folded into its haystack's
// nearest word and count.
__device__ __forceinline__ void sx_exact_emit(const SearchCrossParams &P, uint64_t idx, bool live, const SxRec &r, const ta_match &m,
                                              uint32_t n_matches) {
    const uint32_t lane = threadIdx.x & 63u;
    const bool hit = n_matches != 0;
    if (live) P.rec[idx] = SxRec{r.hay, r.needle, (uint32_t)m.start, (uint32_t)m.end, hit ? m.k : TA_NONE};
    const unsigned long long mask = __ballot(hit);
    if (!mask) return;
    const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(P.count, (unsigned long long)__popcll(mask));
    base = ((unsigned long long)__builtin_amdgcn_readlane((uint32_t)(base >> 32), leader) << 32) |
           __builtin_amdgcn_readlane((uint32_t)base, leader);
    const unsigned long long at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (hit) {
        if (at < P.cap) P.hits[at] = ta_search_cross_hit{r.hay, r.needle, (uint32_t)m.start, (uint32_t)m.end, m.k, n_matches};
        if (P.nearest) atomicMin(P.nearest + r.hay, (unsigned long long)sx_word(m.k, r.needle));
        if (P.per_haystack) atomicAdd(P.per_haystack + r.hay, 1u);
    }
}

// ---- the Hamming kernels: pair(hay, h, any, r) scans one haystack the lane's needle fits in (scans: the lane has a needle its kernel
// takes; any(p): p holds on some lane of the wavefront).  At the end of a haystack a lane with a hit puts its record into its wavefront's
// stage in LDS (HSX_STAGE records), bumps the haystack's count and folds its packed word into the haystack's minimum; a haystack with a
// 0x00 byte gets the NUL mark instead.
template <class Pair>
__device__ __forceinline__ void hsx_walk_emit(const HamSearchCrossParams &P, const SxLane &L, bool scans, ta_search_cross_hit *stage,
                                              Pair pair) {
    const uint32_t lane = threadIdx.x & 63u;
    auto any = [](bool p) -> bool { return __ballot(p) != 0ull; };
    // the wavefront's staged records go out: ONE add to the counter for up to 64 records (one add per wavefront and step made a million
    // returning atomics on one address of a million haystacks with a hit each: they serialise at the memory side)
    auto flush = [&](uint32_t cnt) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(P.count, (unsigned long long)cnt);
        base = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(base >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)base);
        if (lane < cnt && base + lane < P.cap) P.hits[base + lane] = stage[lane];
        __builtin_amdgcn_wave_barrier();
    };
    uint32_t staged = 0;                                                          // records in the wavefront's stage (wavefront-uniform)
    sx_walk(0u, P.nh, P.hpw, L.S, L.slot, [&](uint64_t hi, bool inside) {
        HsxBest r = {TA_NONE, 0u, 0u, false};
        bool live = false;                                                       // 1 <= n <= h: the pairs the reference looks at
        if (scans && inside) {
            const uint8_t *hay;
            uint64_t h;
            dev_str(P.hs, (uint32_t)hi, hay, h);
            live = (uint64_t)L.n <= h;
            if (live) pair(hay, (uint32_t)h, any, r);
        }
        const bool hit = live && !r.nul && r.count != 0u;
        if (live && r.nul && P.per_haystack) P.per_haystack[hi] = TA_NONE;       // (every lane of the haystack stores the same word)
        const unsigned long long mask = __ballot(hit);
        if (!mask) return;
        const uint32_t hits_now = (uint32_t)__popcll(mask);
        if (staged + hits_now > HSX_STAGE) { flush(staged); staged = 0; }          // (wavefront-uniform)
        if (hit) {
            stage[staged + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] =
                ta_search_cross_hit{(uint32_t)hi, L.needle, r.start, r.start + L.n, r.d, r.count};
            if (P.per_haystack) atomicAdd(P.per_haystack + hi, 1u);
            if (P.packed) atomicMin(P.packed + hi, (unsigned long long)hsx_word(r.d, L.needle, r.start));
        }
        staged += hits_now;
    });
    if (staged) flush(staged);
}

}  // namespace ta
