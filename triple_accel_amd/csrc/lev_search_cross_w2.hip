// lev_search_cross_w2.hip -- gfx950 kernels of ta_levenshtein_search_cross_with_opts's two-word route: a panel whose longest needle is
// 33..64 bytes, every needle in every haystack.  The finish kernel is lev_search_cross.hip's.
//
// Scan: a workgroup of 512 threads builds ONE group's match table in LDS -- 256 rows of 32 columns of 2 words, 64 KB as the one-word
// table, so two workgroups share a CU's 160 KB: four wavefronts per SIMD -- and its eight wavefronts then walk the workgroup's
// haystacks, 64 / G >= 2 of them per wavefront and step.  Lane l reads column l mod 32 (needle l mod G of the group: the columns repeat
// the group's needles where G < 32), both words with ONE ds_read_b64 of dwords (c * 32 + l mod 32) * 2 + {0, 1}.  The bank argument:
// ds_read_b64 serves a 32-lane half per pass and banks dwords modulo 64; the lanes of a half read 32 different columns, so their 64
// dwords are banks 2 (l mod 32) + {0, 1} of ONE 256-byte row each -- every bank once, whatever the haystacks' bytes c are and however
// many slots (haystacks) a half holds.  Lanes l and l + 32 share a column but sit in different halves: they never meet.
// The build's stores (ds_write_b32 banks modulo 32: word w of columns j and j + 16 meet, 2-way) run once per workgroup.
// Exact: one lane per candidate (anchored: per (haystack, needle) of the sub-batch), the recurrence with its DP column in HBM scratch
// (lev_search_tile_mem, element-major over the resident lanes: a wavefront's accesses coalesce) over the span with the online Best
// fold; its epilogue is search_cross_dev.h's sx_exact_emit, shared with lev_search_cross.hip.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "lev_search_cross_w2_body.h"
#include "search_cross_dev.h"
#include "ta_internal.h"

namespace ta {

template <bool TRANS>
__global__ __launch_bounds__(512) void lev_search_cross_w2_scan_kernel(SearchCrossParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t peq[256 * SX2_GROUP * 2];
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    // (lane ownership, the walk and the append are written out here and not taken from search_cross_dev.h's sx_lane and sx_scan_walk:
    // with them this kernel alone measured 0.5 % and 1.5 % slower on the 12 x 34 and 96 x 40 panels -- profiles/r16)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t g0 = blockIdx.y * SX2_GROUP;
    const uint32_t size = sx_group_size(P.nn, blockIdx.y, SX2_GROUP), G = sx_group_cols(size), S = 64u / G;
    const uint32_t col = lane & (G - 1u), slot = lane / G, column = lane & (SX2_GROUP - 1u), half = lane >> 5;
    const bool has_needle = col < size;
    const uint32_t needle = g0 + col;
    const uint8_t *np = nullptr;
    uint32_t n = 0;
    if (has_needle) {
        uint64_t nl;
        dev_str(P.nd, needle, np, nl);
        n = nl < (uint64_t)SX2_MAX_NEEDLE ? (uint32_t)nl : SX2_MAX_NEEDLE;     // (max_len bounds every needle: no clamp in a valid call)
    }
    const bool scans = has_needle && sx_scans(n, P.kf);
    // the table: lanes l and l + 32 own one column (the same needle), word l / 32 of it each.  Wavefront w fills rows 32 w .. 32 w + 31
    // with the wildcard words, then (behind a barrier) the needles' own bits are added, needle byte j by half-wavefront j mod 16 -- two
    // bytes of one needle may name the same row: an LDS atomic
    const uint32_t wild = scans ? sx2_peq_wild(n, half) : 0u;
#pragma unroll 8
    for (uint32_t c = wave * 32u; c < wave * 32u + 32u; c++) peq[sx2_peq_at(c, column, half)] = wild;
    __syncthreads();
    if (scans)
        for (uint32_t j = wave * 2u + half; j < n; j += 2u * SX_WAVES) {
            uint32_t w;
            const uint32_t bit = sx2_peq_bit(n, j, w);
            atomicOr(&peq[sx2_peq_at((uint32_t)np[j], column, w)], bit);
        }
    __syncthreads();

    const uint64_t wg0 = (uint64_t)P.h0 + (uint64_t)blockIdx.x * P.hpw;          // the workgroup's haystacks: [wg0, wg1)
    const uint64_t wg1 = wg0 + P.hpw < P.h1 ? wg0 + P.hpw : P.h1;
    for (uint32_t it = 0;; it++) {
        if (wg0 + sx_local_hay(it, wave, S, 0) >= wg1) break;                    // (wavefront-uniform: the ballot below sees every lane)
        const uint64_t hi = wg0 + sx_local_hay(it, wave, S, slot);
        const bool valid = has_needle && hi < wg1;
        uint32_t first = 0, last = 0;
        if (valid) {
            const uint8_t *hay;
            uint64_t h;
            dev_str(P.hs, (uint32_t)hi, hay, h);
            sx2_scan_pair<TRANS>(hay, h, [&](uint32_t c, uint32_t (&Eq)[2]) {
                const u32x2 v = *(const u32x2 *)&peq[sx2_peq_at(c, column, 0)];
                Eq[0] = v.x; Eq[1] = v.y;
            }, n, P.kf, first, last);
        }
        const bool cand = valid && first != 0;
        const unsigned long long mask = __ballot(cand);
        if (mask) {
            const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
            uint32_t base = 0;
            if (lane == leader) base = atomicAdd(P.n_rec, (uint32_t)__popcll(mask));
            base = (uint32_t)__shfl((int)base, (int)leader);
            if (cand) P.rec[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = SxRec{(uint32_t)hi, needle, first, last, TA_NONE};
        }
    }
}

// a persistent grid of P.col_lanes lanes, one memory-backed column each; the lanes stride over the records in whole wavefronts
// (sx_exact_emit's appends are per wavefront).  TRANS: the costs have a transposition term (P.tc is its cost)
template <bool TRANS>
__global__ __launch_bounds__(256) void lev_search_cross_w2_exact_kernel(SearchCrossParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t per = (uint64_t)(P.h1 - P.h0) * P.nn;
    const uint64_t n_work = P.n_rec ? (uint64_t)*P.n_rec : per;
    const SearchCosts C{P.k, P.mc, P.gc, P.sg, P.tc, P.anchored};
    uint32_t *col = P.col + ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x);
    for (uint64_t w0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); w0 < n_work; w0 += lanes) {
        const uint64_t idx = w0 + lane;
        const bool live = idx < n_work;
        SxRec r = {0u, 0u, 1u, 0u, TA_NONE};
        uint32_t n_matches = 0;
        ta_match m = {0, 0, TA_NONE, 0u};
        if (live) {
            if (P.n_rec) r = P.rec[idx];
            else { r.hay = P.h0 + (uint32_t)(idx / P.nn); r.needle = (uint32_t)(idx % P.nn); }
            const uint8_t *np, *hay;
            uint64_t nl, h;
            dev_str(P.nd, r.needle, np, nl);
            dev_str(P.hs, r.hay, hay, h);
            const uint32_t n = nl < (uint64_t)SX2_MAX_NEEDLE ? (uint32_t)nl : SX2_MAX_NEEDLE;   // (the column has room for 64 rows)
            n_matches = sx2_exact_pair<TRANS>(hay, h, np, n, C, P.n_rec != nullptr, r.a, r.b, P.halo, col, lanes, m);
        }
        sx_exact_emit(P, idx, live, r, m, n_matches);
    }
}

hipError_t search_cross_w2_scan_launch(const SearchCrossParams &P, bool trans, hipStream_t st) {
    if (P.h1 <= P.h0 || P.nn == 0 || P.hpw == 0) return hipSuccess;
    const uint32_t groups = (P.nn + SX2_GROUP - 1) / SX2_GROUP;
    if (groups > 65535u) return hipErrorInvalidValue;
    const dim3 grid((P.h1 - P.h0 + P.hpw - 1) / P.hpw, groups);
    set_last_kernel_name("lev_search_cross_w2_scan_kernel<%s>", trans ? "true" : "false");
    if (trans) hipLaunchKernelGGL((lev_search_cross_w2_scan_kernel<true>), grid, dim3(512), 0, st, P);
    else hipLaunchKernelGGL((lev_search_cross_w2_scan_kernel<false>), grid, dim3(512), 0, st, P);
    return hipGetLastError();
}

hipError_t search_cross_w2_exact_launch(const SearchCrossParams &P, bool trans, hipStream_t st) {
    if (P.h1 <= P.h0 || P.nn == 0) return hipSuccess;
    if (P.max_needle > SX2_MAX_NEEDLE || !P.col || P.col_lanes == 0 || P.col_lanes % 256u) return hipErrorInvalidValue;
    set_last_kernel_name("lev_search_cross_w2_exact_kernel<%s>", trans ? "true" : "false");
    if (trans) hipLaunchKernelGGL((lev_search_cross_w2_exact_kernel<true>), dim3(P.col_lanes / 256u), dim3(256), 0, st, P);
    else hipLaunchKernelGGL((lev_search_cross_w2_exact_kernel<false>), dim3(P.col_lanes / 256u), dim3(256), 0, st, P);
    return hipGetLastError();
}

}  // namespace ta
