// lev_search_cross.hip -- gfx950 kernels of ta_levenshtein_search_cross: every needle of a panel in every haystack.
//
// Scan: a workgroup of 512 threads builds ONE group's match table peq[256][64] in LDS -- column l the rows of needle l mod G of the
// group -- and its eight wavefronts then walk the workgroup's haystacks, 64 / G of them per wavefront and step: every lane of a slot
// reads the same haystack bytes and looks its own column up (peq[c * 64 + lane]: no two lanes of a 32-lane half share a bank whatever
// the bytes are).  Pairs with a candidate end go to the candidate list, one atomic per wavefront and step.
// Exact: one lane per candidate (anchored: per (haystack, needle) of the sub-batch), lev_search_batch_body.h's recurrence over the span
// with the online Best fold; a hit is counted, appended, folded into its haystack's nearest word and count, and kept in its record.
// Finish: the record that carries its haystack's nearest word writes best[i].
// Lane ownership, the walk, the candidate append and the exact kernel's epilogue are search_cross_dev.h's (the epilogue shared with
// lev_search_cross_w2.hip, the rest with the Hamming panel kernels).
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "lev_search_cross_body.h"
#include "search_cross_dev.h"
#include "ta_internal.h"

namespace ta {

__global__ void search_cross_init_best_kernel(ta_match *best, uint32_t nh) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nh) best[i] = ta_match{0, 0, TA_NONE, 0u};
}

template <bool TRANS>
__global__ __launch_bounds__(512) void lev_search_cross_scan_kernel(SearchCrossParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t peq[256 * SX_GROUP];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const SxLane L = sx_lane(P.nd, P.nn, blockIdx.y, SX_GROUP, SX_MAX_NEEDLE);
    const uint32_t n = L.n;
    const bool scans = L.has_needle && sx_scans(n, P.kf);
    // the table: wavefront w fills rows 32 w .. 32 w + 31 of its lanes' columns with the wildcard word, then (behind a barrier) adds the
    // needles' own bits, needle byte j by wavefront j mod 8 -- two bytes of one needle may name the same row: an LDS atomic
    const uint32_t wild = scans ? sx_peq_wild(n) : 0u;
#pragma unroll 8
    for (uint32_t c = wave * 32u; c < wave * 32u + 32u; c++) peq[c * SX_GROUP + lane] = wild;
    __syncthreads();
    if (scans)
        for (uint32_t j = wave; j < n; j += SX_WAVES) atomicOr(&peq[(uint32_t)L.np[j] * SX_GROUP + lane], sx_peq_bit(n, j));
    __syncthreads();

    auto lookup = [&](uint32_t c) -> uint32_t { return peq[c * SX_GROUP + lane]; };
    sx_scan_walk(P, L, [&](const uint8_t *hay, uint64_t h, uint32_t &first, uint32_t &last) {
        sx_scan_pair<TRANS>(hay, h, lookup, n, P.kf, first, last);
    });
}

// lanes stride over the records in whole wavefronts (sx_exact_emit's appends are per wavefront)
template <int N, bool TRANS, bool PACKED>
__global__ __launch_bounds__(256) void lev_search_cross_exact_kernel(SearchCrossParams P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t per = (uint64_t)(P.h1 - P.h0) * P.nn;
    const uint64_t n_work = P.n_rec ? (uint64_t)*P.n_rec : per;
    const SearchCosts C{P.k, P.mc, P.gc, P.sg, P.tc, P.anchored};
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
            const uint32_t n = nl < (uint64_t)N ? (uint32_t)nl : (uint32_t)N;  // (max_len bounds every needle: no clamp in a valid call)
            n_matches = sx_exact_pair<N, TRANS, PACKED>(hay, h, np, n, C, P.n_rec != nullptr, r.a, r.b, P.halo, m);
        }
        sx_exact_emit(P, idx, live, r, m, n_matches);
    }
}

__global__ __launch_bounds__(256) void lev_search_cross_finish_kernel(SearchCrossParams P) {
    const uint64_t lanes = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n_work = P.n_rec ? (uint64_t)*P.n_rec : (uint64_t)(P.h1 - P.h0) * P.nn;
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n_work; idx += lanes) {
        const SxRec r = P.rec[idx];
        if (r.k != TA_NONE && sx_wins(r, P.nearest[r.hay])) P.best[r.hay] = ta_match{r.a, r.b, r.k, 0u};
    }
}

template <int N>
static void launch_n(const SearchCrossParams &P, bool trans, bool packed, uint32_t grid, hipStream_t s) {
    if (packed) {
        if (trans) hipLaunchKernelGGL((lev_search_cross_exact_kernel<N, true, true>), dim3(grid), dim3(256), 0, s, P);
        else hipLaunchKernelGGL((lev_search_cross_exact_kernel<N, false, true>), dim3(grid), dim3(256), 0, s, P);
    } else if constexpr (N % 8 == 0) {
        if (trans) hipLaunchKernelGGL((lev_search_cross_exact_kernel<N, true, false>), dim3(grid), dim3(256), 0, s, P);
        else hipLaunchKernelGGL((lev_search_cross_exact_kernel<N, false, false>), dim3(grid), dim3(256), 0, s, P);
    }
}

// the grid of a pass over up to `work` records: one lane each, at most 8,192 workgroups (the lanes stride beyond)
static uint32_t work_grid(uint64_t work) {
    const uint64_t g = (work + 255) / 256;
    return (uint32_t)(g < 8192 ? (g ? g : 1) : 8192);
}

hipError_t search_cross_init_best_launch(ta_match *best, uint32_t nh, hipStream_t st) {
    if (nh == 0) return hipSuccess;
    hipLaunchKernelGGL(search_cross_init_best_kernel, dim3((nh + 255u) / 256u), dim3(256), 0, st, best, nh);
    return hipGetLastError();
}

hipError_t search_cross_scan_launch(const SearchCrossParams &P, bool trans, hipStream_t st) {
    if (P.h1 <= P.h0 || P.nn == 0 || P.hpw == 0) return hipSuccess;
    const uint32_t groups = (P.nn + SX_GROUP - 1) / SX_GROUP;
    if (groups > 65535u) return hipErrorInvalidValue;
    const dim3 grid((P.h1 - P.h0 + P.hpw - 1) / P.hpw, groups);
    set_last_kernel_name("lev_search_cross_scan_kernel<%s>", trans ? "true" : "false");
    if (trans) hipLaunchKernelGGL((lev_search_cross_scan_kernel<true>), grid, dim3(512), 0, st, P);
    else hipLaunchKernelGGL((lev_search_cross_scan_kernel<false>), grid, dim3(512), 0, st, P);
    return hipGetLastError();
}

hipError_t search_cross_exact_launch(const SearchCrossParams &P, bool trans, bool packed, hipStream_t st) {
    if (P.h1 <= P.h0 || P.nn == 0) return hipSuccess;
    const uint32_t n = P.max_needle;
    if (n > SX_MAX_NEEDLE) return hipErrorInvalidValue;
    const uint32_t grid = work_grid((uint64_t)(P.h1 - P.h0) * P.nn);
    const uint32_t nr = packed ? n : n <= 8 ? 8u : n <= 16 ? 16u : n <= 24 ? 24u : 32u;
    set_last_kernel_name("lev_search_cross_exact_kernel<%u, %s, %s>", nr, trans ? "true" : "false", packed ? "true" : "false");
    if (packed) {                            // one instantiation per needle length (packed form: N == the needle's length)
        switch (n) {
#define TA_N(x) case x: launch_n<x>(P, trans, true, grid, st); return hipGetLastError();
            TA_N(1) TA_N(2) TA_N(3) TA_N(4) TA_N(5) TA_N(6) TA_N(7) TA_N(8) TA_N(9) TA_N(10) TA_N(11) TA_N(12)
            TA_N(13) TA_N(14) TA_N(15) TA_N(16) TA_N(17) TA_N(18) TA_N(19) TA_N(20) TA_N(21) TA_N(22) TA_N(23) TA_N(24)
            TA_N(25) TA_N(26) TA_N(27) TA_N(28) TA_N(29) TA_N(30) TA_N(31) TA_N(32)
#undef TA_N
        }
    }
    if (n <= 8) launch_n<8>(P, trans, false, grid, st);
    else if (n <= 16) launch_n<16>(P, trans, false, grid, st);
    else if (n <= 24) launch_n<24>(P, trans, false, grid, st);
    else launch_n<32>(P, trans, false, grid, st);
    return hipGetLastError();
}

hipError_t search_cross_finish_launch(const SearchCrossParams &P, hipStream_t st) {
    if (P.h1 <= P.h0 || P.nn == 0 || !P.best || !P.nearest) return hipSuccess;
    hipLaunchKernelGGL(lev_search_cross_finish_kernel, dim3(work_grid((uint64_t)(P.h1 - P.h0) * P.nn)), dim3(256), 0, st, P);
    return hipGetLastError();
}

}  // namespace ta
