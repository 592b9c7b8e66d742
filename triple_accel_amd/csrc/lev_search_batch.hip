// lev_search_batch.hip -- gfx950 kernels of ta_levenshtein_search_batch: one lane per (needle, haystack) pair.
//
// Route E: the exact recurrence (lev_search_body.h) from column 0 over the pair's whole haystack, hits folded on the fly
// (lev_search_batch_body.h).  Route S (a shared needle of up to 64 bytes): a bit-parallel unit-cost scan finds each pair's
// span of candidate ends and answers the pairs without one; the exact kernel then runs on the listed pairs' spans only.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "dev_str.h"
#include "lds_tab64.h"
#include "lev_search_batch_body.h"
#include "ta_internal.h"

namespace ta {

// the longest string of each CSR side (max[0] needles, max[1] haystacks; pre-zeroed): 64-bit, a haystack may pass 4 GiB
__global__ void search_batch_maxlen_kernel(StrView nd, StrView hs, uint32_t n, unsigned long long *max) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t *p;
    uint64_t ln = 0, lh = 0;
    if (nd.off) dev_str(nd, i, p, ln);
    if (hs.off) dev_str(hs, i, p, lh);
    if (ln) atomicMax(&max[0], (unsigned long long)ln);
    if (lh) atomicMax(&max[1], (unsigned long long)lh);
}

// Exact pass, needles of up to N <= 32 bytes held in registers (loaded once).  P.span == nullptr: Route E over the whole haystack
// (or its anchored prefix); else Route S over the pair's scanned span, the pairs of the candidate list.
template <int N, bool TRANS, bool PACKED>
__global__ __launch_bounds__(256) void lev_search_batch_kernel(SearchBatchParams P) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n_work = P.n_list ? *P.n_list : P.n;
    if (idx >= n_work) return;
    const uint32_t pair = P.list ? P.list[idx] : idx;
    const uint8_t *np, *hay;
    uint64_t nl, h;
    dev_str(P.nd, pair, np, nl);
    dev_str(P.hs, pair, hay, h);
    const SearchCosts C{P.k, P.mc, P.gc, P.sg, P.tc, P.anchored};
    SearchBatchSink sink;
    sink.init(P.matches + (uint64_t)pair * P.cap, P.cap, P.best != 0, P.k);
    const uint32_t n = nl < (uint64_t)N ? (uint32_t)nl : (uint32_t)N;      // (max_len bounds every needle: no clamp in a valid call)
    if (lev_search_batch_prologue(n, h, C, sink)) {
        uint8_t needle[N];
#pragma unroll
        for (int j = 0; j < N; j++) needle[j] = (uint32_t)j < n ? np[j] : (uint8_t)0;
        uint64_t cb = 0, eb = 0, ce = lev_search_batch_cols(n, h, C);
        if (P.span) lev_search_batch_span_cols(P.span[2 * (uint64_t)pair], P.span[2 * (uint64_t)pair + 1], P.halo, cb, eb, ce);
        lev_search_batch_exact<N, TRANS, PACKED>(hay, needle, n, C, cb, eb, ce, sink);
    }
    P.counts[pair] = sink.count;
}

// Exact pass, needles beyond 32 bytes: the DP column in HBM scratch, one column per resident lane (persistent grid, element-major
// so that a wavefront's accesses coalesce); lanes stride over the pairs (or the candidate list, P.span: Route S).
__global__ __launch_bounds__(256) void lev_search_batch_mem_kernel(SearchBatchParams P) {
    const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x, lanes = gridDim.x * blockDim.x;
    const uint32_t n_work = P.n_list ? *P.n_list : P.n;
    const SearchCosts C{P.k, P.mc, P.gc, P.sg, P.tc, P.anchored};
    for (uint32_t idx = lane; idx < n_work; idx += lanes) {
        const uint32_t pair = P.list ? P.list[idx] : idx;
        const uint8_t *np, *hay;
        uint64_t nl, h;
        dev_str(P.nd, pair, np, nl);
        dev_str(P.hs, pair, hay, h);
        SearchBatchSink sink;
        sink.init(P.matches + (uint64_t)pair * P.cap, P.cap, P.best != 0, P.k);
        const uint32_t n = nl < (uint64_t)P.max_needle ? (uint32_t)nl : P.max_needle;
        if (lev_search_batch_prologue(n, h, C, sink)) {
            uint64_t cb = 0, eb = 0, ce = lev_search_batch_cols(n, h, C);
            if (P.span) lev_search_batch_span_cols(P.span[2 * (uint64_t)pair], P.span[2 * (uint64_t)pair + 1], P.halo, cb, eb, ce);
            lev_search_tile_mem(hay, np, n, C, P.tc != 0, P.col + lane, lanes, cb, eb, ce,
                                [&sink](uint64_t end, uint32_t len, uint32_t cost) { sink.put(end - len, end, cost); });
        }
        P.counts[pair] = sink.count;
    }
}

// Route S scan: one lane per pair over its haystack.  The shared needle's match table is built once per workgroup in LDS; NWF = 1
// keeps it once per lane of a wavefront (lds_tab64.h: lane l reads dword l of row c, no two lanes of a 32-lane group share a bank
// whatever the bytes are), NWF = 2 keeps one [256][2] table.  Pairs with a candidate end get their span and a place in the list;
// the others are finished here: their result is the end == 0 match or nothing.
template <int NWF, bool TRANS>
__global__ __launch_bounds__(NWF == 1 ? 512 : 256) void lev_search_batch_scan_kernel(SearchBatchParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t peq[NWF == 1 ? 256 * 64 : 256 * 2];
    const uint8_t *needle = P.nd.blob;
    const uint32_t nlen = (uint32_t)P.nd.len;
    if (NWF == 1) {
        tab64_fill(peq, lev_filter_peq(needle, nlen, threadIdx.x >> 1));
    } else {
        peq[2 * threadIdx.x] = lev_filter_peq_word(needle, nlen, 2, threadIdx.x, 0);
        peq[2 * threadIdx.x + 1] = lev_filter_peq_word(needle, nlen, 2, threadIdx.x, 1);
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pair = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = pair < P.n;
    uint64_t first = 0, last = 0;
    if (valid) {
        const uint8_t *hay;
        uint64_t h;
        dev_str(P.hs, pair, hay, h);
        auto lookup = [&](uint32_t c, int w) -> uint32_t {
            if (NWF == 1) return peq[c * 64u + lane];
            return peq[2u * c + (uint32_t)w];
        };
        lev_search_batch_scan<NWF, TRANS>(hay, h, lookup, nlen, P.kf, first, last);
    }
    const bool cand = valid && first != 0;
    // the list: one atomic per wavefront, the lanes with a candidate take consecutive places
    const unsigned long long mask = __ballot(cand);
    if (mask) {
        const uint32_t leader = (uint32_t)__ffsll((long long)mask) - 1u;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(P.cand_count, (uint32_t)__popcll(mask));
        base = (uint32_t)__shfl((int)base, (int)leader);
        if (cand) P.cand_list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = pair;
    }
    if (cand) {
        P.span[2 * (uint64_t)pair] = (uint32_t)first;
        P.span[2 * (uint64_t)pair + 1] = (uint32_t)last;
    } else if (valid) {
        const uint32_t whole_gap = nlen * P.gc + P.sg;             // src/levenshtein.rs:1693-1706
        const bool end0 = whole_gap <= P.k;
        if (end0 && P.cap) P.matches[(uint64_t)pair * P.cap] = ta_match{0, 0, whole_gap, 0u};
        P.counts[pair] = end0 ? 1u : 0u;
    }
}

template <int N>
static void launch_n(const SearchBatchParams &P, bool trans, bool packed, uint32_t grid, hipStream_t s) {
    if (packed) {
        if (trans) hipLaunchKernelGGL((lev_search_batch_kernel<N, true, true>), dim3(grid), dim3(256), 0, s, P);
        else hipLaunchKernelGGL((lev_search_batch_kernel<N, false, true>), dim3(grid), dim3(256), 0, s, P);
    } else if constexpr (N % 8 == 0) {
        if (trans) hipLaunchKernelGGL((lev_search_batch_kernel<N, true, false>), dim3(grid), dim3(256), 0, s, P);
        else hipLaunchKernelGGL((lev_search_batch_kernel<N, false, false>), dim3(grid), dim3(256), 0, s, P);
    }
}

static void launch_exact(const SearchBatchParams &P, bool trans, bool packed, uint32_t grid, hipStream_t s) {
    const uint32_t n = P.max_needle;
    if (packed) {                            // one instantiation per needle length (packed form: N == the needle's length)
        switch (n) {
#define TA_N(x) case x: launch_n<x>(P, trans, true, grid, s); return;
            TA_N(1) TA_N(2) TA_N(3) TA_N(4) TA_N(5) TA_N(6) TA_N(7) TA_N(8) TA_N(9) TA_N(10) TA_N(11) TA_N(12)
            TA_N(13) TA_N(14) TA_N(15) TA_N(16) TA_N(17) TA_N(18) TA_N(19) TA_N(20) TA_N(21) TA_N(22) TA_N(23) TA_N(24)
            TA_N(25) TA_N(26) TA_N(27) TA_N(28) TA_N(29) TA_N(30) TA_N(31) TA_N(32)
#undef TA_N
        }
    }
    if (n <= 8) launch_n<8>(P, trans, false, grid, s);
    else if (n <= 16) launch_n<16>(P, trans, false, grid, s);
    else if (n <= 24) launch_n<24>(P, trans, false, grid, s);
    else launch_n<32>(P, trans, false, grid, s);
}

hipError_t search_batch_maxlen_launch(const StrView &nd, const StrView &hs, uint32_t n, unsigned long long *max, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(search_batch_maxlen_kernel, dim3((n + 255) / 256), dim3(256), 0, st, nd, hs, n, max);
    return hipGetLastError();
}

hipError_t search_batch_exact_launch(const SearchBatchParams &P, bool trans, bool packed, uint32_t mem_lanes, hipStream_t st) {
    if (P.n == 0) return hipSuccess;
    if (P.max_needle > 32) {
        set_last_kernel_name("lev_search_batch_mem_kernel");
        hipLaunchKernelGGL(lev_search_batch_mem_kernel, dim3((mem_lanes + 255) / 256), dim3(256), 0, st, P);
        return hipGetLastError();
    }
    const uint32_t m = P.max_needle, nr = packed ? m : m <= 8 ? 8u : m <= 16 ? 16u : m <= 24 ? 24u : 32u;
    set_last_kernel_name("lev_search_batch_kernel<%u, %s, %s>", nr, trans ? "true" : "false", packed ? "true" : "false");
    const uint32_t grid = (P.n + 255) / 256;
    launch_exact(P, trans, packed, grid, st);
    return hipGetLastError();
}

hipError_t search_batch_scan_launch(const SearchBatchParams &P, bool trans, hipStream_t st) {
    if (P.n == 0) return hipSuccess;
    if (P.nd.len <= 32) {
        const uint32_t grid = (P.n + 511) / 512;
        if (trans) hipLaunchKernelGGL((lev_search_batch_scan_kernel<1, true>), dim3(grid), dim3(512), 0, st, P);
        else hipLaunchKernelGGL((lev_search_batch_scan_kernel<1, false>), dim3(grid), dim3(512), 0, st, P);
    } else {
        const uint32_t grid = (P.n + 255) / 256;
        if (trans) hipLaunchKernelGGL((lev_search_batch_scan_kernel<2, true>), dim3(grid), dim3(256), 0, st, P);
        else hipLaunchKernelGGL((lev_search_batch_scan_kernel<2, false>), dim3(grid), dim3(256), 0, st, P);
    }
    return hipGetLastError();
}

}  // namespace ta
