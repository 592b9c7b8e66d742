// ham_search_batch.hip -- gfx950 kernels of ta_hamming_search_batch: one lane per (needle, haystack) pair.
//
// General route: the SWAR window compare of ham_search_batch_body.h, the needle in registers up to 64 bytes (NW = 2 / 4 / 8 / 16 dwords),
// both sides from memory beyond.  Shared-needle route (1..32 bytes, 4 k <= n): bit-sliced mismatch counters, the needle's 256-entry Mis
// table built once per workgroup in LDS.  Every lane folds its own result (HamBatchSink) and writes its own count; the NUL scan of the
// SIMD contract rides on the haystack words the scan loads.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "dev_str.h"
#include "ham_search_batch_body.h"
#include "lds_tab64.h"
#include "ta_internal.h"

namespace ta {

template <int NW>
__global__ __launch_bounds__(256) void ham_search_batch_kernel(HamBatchParams P) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P.n) return;
    const uint32_t pair = P.list ? P.list[idx] : idx;
    const uint8_t *np, *hay;
    uint64_t nl, h;
    dev_str(P.nd, pair, np, nl);
    dev_str(P.hs, pair, hay, h);
    P.counts[pair] = ham_batch_pair_regs<NW>(np, nl, hay, h, P.k, P.best != 0, P.matches + (uint64_t)pair * P.cap, P.cap);
}

__global__ __launch_bounds__(256) void ham_search_batch_mem_kernel(HamBatchParams P) {
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P.n) return;
    const uint32_t pair = P.list ? P.list[idx] : idx;
    const uint8_t *np, *hay;
    uint64_t nl, h;
    dev_str(P.nd, pair, np, nl);
    dev_str(P.hs, pair, hay, h);
    P.counts[pair] = ham_batch_pair_mem(np, nl, hay, h, P.k, P.best != 0, P.matches + (uint64_t)pair * P.cap, P.cap);
}

// Shared needle: Mis[c] kept once per lane of a wavefront (lds_tab64.h) -- 64 KB, 512 threads, two workgroups per CU.
template <int B>
__global__ __launch_bounds__(512) void ham_search_batch_bits_kernel(HamBatchParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t mis[256 * 64];
    const uint8_t *needle = P.nd.blob;
    const uint32_t nlen = P.max_needle;
    tab64_fill(mis, ham_bits_mis(needle, nlen, threadIdx.x >> 1));
    __syncthreads();
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P.n) return;
    const uint32_t pair = P.list ? P.list[idx] : idx;
    const uint32_t lane_off = (threadIdx.x & 63u) * 4u;
    auto lookup = [&](uint32_t v, int b) -> uint32_t { return tab64_lookup(mis, lane_off, v, b); };
    const uint8_t *hay;
    uint64_t h;
    dev_str(P.hs, pair, hay, h);
    P.counts[pair] = ham_batch_pair_bits<B>(needle, nlen, hay, h, P.k, P.best != 0, lookup, P.matches + (uint64_t)pair * P.cap, P.cap);
}

hipError_t ham_search_batch_launch(const HamBatchParams &P, bool bits, hipStream_t st) {
    if (P.n == 0) return hipSuccess;
    if (bits) {
        const int planes = ham_bits_planes(P.k);
        const dim3 grid((P.n + 511) / 512), block(512);
        set_last_kernel_name("ham_search_batch_bits_kernel<%d>", planes);
        switch (planes) {
            case 1: hipLaunchKernelGGL(ham_search_batch_bits_kernel<1>, grid, block, 0, st, P); break;
            case 2: hipLaunchKernelGGL(ham_search_batch_bits_kernel<2>, grid, block, 0, st, P); break;
            case 3: hipLaunchKernelGGL(ham_search_batch_bits_kernel<3>, grid, block, 0, st, P); break;
            case 4: hipLaunchKernelGGL(ham_search_batch_bits_kernel<4>, grid, block, 0, st, P); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    const dim3 grid((P.n + 255) / 256), block(256);
    const uint32_t m = P.max_needle;
    if (m > 64) {
        set_last_kernel_name("ham_search_batch_mem_kernel");
        hipLaunchKernelGGL(ham_search_batch_mem_kernel, grid, block, 0, st, P);
        return hipGetLastError();
    }
    const int nw = m <= 8 ? 2 : m <= 16 ? 4 : m <= 32 ? 8 : 16;
    set_last_kernel_name("ham_search_batch_kernel<%d>", nw);
    switch (nw) {
        case 2: hipLaunchKernelGGL(ham_search_batch_kernel<2>, grid, block, 0, st, P); break;
        case 4: hipLaunchKernelGGL(ham_search_batch_kernel<4>, grid, block, 0, st, P); break;
        case 8: hipLaunchKernelGGL(ham_search_batch_kernel<8>, grid, block, 0, st, P); break;
        default: hipLaunchKernelGGL(ham_search_batch_kernel<16>, grid, block, 0, st, P); break;
    }
    return hipGetLastError();
}

}  // namespace ta
