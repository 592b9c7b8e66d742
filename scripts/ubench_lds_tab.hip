// Micro-benchmark: the LDS side of the table form's column alone (lev_bits_tab_body.h) -- per column two conflict-free [entry][lane] reads
// (TL and TH, bank = lane) and four read-modify-writes (ds_xor_b32, no return) on entries picked per lane at random, with next to no VALU
// work beside them (one v_xor per read keeps the results alive).  One wavefront per block; the block's LDS request sets how many
// wavefronts a CU holds: 8, 11, 12 and 16.  Reported: cycles per wave-column per CU = the LDS floor of the new column, to be set beside
// its VALU count x 4.1 cycles / 4 SIMDs.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 scripts/ubench_lds_tab.hip -o scripts/ubench_lds_tab
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#define COLS_PER_ITER 8
#define ITERS 512

typedef __attribute__((address_space(3))) unsigned lds_u32;

__global__ __launch_bounds__(64) void k_lds_tab(unsigned *out, unsigned seed) {
#if defined(__HIP_DEVICE_COMPILE__)      // (LDS pointers are 32 bits wide on the device alone: the host pass skips the body)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const unsigned lane = threadIdx.x;
    // the tables (8 KB at the start of the block's LDS) zeroed, then eight addresses per role with random entries: lane * 4 | entry << 8
    for (unsigned e = 0; e < 32; e++) *(unsigned *)(lds + lane * 4 + 256 * e) = 0;
    unsigned r = (blockIdx.x * 64 + lane) * 2654435761u + seed;
    unsigned A[8];
    for (int i = 0; i < 8; i++) { r ^= r << 13; r ^= r >> 17; r ^= r << 5; A[i] = (unsigned)(size_t)(lds_u32 *)lds + lane * 4 + ((r >> 7) & 15u) * 256u; }
    unsigned acc = 0;
    __syncthreads();
    for (int it = 0; it < ITERS; it++) {
#pragma unroll
        for (int c = 0; c < COLS_PER_ITER; c++) {
            const unsigned bit = 1u << ((it * COLS_PER_ITER + c) & 31);
            acc ^= *(lds_u32 *)(A[c & 7]) & *(lds_u32 *)(A[(c + 3) & 7] + 4096u);
            (void)__hip_atomic_fetch_xor((lds_u32 *)(A[(c + 1) & 7]), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            (void)__hip_atomic_fetch_xor((lds_u32 *)(A[(c + 2) & 7] + 4096u), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            (void)__hip_atomic_fetch_xor((lds_u32 *)(A[(c + 5) & 7]), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            (void)__hip_atomic_fetch_xor((lds_u32 *)(A[(c + 6) & 7] + 4096u), bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
    }
    out[blockIdx.x * 64 + lane] = acc;
#endif
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const double hz = prop.clockRate * 1e3;
    printf("%s: %d CUs, %.0f MHz; %d columns per wavefront, per column 2 ds_read_b32 + 4 ds_xor_b32\n", prop.gcnArchName, cus, hz / 1e6, ITERS * COLS_PER_ITER);
    const int waves_per_cu[4] = {8, 11, 12, 16};
    for (int w = 0; w < 4; w++) {
        const int wpc = waves_per_cu[w];
        const size_t lds = ((160u * 1024u) / wpc) & ~255u;          // the LDS request that lets exactly wpc blocks share a CU
        const int blocks = cus * wpc * 4;                            // four rounds of a full chip
        unsigned *out;
        CK(hipMalloc(&out, (size_t)blocks * 64 * 4));
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        hipLaunchKernelGGL(k_lds_tab, dim3(blocks), dim3(64), lds, 0, out, 1u);      // warm-up
        CK(hipDeviceSynchronize());
        float best = 1e30f;
        for (int rep = 0; rep < 5; rep++) {
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(k_lds_tab, dim3(blocks), dim3(64), lds, 0, out, 2u + rep);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (ms < best) best = ms;
        }
        const double wave_cols_per_cu = (double)blocks * ITERS * COLS_PER_ITER / cus;
        printf("%2d waves/CU (LDS %6zu B/block, %d blocks): %.4f ms -> %.2f cycles per wave-column per CU\n", wpc, lds, blocks, best,
               best * 1e-3 * hz / wave_cols_per_cu);
        CK(hipFree(out));
    }
    return 0;
}
