// tab_parity_dev.hip -- TabOps<DevWave, DevTab> (tab_ops_body.h) as one gfx950 kernel: libta_tab_parity.so, TESTS ONLY.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tab_ops_body.h"
#include "wave_tab.h"

using namespace ta;

// two wavefronts per block, each with its own slice of the cases and of LDS: the second one's LDS does not start at address 0
__global__ __launch_bounds__(128) void ta_tab_parity_kernel(const uint32_t *in, uint32_t *out, uint32_t n_cases) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][TA_TP_LDS_BYTES];
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t c = blockIdx.x * 2u + w; c < n_cases; c += gridDim.x * 2u) TabOps<DevWave, DevTab>::run_case(in, out, n_cases, c, lds[w]);
}

// launches on `stream` and returns the launch's HIP error; does not synchronise
extern "C" int ta_tab_parity_run(const uint32_t *in_dev, uint32_t *out_dev, uint32_t n_cases, void *stream) {
    uint32_t blocks = (n_cases + 3u) / 4u;
    if (blocks < 2u) blocks = 2u;
    hipLaunchKernelGGL(ta_tab_parity_kernel, dim3(blocks), dim3(128), 0, (hipStream_t)stream, in_dev, out_dev, n_cases);
    return (int)hipGetLastError();
}
extern "C" int ta_tab_parity_n_ops(void) { return (int)TA_TP_N_OPS; }
