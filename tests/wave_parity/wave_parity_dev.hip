// wave_parity_dev.hip -- WaveOps<DevWave> (wave_ops_body.h) as one gfx950 kernel: libta_wave_parity.so, TESTS ONLY.  Links nothing of the
// product; tests/test_gpu_wave_parity.py compares its output with the host emulation's (wave_parity_emu.cpp) bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_ops_body.h"

using namespace ta;

TA_WP_DEFINE_OP_NAMES()

// four wavefronts per block, every wavefront its own slice of the cases and of LDS
__global__ __launch_bounds__(256) void ta_wave_parity_kernel(const uint32_t *in, const uint32_t *hdr, uint32_t *out, uint32_t n_cases) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4][TA_WP_LDS_BYTES];
    const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t first = blockIdx.x * 4u + w, stride = gridDim.x * 4u;
    for (uint32_t c = first; c < n_cases; c += stride) WaveOps<DevWave>::run_case(in, hdr, out, n_cases, c, lds[w]);
}

// launches on `stream` and returns the launch's HIP error; does not synchronise
extern "C" int ta_wave_parity_run(const uint32_t *in_dev, const uint32_t *hdr_dev, uint32_t *out_dev, uint32_t n_cases, void *stream) {
    uint32_t blocks = (n_cases + 7u) / 8u;
    if (blocks < 2u) blocks = 2u;
    if (blocks > 256u) blocks = 256u;
    hipLaunchKernelGGL(ta_wave_parity_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, in_dev, hdr_dev, out_dev, n_cases);
    return (int)hipGetLastError();
}
