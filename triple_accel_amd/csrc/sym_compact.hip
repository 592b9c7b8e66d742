// sym_compact.hip -- the per-pair symbol compaction of token batches (sym_compact_body.h): one wavefront per pair, four per workgroup.
#include <hip/hip_runtime.h>

#include "sym_compact_body.h"
#include "ta_internal.h"

namespace ta {

__global__ __launch_bounds__(256) void sym_compact_kernel(SymCompactParams P) {
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = gridDim.x * 4u;
    SymCompact<DevWave>::run(P, wave, n_waves);
}

// waves: the wavefronts to launch (a multiple of 4 is used; long pairs' tables need P.table_cap entries for each of them)
hipError_t sym_compact_launch(const SymCompactParams &P, uint32_t waves, hipStream_t s) {
    const uint32_t blocks = (waves + 3u) / 4u;
    if (blocks == 0) return hipSuccess;
    set_last_kernel_name("sym_compact_kernel");
    hipLaunchKernelGGL(sym_compact_kernel, dim3(blocks), dim3(256), 0, s, P);
    return hipGetLastError();
}

}  // namespace ta
