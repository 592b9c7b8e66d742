// lev_bits_tab_alt.hip -- the table form of the band kernel (lev_bits_tab_body.h) at the depth that does NOT ship: the same body, the same
// tables, the same LDS request and launch shape as lev_bits_tab_kernel, with the other lead of the LDS stream over the recurrence
// (LEV_TAB_ALT_DEPTH = 3 - LEV_TAB_DEPTH).  Taken only under TA_TUNING with TA_TAB_DEPTH set to that depth (lev_bits_tab_launch): the A/B
// of the two depths in one binary.  A translation unit of its own, so that lev_bits_tab.hip holds exactly one kernel.
#include <hip/hip_runtime.h>

#include "lev_bits_tab_body.h"
#include "lev_plan.h"
#include "wave_tab.h"
#include "ta_internal.h"

namespace ta {

// (one wavefront per block, the tables at LDS address 0, capped for four wavefronts per SIMD: lev_bits_tab.hip)
template <int DEPTH>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void lev_tab_depth_kernel(LevParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    if (DevTab::lds_address(lds, lds) != 0u) return;         // (never: this kernel has no static LDS in front of the dynamic one)
    LevBitsTab<DevWave, DevTab, TabNoProbe, DEPTH>::run(P, blockIdx.x, lds);
}

hipError_t lev_bits_tab_alt_launch(const LevParams &P, uint32_t grid, uint32_t lds, hipStream_t s) {
    set_last_kernel_name(LEV_TAB_ALT_DEPTH == 2 ? "lev_tab_depth_kernel<2>" : "lev_tab_depth_kernel<1>");
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(lev_tab_depth_kernel<LEV_TAB_ALT_DEPTH>, dim3(grid), dim3(64), lds, s, P);
    return hipGetLastError();
}

}  // namespace ta
