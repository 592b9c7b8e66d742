// lev_bits_tab.hip -- gfx950 instantiation of the table form of the bit-parallel band kernel (lev_bits_tab_body.h).
#include <hip/hip_runtime.h>

#include "lev_bits_tab_body.h"
#include "lev_plan.h"
#include "wave_tab.h"
#include "ta_internal.h"

namespace ta {

// One wavefront per block: the nibble tables sit at the start of the block's LDS, address 0 (the body's table addresses are absolute:
// lane * 4 | nibble << 8 as they stand) and are all of it, 8,192 bytes: the strings stay in registers.  The registers, capped for four
// wavefronts per SIMD (128; the kernel takes 121, no scratch), set the occupancy: 16 wavefronts per CU = 128 KB of the CU's 160 KB of LDS
// (the LDS would hold 20).  The body holds no slot-bit constants across the column loop (lev_bits_tab_body.h, flips()): parked, they were
// 32 registers more and the cap was three wavefronts per SIMD.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void lev_bits_tab_kernel(LevParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    if (DevTab::lds_address(lds, lds) != 0u) return;         // (never: this kernel has no static LDS in front of the dynamic one)
    LevBitsTab<DevWave, DevTab>::run(P, blockIdx.x, lds);
}

hipError_t lev_bits_tab_launch(const LevParams &P0, hipStream_t s, uint32_t *grid_out, uint32_t *lds_out) {
    LevParams P = P0;
    P.lds_per_wave = LEV_TAB_LDS_PER_WAVE;
    const uint32_t waves = (P.n + 63u) / 64u;
    const uint32_t grid = waves;
    // TA_TAB_LDS_PAD_KB (TA_TUNING only, the occupancy probe of profiles/r12): unused KB behind the tables, so that fewer wavefronts share
    // a CU -- 16 / 14 / 13 / 12 of them at 0 / 3 / 4 / 5.  The kernel never touches the pad
    const int pad_kb = env_int("TA_TAB_LDS_PAD_KB");
    const uint32_t lds = LEV_TAB_LDS_PER_WAVE + 1024u * (uint32_t)(pad_kb < 0 ? 0 : pad_kb > 56 ? 56 : pad_kb);
    if (grid_out) *grid_out = grid;
    if (lds_out) *lds_out = lds;
    // TA_TAB_DEPTH (TA_TUNING only): the depth that does not ship, from lev_bits_tab_alt.hip; any other value is the default's
    if (env_int("TA_TAB_DEPTH") == LEV_TAB_ALT_DEPTH) return lev_bits_tab_alt_launch(P, grid, lds, s);
    set_last_kernel_name("lev_bits_tab_kernel");
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(lev_bits_tab_kernel, dim3(grid), dim3(64), lds, s, P);
    return hipGetLastError();
}

}  // namespace ta
