// lev_cross_win.hip -- gfx950 kernel of ta_levenshtein_cross_with_opts for queries of 65 .. 256 bytes.
//
// lev_cross.hip's shape: one lane per target, 64 targets per wavefront, four wavefronts per workgroup, a wavefront walks a tile of
// P.qtile queries (lev_cross_walk.h).  The query step is lev_cross_win_body.h: the query's match vectors as a table in the wavefront's
// own 9 KB of LDS (36 KB per workgroup), and of the column only a window of WW 32-row blocks in the lane's registers, WW = 2, 3 or 4 by
// the threshold, or the whole column (WW = 8).
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "lev_cross_walk.h"
#include "lev_cross_win_body.h"
#include "ta_internal.h"

namespace ta {

template <int WW, bool TRANS>
__global__ __launch_bounds__(256) void lev_cross_win_kernel(CrossParams P) {
    using B = LevCrossWin<DevWave, WW, TRANS>;
    __shared__ __attribute__((aligned(16))) uint8_t tables[4u * B::LDS_BYTES];
    lev_cross_walk<B, true>(P, tables);
}

template <int WW>
static void win_launch(const CrossParams &P, bool trans, dim3 grid, dim3 block, hipStream_t st) {
    if (trans) hipLaunchKernelGGL((lev_cross_win_kernel<WW, true>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((lev_cross_win_kernel<WW, false>), grid, block, 0, st, P);
}

hipError_t lev_cross_win_launch(const CrossParams &P, int ww, bool trans, hipStream_t st) {
    if (P.nq == 0 || P.nt == 0) return hipSuccess;
    if (P.qtile == 0 || ww < win_ww(P.k) || (ww != 2 && ww != 3 && ww != 4 && ww != (int)WIN_NB)) return hipErrorInvalidValue;
    const uint32_t tgroups = (uint32_t)(((uint64_t)P.nt + 63u) / 64u);
    const uint64_t qtiles = ((uint64_t)P.nq + P.qtile - 1u) / P.qtile;
    if (qtiles > 65535u) return hipErrorInvalidValue;
    const dim3 grid((tgroups + 3u) / 4u, (uint32_t)qtiles), block(256);
    set_last_kernel_name("lev_cross_win_kernel<%d, %s>", ww, trans ? "true" : "false");
    if (ww == 2) win_launch<2>(P, trans, grid, block, st);
    else if (ww == 3) win_launch<3>(P, trans, grid, block, st);
    else if (ww == 4) win_launch<4>(P, trans, grid, block, st);
    else win_launch<(int)WIN_NB>(P, trans, grid, block, st);
    return hipGetLastError();
}

}  // namespace ta
