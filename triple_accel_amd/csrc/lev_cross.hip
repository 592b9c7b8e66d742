// lev_cross.hip -- gfx950 kernel of ta_levenshtein_cross: every query against every target within k.
//
// One lane per target, 64 targets per wavefront, four wavefronts per workgroup; a wavefront walks a tile of P.qtile queries with
// lev_cross_body.h (the query's match vectors as a table in the wavefront's own 1 / 2 KB of LDS, the column in the lane's registers).
// What it does with the 64 answers of a query -- the count, the records, nearest, the per-query count, TA_CROSS_UPPER -- is
// lev_cross_walk.h's, shared with lev_cross_win.hip.  Nothing of size nq x nt exists anywhere.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "lev_cross_body.h"
#include "lev_cross_walk.h"
#include "ta_internal.h"

namespace ta {

// OPTS = false is ta_levenshtein_cross's kernel; a call with TA_CROSS_UPPER or per-query counts takes the other instantiation
template <int NW, bool TRANS, bool OPTS = false>
__global__ __launch_bounds__(256) void lev_cross_kernel(CrossParams P) {
    using B = LevCross<DevWave, NW, TRANS>;
    __shared__ __attribute__((aligned(16))) uint8_t tables[4u * B::LDS_BYTES];
    lev_cross_walk<B, OPTS>(P, tables);
}

template <int NW, bool OPTS>
static void cross_launch(const CrossParams &P, bool trans, dim3 grid, dim3 block, hipStream_t st) {
    if (trans) hipLaunchKernelGGL((lev_cross_kernel<NW, true, OPTS>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((lev_cross_kernel<NW, false, OPTS>), grid, block, 0, st, P);
}

hipError_t lev_cross_launch(const CrossParams &P, int nw, bool trans, hipStream_t st) {
    if (P.nq == 0 || P.nt == 0) return hipSuccess;
    if (P.qtile == 0 || (nw != 1 && nw != 2)) return hipErrorInvalidValue;
    const uint32_t tgroups = (uint32_t)(((uint64_t)P.nt + 63u) / 64u);
    const uint64_t qtiles = ((uint64_t)P.nq + P.qtile - 1u) / P.qtile;
    if (qtiles > 65535u) return hipErrorInvalidValue;
    const dim3 grid((tgroups + 3u) / 4u, (uint32_t)qtiles), block(256);
    set_last_kernel_name("lev_cross_kernel<%d, %s>", nw, trans ? "true" : "false");
    const bool opts = P.flags != 0 || P.per_query != nullptr;
    if (nw == 1) {
        if (opts) cross_launch<1, true>(P, trans, grid, block, st);
        else cross_launch<1, false>(P, trans, grid, block, st);
    } else {
        if (opts) cross_launch<2, true>(P, trans, grid, block, st);
        else cross_launch<2, false>(P, trans, grid, block, st);
    }
    return hipGetLastError();
}

}  // namespace ta
