// lds_tab64.h -- a 256-entry byte table kept once per lane of a wavefront in LDS (device only).
//
// Row c (256 bytes) holds entry c once per lane, lane l reads its own copy: the 64 lookups of a wavefront fall on 64 different addresses
// of which no two in a 32-lane group share a bank, whatever the bytes are.  One flat 256-entry table indexed by a random byte per lane
// costs ~4.3 extra LDS cycles per lookup (SQ_LDS_BANK_CONFLICT 72.6 M per GiB, profiles/r02).  The address is built by ONE v_perm_b32
// per byte -- [lane_off | c << 8] -- where the flat table needs one SDWA shift: the VALU count is unchanged.
#pragma once
#include <stdint.h>

namespace ta {

// 512 threads build the 64 KB table of dword entries, two per row, half a row each; `word` = the entry of row threadIdx.x >> 1.
// The caller synchronises.
static __device__ __forceinline__ void tab64_fill(uint32_t *tab, uint32_t word) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 *row = (u32x4 *)(tab + (threadIdx.x >> 1) * 64 + (threadIdx.x & 1u) * 32);
#pragma unroll
    for (int q = 0; q < 8; q++) row[q] = u32x4{word, word, word, word};
}

// this lane's copy of the entry of byte b (0..3) of dword v; lane_off = the lane's byte offset inside a row (below 256).
// (T of two dwords: rows of 32 columns, one ds_read_b64 -- ham_search_cross_w2.hip, which has the bank argument for that shape.)
template <class T = uint32_t>
static __device__ __forceinline__ T tab64_lookup(const void *tab, uint32_t lane_off, uint32_t v, int b) {
    const uint32_t a = __builtin_amdgcn_perm(v, lane_off, 0x0C0C0000u | ((4u + (uint32_t)b) << 8));   // lane_off | byte b << 8
    return *(const T *)((const uint8_t *)tab + a);
}

}  // namespace ta
