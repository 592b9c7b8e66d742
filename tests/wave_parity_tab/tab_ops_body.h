// tab_ops_body.h -- every operation of the table form's policy (triple_accel_amd/csrc/wave_tab.h), applied once per case and written out lane
// by lane.  TESTS ONLY.  Compiled twice: TabOps<DevWave, DevTab> in a gfx950 kernel (tab_parity_dev.hip) and TabOps<EmuWave, EmuTab> on the
// host (tab_parity_emu.cpp); tests/test_gpu_wave_parity_tab.py asserts that the two outputs are equal bit for bit.
//
//   in   n_cases blocks of 192 words: x, y, z for the 64 lanes (word (c * 3 + j) * 64 + lane)
//   out  TA_TP_N_OPS rows of n_cases * 64 words: out[(op * n_cases + c) * 64 + lane]
// Rows: nib_to_byte1<N>(lo, hi, x) with lo = z and hi = ~z: 0..3 the lo result for N = 0..3, 4..7 the hi result; 8 lds_address of the wavefront's LDS modulo its size (0);
// 9 the lane's dword x after lds_abs_xor32 with y, read back by lane + 7 through the plain path; 10 the same read by lane + 9 with
// lds_abs_read32; 11 two address updates back to back feeding an xor and a read, as the kernel body issues them.
#pragma once
#include <stdint.h>

#include "wave.h"

namespace ta {

#define TA_TP_N_OPS 12u
#define TA_TP_LDS_BYTES 8192u      // per wave: [entry 0..15][lane] dwords at 0, the same again at 4096 (the kernel's table layout)

template <class W, class T>
struct TabOps {
    using U32 = typename W::U32;
    using Bool = typename W::Bool;

    template <int N> static TA_HD inline void nib(const U32 &z, const U32 &x, U32 &lo, U32 &hi) { lo = z; hi = ~z; T::template nib_to_byte1<N>(lo, hi, x); }

    // all of case c; called by a whole wavefront; lds: this wave's TA_TP_LDS_BYTES
    static TA_HD inline void run_case(const uint32_t *in, uint32_t *out, uint32_t n_cases, uint32_t c, uint8_t *lds) {
        const U32 lane = W::lane();
        const Bool all = lane == lane;
        const uint32_t *cin = in + c * 192u;
        const U32 x = W::load_u32(cin, lane, all, 0u), y = W::load_u32(cin, lane + 64u, all, 0u), z = W::load_u32(cin, lane + 128u, all, 0u);
        const uint32_t labs = T::lds_address(lds, lds);
        U32 row[TA_TP_N_OPS];
        nib<0>(z, x, row[0], row[4]); nib<1>(z, x, row[1], row[5]); nib<2>(z, x, row[2], row[6]); nib<3>(z, x, row[3], row[7]);
        row[8] = W::splat(labs % TA_TP_LDS_BYTES);
        // every lane's own dword, XOR-ed by absolute address, read back by other lanes both ways
        W::lds_wave_sync();
        W::lds_write32(lds, lane << 2, x);
        W::lds_wave_sync();
        T::lds_abs_xor32(lds, W::splat(labs) + (lane << 2), y);
        W::lds_wave_sync();
        row[9] = W::lds_read32(lds, ((lane + 7u) & 63u) << 2);
        row[10] = T::lds_abs_read32(lds, W::splat(labs) + (((lane + 9u) & 63u) << 2));
        // as the body: the table zeroed in the lane's column, bit (c & 31) flipped in TL[lo(byte 2 of x)] and TH[hi(byte 2 of x)], then
        // looked up with byte 1 of y: the AND of the two entries
        W::lds_wave_sync();
#pragma unroll
        for (uint32_t e = 0; e < 32u; e++) W::lds_write32(lds, (lane << 2) + 256u * e, W::splat(0u));
        W::lds_wave_sync();
        U32 a_lo = lane << 2, a_hi = a_lo, l_lo = a_lo, l_hi = a_lo;       // (byte 1 of the register is the nibble's: the wavefront's base is added behind it)
        const U32 bit = W::splat(1u << (c & 31u));
        T::template nib_to_byte1<2>(a_lo, a_hi, x);
        T::lds_abs_xor32(lds, a_lo + labs, bit);
        T::lds_abs_xor32(lds, a_hi + (labs + 4096u), bit);
        T::template nib_to_byte1<1>(l_lo, l_hi, y);
        row[11] = T::lds_abs_read32(lds, l_lo + labs) & T::lds_abs_read32(lds, l_hi + (labs + 4096u));
        W::lds_wave_sync();
#pragma unroll
        for (uint32_t op = 0; op < TA_TP_N_OPS; op++) W::store_u32(out, lane + (op * n_cases + c) * 64u, row[op], all);
    }
};

}  // namespace ta
