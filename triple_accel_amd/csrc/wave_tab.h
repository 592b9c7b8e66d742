// wave_tab.h -- the table form's own operations (lev_bits_tab_body.h), a second policy T beside the wave policy W of wave.h: DevTab maps each
// to one gfx950 instruction, EmuTab (tests/emu_tab/emu_tab_ops.h, host only, TESTS ONLY) is its 64-lane twin.  Device and emulation are
// compared bit for bit by tests/wave_parity_tab/.
#pragma once
#include <stdint.h>

#include "wave.h"

namespace ta {

#if defined(__HIPCC__)

struct DevTab {
    using U32 = uint32_t;
    // LDS addresses of the nibble tables: byte 1 of addr_lo <- the low nibble of byte N of x, byte 1 of addr_hi <- its high nibble, the
    // other three bytes of both stay -> TWO SDWA instructions (v_and_b32 / v_lshrrev_b32 on the selected byte, written to byte 1 with the
    // rest of the destination preserved).  hipcc's own sequence is v_bfe_u32 + v_lshl_or_b32 and a copy of the base, per address.
    // On gfx940 and later a VALU instruction that reads a register in the slot right behind a sub-dword write to it needs one wait state,
    // Both writes are ONE statement: the second instruction (which reads neither result) is the first one's wait state.  The second
    // one's is the compiler's to keep: hipcc takes every VGPR an asm statement writes for such a write and puts an s_nop in front of a VALU
    // instruction or another statement that reads it in the next slot (it did so in every such place while the body was being ordered).
    // The body has no such reader: an address goes to LDS instructions, which are not VALU instructions, and to the next statement on the
    // same register a column later.  A statement used to end in an s_nop 0 of its own -- three issue slots per column, 0.6 % of cfg2
    // (profiles/r13) -- and tests/test_lev_bits_tab_waits_cpu.py now reads the kernels' assembly for a VALU reader in the slot behind.
    // The two registers must be different ones.
    // VOLATILE: the statements keep their order among themselves and against W::opaque, which is how the body places a column's addresses
    // in front of its wait (lev_bits_tab_body.h, column()).
    template <int N>
    static __device__ __forceinline__ void nib_to_byte1(U32 &addr_lo, U32 &addr_hi, U32 x) {
        static_assert(N >= 0 && N < 4, "byte index");
        if constexpr (N == 0) asm volatile("v_and_b32_sdwa %0, 15, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:BYTE_0\n\t"
                                  "v_lshrrev_b32_sdwa %1, 4, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:BYTE_0" : "+v"(addr_lo), "+v"(addr_hi) : "v"(x));
        if constexpr (N == 1) asm volatile("v_and_b32_sdwa %0, 15, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:BYTE_1\n\t"
                                  "v_lshrrev_b32_sdwa %1, 4, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:BYTE_1" : "+v"(addr_lo), "+v"(addr_hi) : "v"(x));
        if constexpr (N == 2) asm volatile("v_and_b32_sdwa %0, 15, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:BYTE_2\n\t"
                                  "v_lshrrev_b32_sdwa %1, 4, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:BYTE_2" : "+v"(addr_lo), "+v"(addr_hi) : "v"(x));
        if constexpr (N == 3) asm volatile("v_and_b32_sdwa %0, 15, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:BYTE_3\n\t"
                                  "v_lshrrev_b32_sdwa %1, 4, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:BYTE_3" : "+v"(addr_lo), "+v"(addr_hi) : "v"(x));
    }
    // LDS by ABSOLUTE address (one wavefront per block and no static LDS, so the block's LDS starts at address 0 and `addr` is the
    // instruction's address operand as it stands -- through `lds + off` hipcc adds the base, a link-time zero, with a VALU instruction per
    // access).  lds0 = the start of the block's LDS: the host emulation's base, not used here.
#if defined(__HIP_DEVICE_COMPILE__)
    static __device__ __forceinline__ U32 lds_abs_read32(const uint8_t *lds0, U32 addr) {
        (void)lds0;
        return *(const __attribute__((address_space(3))) uint32_t *)addr;
    }
    static __device__ __forceinline__ void lds_abs_xor32(uint8_t *lds0, U32 addr, U32 v) {     // ds_xor_b32, no return
        (void)lds0;
        (void)__hip_atomic_fetch_xor((__attribute__((address_space(3))) uint32_t *)addr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    // the absolute LDS address of p, a pointer into the block's LDS (lds0: as above)
    static __device__ __forceinline__ uint32_t lds_address(const uint8_t *lds0, const uint8_t *p) {
        (void)lds0;
        return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t *)p;
    }
#else               // (the host pass of a device translation unit only parses these: LDS pointers are 32 bits wide on the device alone)
    static __device__ U32 lds_abs_read32(const uint8_t *lds0, U32 addr);
    static __device__ void lds_abs_xor32(uint8_t *lds0, U32 addr, U32 v);
    static __device__ uint32_t lds_address(const uint8_t *lds0, const uint8_t *p);
#endif
};

#endif  // __HIPCC__

}  // namespace ta
