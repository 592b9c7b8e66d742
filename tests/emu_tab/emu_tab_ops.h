// emu_tab_ops.h -- 64-lane host twin of DevTab (triple_accel_amd/csrc/wave_tab.h).  TESTS ONLY, like emu_wave.h.
#pragma once
#include <stdint.h>
#include <string.h>

#include "emu_wave.h"

namespace ta {

struct EmuTab {
    using U32 = V32;
    template <int N>
    static void nib_to_byte1(U32 &addr_lo, U32 &addr_hi, const U32 &x) {
        TA_EMU_REQUIRE(&addr_lo != &addr_hi, "nib_to_byte1: two different address registers");
        for (int i = 0; i < 64; i++) {
            const uint32_t byte = (x.v[i] >> (8 * N)) & 0xFFu;
            addr_lo.v[i] = (addr_lo.v[i] & 0xFFFF00FFu) | ((byte & 0x0Fu) << 8);
            addr_hi.v[i] = (addr_hi.v[i] & 0xFFFF00FFu) | ((byte >> 4) << 8);
        }
    }
    static U32 lds_abs_read32(const uint8_t *lds0, const U32 &addr) { V32 r; for (int i = 0; i < 64; i++) memcpy(&r.v[i], lds0 + addr.v[i], 4); return r; }
    static void lds_abs_xor32(uint8_t *lds0, const U32 &addr, const U32 &v) {
        for (int i = 0; i < 64; i++) { uint32_t t; memcpy(&t, lds0 + addr.v[i], 4); t ^= v.v[i]; memcpy(lds0 + addr.v[i], &t, 4); }
    }
    static uint32_t lds_address(const uint8_t *lds0, const uint8_t *p) { return (uint32_t)(p - lds0); }
};

}  // namespace ta
