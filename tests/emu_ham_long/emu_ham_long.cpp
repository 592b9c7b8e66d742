// emu_ham_long.cpp -- host emulation driver of the long-pair Hamming body (ham_long_body.h).  TESTS ONLY: a wavefront of 64 emulated
// lanes counts the mismatches of ONE slice, as one round of ham_long_kernel's loop over the slice ids does; and the slice length rule.
#include <stdint.h>

#include "emu_wave.h"
#include "ham_long_body.h"
#include "lev_plan.h"

using namespace ta;

// the number of i < n with a[i] != b[i].  Nothing outside a[0 .. n) and b[0 .. n) is read.
extern "C" uint32_t emu_ham_long_slice(const uint8_t *a, const uint8_t *b, uint32_t n) { return HamLong<EmuWave>::slice(a, b, n); }

// a whole pair the way the kernel cuts it: slices of S bytes, the per-slice counts added up
extern "C" uint64_t emu_ham_long_pair(const uint8_t *a, const uint8_t *b, uint64_t len, uint32_t S) {
    uint64_t sum = 0;
    for (uint64_t at = 0; at < len; at += S) sum += HamLong<EmuWave>::slice(a + at, b + at, len - at < S ? (uint32_t)(len - at) : S);
    return sum;
}

extern "C" uint32_t emu_ham_long_slice_bytes(uint64_t bytes, uint32_t s0) { return ham_long_slice_bytes(bytes, s0); }
