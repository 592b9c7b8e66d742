// hay_line.h -- a lane's share of the haystack, requested one line ahead (device only).
//
// A line is NQ 16-byte quads, all requested in one burst: with NQ = 8 and tiles that start on 128-byte multiples every line of the
// haystack crosses the L2's fabric side once (two 64-byte bursts 64 columns apart measured 1.31x: the second half had left the 4 MB L2 by
// the time its lane came back for it).  Quads that start at or behind `end` are not read (haystack blobs carry 16 bytes of slack: the
// last quad may reach that far past `end`).
#pragma once
#include <stdint.h>

namespace ta {

typedef uint32_t u32x4u __attribute__((ext_vector_type(4), aligned(1)));

// nxt = the line at byte i (zeros from `end` on)
template <int NQ>
static __device__ __forceinline__ void hay_line_prime(u32x4u (&nxt)[NQ], const uint8_t *hay, uint64_t i, uint64_t end) {
#pragma unroll
    for (int q = 0; q < NQ; q++) nxt[q] = (i + 16u * q < end) ? *(const u32x4u *)(hay + i + 16u * q) : u32x4u{0, 0, 0, 0};
}

// cur = the line at byte i (requested a turn ago); nxt = the one behind it, requested now
template <int NQ>
static __device__ __forceinline__ void hay_line_turn(u32x4u (&cur)[NQ], u32x4u (&nxt)[NQ], const uint8_t *hay, uint64_t i, uint64_t end) {
#pragma unroll
    for (int q = 0; q < NQ; q++) cur[q] = nxt[q];
#pragma unroll
    for (int q = 0; q < NQ; q++)
        if (i + 16u * NQ + 16u * q < end) nxt[q] = *(const u32x4u *)(hay + i + 16u * NQ + 16u * q);
}

}  // namespace ta
