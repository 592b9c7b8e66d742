// bitop3.h -- any boolean function of three bit-vectors as ONE operation: on gfx950 a single v_bitop3_b32.
//
//     bitop3<TT>(a, b, c): result bit = bit (4 a + 2 b + c) of the truth table TT, bit position by bit position,
// i.e. TT is the function applied to the constants a = 0xF0, b = 0xCC, c = 0xAA  (bfi(a, b, c) = (a & b) | (~a & c) is 0xCA,
// a | ~(b | c) is 0xF1).  Written with this helper a formula reaches the instruction selector as it stands: hipcc neither
// re-associates it nor spreads an inversion over its neighbours (lev_bits_body.h, step8).
// For uint32_t in device code it is the builtin; for every other type -- the host, the 64-lane emulation type of the tests -- the
// table is evaluated with & | ^ ~ (Shannon expansion over a, the two halves of the table as functions of b and c).
#pragma once
#include <stdint.h>

#include <type_traits>

#include "wave.h"

namespace ta {

// the function of (b, c) whose 4-bit table is T4 (bit 2 b + c)
template <uint8_t T4, class T>
TA_HD inline T bitop2_generic(const T &b, const T &c) {
    static_assert(T4 < 16, "a table of two inputs has four rows");
    if constexpr (T4 == 0) return T(0u);
    else if constexpr (T4 == 1) return ~(b | c);
    else if constexpr (T4 == 2) return ~b & c;
    else if constexpr (T4 == 3) return ~b;
    else if constexpr (T4 == 4) return b & ~c;
    else if constexpr (T4 == 5) return ~c;
    else if constexpr (T4 == 6) return b ^ c;
    else if constexpr (T4 == 7) return ~(b & c);
    else if constexpr (T4 == 8) return b & c;
    else if constexpr (T4 == 9) return ~(b ^ c);
    else if constexpr (T4 == 10) return c;
    else if constexpr (T4 == 11) return ~b | c;
    else if constexpr (T4 == 12) return b;
    else if constexpr (T4 == 13) return b | ~c;
    else if constexpr (T4 == 14) return b | c;
    else return ~T(0u);
}

template <uint8_t TT, class T>
TA_HD inline T bitop3_generic(const T &a, const T &b, const T &c) {
    constexpr uint8_t HI = TT >> 4, LO = TT & 15;      // the rows with a = 1 / a = 0
    if constexpr (HI == LO) return bitop2_generic<LO, T>(b, c);
    else if constexpr (LO == 0) return a & bitop2_generic<HI, T>(b, c);
    else if constexpr (HI == 0) return ~a & bitop2_generic<LO, T>(b, c);
    else if constexpr (HI == 15) return a | bitop2_generic<LO, T>(b, c);
    else if constexpr (LO == 15) return ~a | bitop2_generic<HI, T>(b, c);
    else if constexpr ((HI ^ LO) == 15) return a ^ bitop2_generic<LO, T>(b, c);
    else return (a & bitop2_generic<HI, T>(b, c)) | (~a & bitop2_generic<LO, T>(b, c));
}

template <uint8_t TT, class T>
TA_HD inline __attribute__((always_inline)) T bitop3(const T &a, const T &b, const T &c) {
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (std::is_same<T, uint32_t>::value) return __builtin_amdgcn_bitop3_b32(a, b, c, TT);
    else
#endif
    return bitop3_generic<TT, T>(a, b, c);
}

}  // namespace ta
