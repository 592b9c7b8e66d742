// bitop3_check.cpp -- the generic (non-builtin) path of bitop3<TT>() (triple_accel_amd/csrc/bitop3.h) against the definition of a
// truth table: all 256 tables x 8 input rows, on uint32_t and on the 64-lane emulation type the kernel bodies run on in the tests;
// then the tables lev_bits_body.h uses against their written-out expressions on random words.  Plain g++, no GPU.
#include <stdint.h>
#include <stdio.h>

#include <utility>

#include "bitop3.h"
#include "emu_wave.h"

using ta::bitop3;
using ta::V32;

static int failures = 0;

static void fail(const char *what, unsigned tt, unsigned row) {
    if (failures++ < 10) printf("FAIL %s: table 0x%02X row %u\n", what, tt, row);
}

template <uint8_t TT>
static void check_table() {
    // the definition itself: the table applied to the three constants gives the table back
    if ((bitop3<TT>(uint32_t(0xF0u), uint32_t(0xCCu), uint32_t(0xAAu)) & 0xFFu) != TT) fail("constants", TT, 8);
    // row by row on whole words: inputs all-zeros / all-ones, the result is bit (4 a + 2 b + c) of the table in every position
    V32 va, vb, vc;
    for (unsigned row = 0; row < 8; row++) {
        const uint32_t a = (row & 4) ? 0xFFFFFFFFu : 0u, b = (row & 2) ? 0xFFFFFFFFu : 0u, c = (row & 1) ? 0xFFFFFFFFu : 0u;
        const uint32_t want = ((TT >> row) & 1) ? 0xFFFFFFFFu : 0u;
        if (bitop3<TT>(a, b, c) != want) fail("uint32_t", TT, row);
        const uint64_t a64 = (row & 4) ? ~uint64_t(0) : 0u, b64 = (row & 2) ? ~uint64_t(0) : 0u, c64 = (row & 1) ? ~uint64_t(0) : 0u;
        if (bitop3<TT>(a64, b64, c64) != (((TT >> row) & 1) ? ~uint64_t(0) : uint64_t(0))) fail("uint64_t", TT, row);
        for (int l = 0; l < 64; l++) {          // the emulation type: lane l carries row (l + row) & 7, mixed into distinct bit patterns
            const unsigned r = (unsigned)(l + row) & 7u;
            va.v[l] = (r & 4) ? 0xFFFFFFFFu : 0u; vb.v[l] = (r & 2) ? 0xFFFFFFFFu : 0u; vc.v[l] = (r & 1) ? 0xFFFFFFFFu : 0u;
        }
        const V32 vr = bitop3<TT>(va, vb, vc);
        for (int l = 0; l < 64; l++) {
            const unsigned r = (unsigned)(l + row) & 7u;
            if (vr.v[l] != (((TT >> r) & 1) ? 0xFFFFFFFFu : 0u)) fail("V32", TT, r);
        }
    }
}

template <size_t... I>
static void check_all(std::index_sequence<I...>) { (check_table<(uint8_t)I>(), ...); }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

int main() {
    check_all(std::make_index_sequence<256>());
    for (int i = 0; i < 20000; i++) {
        const uint32_t a = rnd(), b = rnd(), c = rnd();
        if (bitop3<0x35>(a, b, c) != ~((a & b) | (~a & c))) fail("0x35 = ~bfi(a, b, c)", 0x35, 0);
        if (bitop3<0xCA>(a, b, c) != ((a & b) | (~a & c))) fail("0xCA = bfi(a, b, c)", 0xCA, 0);
        if (bitop3<0xBE>(a, b, c) != ((a ^ b) | c)) fail("0xBE = (a ^ b) | c", 0xBE, 0);
        if (bitop3<0xF1>(a, b, c) != (a | ~(b | c))) fail("0xF1 = a | ~(b | c)", 0xF1, 0);
        if (bitop3<0xFE>(a, b, c) != (a | b | c)) fail("0xFE = a | b | c", 0xFE, 0);
        if (bitop3<0x08>(a, b, c) != (~a & b & c)) fail("0x08 = ~a & b & c", 0x08, 0);
        // the identities of the 12-operation column (lev_bits_body.h, step8): VP and VN disjoint, D0 = X | VN
        const uint32_t VP = a & ~b, VN = b & ~a, X = c, D0 = X | VN;
        if ((D0 & VP) != (X & VP)) fail("HN = X & VP", 0, 0);
        if ((VN | ~(D0 | VP)) != bitop3<0xF1>(VN, X, VP)) fail("HP = VN | ~(X | VP)", 0xF1, 0);
    }
    if (failures) { printf("bitop3: %d failures\n", failures); return 1; }
    printf("bitop3: ok\n");
    return 0;
}
