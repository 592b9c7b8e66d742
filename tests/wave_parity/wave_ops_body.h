// wave_ops_body.h -- every operation of the wave vocabulary (triple_accel_amd/csrc/wave.h, bitop3.h), applied once per case and written out
// lane by lane.  TESTS ONLY.  Compiled twice: WaveOps<DevWave> in a gfx950 kernel (wave_parity_dev.hip) and WaveOps<EmuWave> on the host
// (wave_parity_emu.cpp); tests/test_gpu_wave_parity.py asserts that the two outputs are equal bit for bit, which is what lets the
// emulation suites (test_emu_*.py) speak for the HIP kernels.
//
// Buffers (all of them the caller's, every address below stays inside them -- also in lanes whose predicate is off):
//   in   n_cases blocks of TA_WP_CASE_WORDS words: x, y, z for the 64 lanes (word (c * 3 + j) * 64 + lane).  The block doubles as the bytes
//        the global loads read (768 bytes, block base 128-byte aligned: `in` itself must be 256-byte aligned on both sides).
//   hdr  TA_WP_HDR_GLOBAL words (65 uint64 CSR offsets into a case block, then padding), then TA_WP_HDR_WORDS wave-uniform scalars per case.
//   out  TA_WP_N_OPS rows of n_cases * 64 words: out[(op * n_cases + c) * 64 + lane].  The caller fills it with a pattern first; the word
//        (append_u32:count, c, lane 0) must start as 0.  Rows of the side-effect list are written by the primitive itself.
// Predicates: p = bit 0 of z, q = bit 1 of z.
#pragma once
#include <stdint.h>

#include "bitop3.h"
#include "wave.h"

namespace ta {

#define TA_WP_CASE_WORDS 192u
#define TA_WP_CASE_BYTES 768u
#define TA_WP_HDR_GLOBAL 256u
#define TA_WP_HDR_WORDS 32u
#define TA_WP_LDS_BYTES 2560u      // per wave: 64 slots of 36 bytes (an odd number of dwords, as the bodies' slots) + slack

// header words of a case
enum : uint32_t {
    TA_WP_H_S = 0,         // shift count, 0..31
    TA_WP_H_M = 1,         // constant mask / splat value
    TA_WP_H_L = 2,         // lane index, 0..63
    TA_WP_H_KAPPA = 3,     // 0..7
    TA_WP_H_D = 4,         // divisor, != 0
    TA_WP_H_TRIPS = 5,     // trip count of the carry-chain loop
    TA_WP_H_M8 = 6,        // dot4_byte multiplier, <= 255
    TA_WP_H_XS = 7,        // lane permutation (xor) of the store_u32 row
    TA_WP_H_BFE_OFF = 8,   // 8 x (off, width): 1 <= width < 32, off + width <= 32
    TA_WP_H_BFE_W = 16,
    TA_WP_H_STRIDE = 24,   // strided StrView: 63 * stride <= 768
    TA_WP_H_LEN = 25,
};

#define TA_WP_N4(X, F) F(X, 0) F(X, 1) F(X, 2) F(X, 3)
#define TA_WP_N8(X, F) TA_WP_N4(X, F) F(X, 4) F(X, 5) F(X, 6) F(X, 7)
#define TA_WP_N32(X, F)                                                                                                          \
    TA_WP_N8(X, F) F(X, 8) F(X, 9) F(X, 10) F(X, 11) F(X, 12) F(X, 13) F(X, 14) F(X, 15) F(X, 16) F(X, 17) F(X, 18) F(X, 19)     \
    F(X, 20) F(X, 21) F(X, 22) F(X, 23) F(X, 24) F(X, 25) F(X, 26) F(X, 27) F(X, 28) F(X, 29) F(X, 30) F(X, 31)
#define TA_WP_HEX(X, FN, h)                                                                                                      \
    FN(X, h, 0) FN(X, h, 1) FN(X, h, 2) FN(X, h, 3) FN(X, h, 4) FN(X, h, 5) FN(X, h, 6) FN(X, h, 7) FN(X, h, 8) FN(X, h, 9)      \
    FN(X, h, A) FN(X, h, B) FN(X, h, C) FN(X, h, D) FN(X, h, E) FN(X, h, F)

#define TA_WP_ALIGNBYTE(X, n) X(alignbyte, n, (W::template alignbyte<n>(x, y)))
#define TA_WP_DOT4BYTE(X, n) X(dot4_byte, n, (W::dot4_byte(x, n, hm8, z)))
#define TA_WP_ALIGNBIT(X, n) X(alignbit, n, (W::template alignbit<n>(x, y)))
#define TA_WP_BFE(X, n) X(bfe, n, (W::bfe(x, hdr_c[TA_WP_H_BFE_OFF + n], hdr_c[TA_WP_H_BFE_W + n])))
#define TA_WP_BYTEOF(X, n) X(byte_of, n, (W::byte_of(x, n)))
#define TA_WP_SPLATN(X, n) X(splat_byte_n, n, (W::template splat_byte_n<n>(x)))
#define TA_WP_SLIDE(X, n) X(slide_in_byte, n, (W::template slide_in_byte<n>(x, y)))
#define TA_WP_BYTEEQ(X, n) X(byte_eq, n, (b2u(W::template byte_eq<n>(x, y))))
#define TA_WP_BYTEEQOR(X, n) X(byte_eq_or, n, (W::template byte_eq_or<n>(x, y, acm)))
#define TA_WP_PERM(X, s) X(perm, s, (W::template perm<0x##s##u>(x, y)))
#define TA_WP_B3(X, h, l) X(bitop3, h##l, (bitop3<0x##h##l>(x, y, z)))
#define TA_WP_QW(X, prim, q) X(prim, w0, (W::qword(q, 0))) X(prim, w1, (W::qword(q, 1))) X(prim, w2, (W::qword(q, 2))) X(prim, w3, (W::qword(q, 3)))
#define TA_WP_LINE(X, n)                                                                                                         \
    X(gload_line_keep, n##_w0, (W::qword(S[n], 0))) X(gload_line_keep, n##_w1, (W::qword(S[n], 1)))                              \
    X(gload_line_keep, n##_w2, (W::qword(S[n], 2))) X(gload_line_keep, n##_w3, (W::qword(S[n], 3)))
#define TA_WP_LDSR(X, n) X(lds_read32, n, (W::lds_read32(lds, nb + 4u * n)))

// every constant selector the kernel bodies pass to W::perm<> (lev_band_body.h advance_a / advance_b with BI = 0..3 and every intake byte,
// lev_bits2_body.h step() with C = 0..7 and the two transposes of run())
#define TA_WP_PERMS(X)                                                                                                           \
    TA_WP_PERM(X, 0605000C) TA_WP_PERM(X, 0605010C) TA_WP_PERM(X, 0605020C) TA_WP_PERM(X, 0605030C)                              \
    TA_WP_PERM(X, 00070605) TA_WP_PERM(X, 01070605) TA_WP_PERM(X, 02070605) TA_WP_PERM(X, 03070605)                              \
    TA_WP_PERM(X, 0C0C0C00) TA_WP_PERM(X, 0C0C0C01) TA_WP_PERM(X, 0C0C0C02) TA_WP_PERM(X, 0C0C0C03)                              \
    TA_WP_PERM(X, 0C0C0005) TA_WP_PERM(X, 0C0C0105) TA_WP_PERM(X, 0C0C0205) TA_WP_PERM(X, 0C0C0305)                              \
    TA_WP_PERM(X, 0C000605) TA_WP_PERM(X, 0C010605) TA_WP_PERM(X, 0C020605) TA_WP_PERM(X, 0C030605)                              \
    TA_WP_PERM(X, 04040000) TA_WP_PERM(X, 05050101) TA_WP_PERM(X, 06060202) TA_WP_PERM(X, 07070303)                              \
    TA_WP_PERM(X, 05030401) TA_WP_PERM(X, 07030601) TA_WP_PERM(X, 05010400) TA_WP_PERM(X, 07030602)

// X(primitive, variant, expression of type U32 in the scope of run_case())
#define TA_WAVE_OPS(X)                                                                                                           \
    X(lane, v, (lane))                                                                                                           \
    X(splat, v, (W::splat(hm)))                                                                                                  \
    X(bfalse, v, (b2u(W::bfalse())))                                                                                             \
    X(sel, v, (W::sel(p, x, y)))                                                                                                 \
    X(land, v, (b2u(W::land(p, q))))                                                                                             \
    X(umin, v, (W::umin(x, y)))                                                                                                  \
    X(umin3, v, (W::umin3(x, y, z)))                                                                                             \
    X(imax, v, (W::imax(x, y)))                                                                                                  \
    X(imax3, v, (W::imax3(x, y, z)))                                                                                             \
    X(sel_bits, v, (W::sel_bits(x, y, z)))                                                                                       \
    X(udiv, v, (W::udiv(x, hd)))                                                                                                 \
    TA_WP_N4(X, TA_WP_ALIGNBYTE)                                                                                                 \
    TA_WP_N4(X, TA_WP_DOT4BYTE)                                                                                                  \
    X(dot4, v, (W::dot4(x, y, z)))                                                                                               \
    X(sdot4, v, (W::sdot4(x, y, z)))                                                                                             \
    X(sdot4_first, v, (W::sdot4_first(x, y)))                                                                                    \
    X(ne12, v, (W::ne12(x)))                                                                                                     \
    X(splat_byte, v, (W::splat_byte(x)))                                                                                         \
    X(addc, sum, (addc_sum))                                                                                                     \
    X(addc, cout, (b2u(addc_cout)))                                                                                              \
    X(bcnt, v, (W::bcnt(x, y)))                                                                                                  \
    TA_WP_N32(X, TA_WP_ALIGNBIT)                                                                                                 \
    TA_WP_N8(X, TA_WP_BFE)                                                                                                       \
    X(lshl_add, v, (W::lshl_add(x, hs, y)))                                                                                      \
    X(alignbyte_v, v, (W::alignbyte_v(x, y, z)))                                                                                 \
    X(clz, v, (W::clz(x)))                                                                                                       \
    X(shlv, v, (W::shlv(x, z & 31u)))                                                                                            \
    X(shrv, v, (W::shrv(x, z & 31u)))                                                                                            \
    TA_WP_N4(X, TA_WP_BYTEOF)                                                                                                    \
    X(bfi, v, (W::bfi(hm, x, y)))                                                                                                \
    TA_WP_N4(X, TA_WP_SPLATN)                                                                                                    \
    TA_WP_N4(X, TA_WP_SLIDE)                                                                                                     \
    TA_WP_PERMS(X)                                                                                                               \
    X(perm_sel, v, (W::perm_sel(x, y, z)))                                                                                       \
    X(shr_u, v, (W::shr_u(x, hs)))                                                                                               \
    X(alignbit_rt, v, (W::alignbit_rt(x, y, hs)))                                                                                \
    X(and_or, v, (W::and_or(x, hm, y)))                                                                                          \
    X(bfi_k, v, (W::bfi_k(hm, x, y)))                                                                                            \
    X(add_carry_mask, sum, (acm_sum))                                                                                            \
    X(add_carry_mask, mask, (W::sel_mask(acm, W::splat(1u), W::splat(0u))))                                                      \
    X(sel_mask, v, (W::sel_mask(acm, x, z)))                                                                                     \
    TA_WP_N4(X, TA_WP_BYTEEQ)                                                                                                    \
    TA_WP_N4(X, TA_WP_BYTEEQOR)                                                                                                  \
    TA_WP_HEX(X, TA_WP_B3, 0) TA_WP_HEX(X, TA_WP_B3, 1) TA_WP_HEX(X, TA_WP_B3, 2) TA_WP_HEX(X, TA_WP_B3, 3)                      \
    TA_WP_HEX(X, TA_WP_B3, 4) TA_WP_HEX(X, TA_WP_B3, 5) TA_WP_HEX(X, TA_WP_B3, 6) TA_WP_HEX(X, TA_WP_B3, 7)                      \
    TA_WP_HEX(X, TA_WP_B3, 8) TA_WP_HEX(X, TA_WP_B3, 9) TA_WP_HEX(X, TA_WP_B3, A) TA_WP_HEX(X, TA_WP_B3, B)                      \
    TA_WP_HEX(X, TA_WP_B3, C) TA_WP_HEX(X, TA_WP_B3, D) TA_WP_HEX(X, TA_WP_B3, E) TA_WP_HEX(X, TA_WP_B3, F)                      \
    /* cross-lane */                                                                                                             \
    X(from_lower, v, (W::from_lower(x, y)))                                                                                      \
    X(from_upper, v, (W::from_upper(x, y)))                                                                                      \
    X(from_lower0, v, (W::from_lower0(x)))                                                                                       \
    X(from_upper0, v, (W::from_upper0(x)))                                                                                       \
    X(shfl, v, (W::shfl(x, y)))                                                                                                  \
    X(shfl_ptr, off, (W::ptr_lo32(W::shfl_ptr(P1, y)) - base_lo))                                                                \
    X(any, v, (W::splat(W::any(p) ? 1u : 0u)))                                                                                   \
    X(first_u32, v, (W::splat(W::any(p) ? W::first_u32(x, p) : 0xFFFFFFFFu)))                                                    \
    X(wave_max, v, (W::splat(W::wave_max(x))))                                                                                   \
    X(wave_sum, v, (W::splat(W::wave_sum(x))))                                                                                   \
    X(readlane, v, (W::splat(W::readlane(x, hl))))                                                                               \
    X(writelane, v, (W::writelane(x, hm, hl)))                                                                                   \
    /* memory */                                                                                                                 \
    X(load_str, csr_off, (W::ptr_lo32(csr_p) - base_lo))                                                                         \
    X(load_str, csr_len, (csr_len))                                                                                              \
    X(load_str, strided_off, (W::ptr_lo32(str_p) - base_lo))                                                                     \
    X(load_str, strided_len, (str_len))                                                                                          \
    X(load_u32, v, (W::load_u32(cin, y & 127u, p, 0x0DEFA017u)))                                                                 \
    X(gload_u8, v, (W::gload_u8(G, p)))                                                                                          \
    TA_WP_QW(X, gload16, W::gload16(G, p))                                                                                       \
    TA_WP_QW(X, gload16_all, qall)                                                                                               \
    TA_WP_QW(X, gload16_nt, W::gload16_nt(G, q))                                                                                 \
    TA_WP_N8(X, TA_WP_LINE)                                                                                                      \
    X(ptr_splat, off, (base_lo - W::ptr_lo32(W::ptr_splat((const uint8_t *)in))))                                                \
    X(ptr_add, off, (W::ptr_lo32(P1) - base_lo))                                                                                 \
    X(ptr_sub, off, (W::ptr_lo32(W::ptr_sub(P1, y & 127u)) - base_lo))                                                           \
    X(ptr_lo32, low7, (W::ptr_lo32(P1) & 127u))                                                                                  \
    X(ptr_piece, off, (W::ptr_lo32(W::ptr_piece(P1)) - base_lo))                                                                 \
    X(ptr_line, off, (W::ptr_lo32(W::ptr_line(P1)) - base_lo))                                                                   \
    X(sel_ptr, off, (W::ptr_lo32(W::sel_ptr(p, P1, G)) - base_lo))                                                               \
    X(qxor, w2, (W::qword(W::qxor(qall, hm), 2)))                                                                                \
    X(qxor_v, w1, (W::qword(W::qxor_v(qall, x), 1)))                                                                             \
    X(qword, w3, (W::qword(qall, 3)))                                                                                            \
    X(qkeep, w0, (W::qword(W::qkeep(qall, p), 0)))                                                                               \
    X(qzero, w3, (W::qword(W::qzero(), 3)))                                                                                      \
    TA_WP_N8(X, TA_WP_LDSR)                                                                                                      \
    X(lds_read32, 8, (W::lds_read32(lds, nb + 32u)))                                                                             \
    X(lds_store16, w2, (W::lds_read32(lds, nb + 24u)))                                                                           \
    X(lds_write32, v, (W::lds_read32(lds, nb)))                                                                                  \
    X(lds_write32p, v, (W::lds_read32(lds, nb + 4u)))                                                                            \
    X(lds_write16, v, (W::lds_read32(lds, nb + 8u)))                                                                             \
    X(lds_or32, v, (W::lds_read32(lds, nb + 12u)))                                                                               \
    X(lds_read64, lo, (r64_lo))                                                                                                  \
    X(lds_read64, hi, (r64_hi))                                                                                                  \
    X(lds_read32u, v, (W::lds_read32u(lds, nb + (y & 31u))))                                                                     \
    X(lds_u8, v, (W::lds_u8(lds, nb + (x & 31u))))                                                                               \
    /* compositions, as the bodies write them */                                                                                 \
    X(comp, carry_a, (cc_a))                                                                                                     \
    X(comp, carry_b, (cc_b))                                                                                                     \
    X(comp, carry_acc, (cc_acc))                                                                                                 \
    X(comp, carry_cnt, (W::splat(cc_cnt)))                                                                                       \
    X(comp, carry_it, (W::splat(cc_it)))                                                                                         \
    X(comp, and_or_tree, (tree_ao))                                                                                              \
    X(comp, bfi_k_tree, (tree_bfi))                                                                                              \
    X(comp, dpp_back_to_back, (W::from_upper(W::from_lower(x, y), z)))                                                           \
    X(comp, wave_max_after_sel, (W::splat(W::wave_max(W::sel(p, x, y)))))

// rows a primitive writes by itself: X(primitive, variant)
#define TA_WAVE_SIDE_ROWS(X) X(store_u32, v) X(append_u32, list) X(append_u32, count)

#define TA_WP_ENUM(prim, variant, expr) TA_WP_OP_##prim##_##variant,
#define TA_WP_ENUM_SIDE(prim, variant) TA_WP_OP_##prim##_##variant,
enum : uint32_t { TA_WAVE_OPS(TA_WP_ENUM) TA_WAVE_SIDE_ROWS(TA_WP_ENUM_SIDE) TA_WP_N_OPS };

#define TA_WP_NAME(prim, variant, expr) #prim ":" #variant,
#define TA_WP_NAME_SIDE(prim, variant) #prim ":" #variant,
#define TA_WP_DEFINE_OP_NAMES()                                                                                                  \
    static const char *const ta_wp_op_names[] = {TA_WAVE_OPS(TA_WP_NAME) TA_WAVE_SIDE_ROWS(TA_WP_NAME_SIDE)};                    \
    extern "C" const char *ta_wave_parity_op_name(int op) { return op >= 0 && op < (int)TA_WP_N_OPS ? ta_wp_op_names[op] : nullptr; } \
    extern "C" int ta_wave_parity_n_ops(void) { return (int)TA_WP_N_OPS; }

template <class W>
struct WaveOps {
    using U32 = typename W::U32;
    using Bool = typename W::Bool;
    using Ptr = typename W::Ptr;
    using Q = typename W::Q;
    using Mask = typename W::Mask;

    static TA_HD inline U32 b2u(const Bool &b) { return W::sel(b, W::splat(1u), W::splat(0u)); }

    // one step of the carry chain as step8 / column() write it: the carry mask of an addition feeds the byte test of the bottom diagonal and
    // a select, three asm statements back to back, between updates of a wave-uniform counter
    template <int N>
    static TA_HD inline __attribute__((always_inline)) void carry_step(const U32 &lane, const U32 &x, const U32 &z, uint32_t it, U32 &a, U32 &b,
                                                                       U32 &acc, uint32_t &cnt) {
        U32 sum;
        const Mask cm = W::add_carry_mask(a, b, sum);
        const U32 d = W::template byte_eq_or<N>(a, b, cm);
        const U32 e = W::sel_mask(cm, x, z);
        cnt = cnt * 3u + it + (uint32_t)N + (W::any(W::land(d == W::splat(1u), lane == W::splat(cnt & 63u))) ? 1u : 0u);
        acc = acc ^ (sum + d);
        a = sum ^ e;
        b = b + e + d + W::splat(cnt);
    }

    // all of case c; called by a whole wavefront (64 active lanes); lds: this wave's TA_WP_LDS_BYTES
    static TA_HD inline void run_case(const uint32_t *in, const uint32_t *hdr, uint32_t *out, uint32_t n_cases, uint32_t c, uint8_t *lds) {
        const U32 lane = W::lane();
        const Bool all = lane == lane;
        const uint32_t *cin = in + c * TA_WP_CASE_WORDS;
        const uint8_t *cbytes = (const uint8_t *)cin;
        const uint32_t *hdr_c = hdr + TA_WP_HDR_GLOBAL + c * TA_WP_HDR_WORDS;
        const uint32_t hs = hdr_c[TA_WP_H_S] & 31u, hm = hdr_c[TA_WP_H_M], hl = hdr_c[TA_WP_H_L] & 63u, hk = hdr_c[TA_WP_H_KAPPA] & 7u;
        const uint32_t hd = hdr_c[TA_WP_H_D], ht = hdr_c[TA_WP_H_TRIPS] & 15u, hm8 = hdr_c[TA_WP_H_M8] & 255u, hx = hdr_c[TA_WP_H_XS] & 63u;

        const U32 x = W::load_u32(cin, lane, all, 0u), y = W::load_u32(cin, lane + 64u, all, 0u), z = W::load_u32(cin, lane + 128u, all, 0u);
        const Bool p = (z & 1u) != W::splat(0u), q = (z & 2u) != W::splat(0u);

        U32 addc_sum;
        Bool addc_cout;
        W::addc(x, y, p, addc_sum, addc_cout);
        U32 acm_sum;
        const Mask acm = W::add_carry_mask(x, y, acm_sum);

        // pointers into the case block: P1 in [128, 384), G in [0, 512) (a 16-byte load at G ends inside the 768 bytes)
        const Ptr base = W::ptr_splat(cbytes);
        const U32 base_lo = W::ptr_lo32(base);
        const Ptr P1 = W::ptr_add(base, (x & 255u) + 128u);
        const Ptr G = W::ptr_add(base, x & 511u);
        const Q qall = W::gload16_all(G);

        StrView csr{cbytes, (const uint64_t *)hdr, 0, 0};
        StrView strided{cbytes, nullptr, hdr_c[TA_WP_H_STRIDE] % 13u, hdr_c[TA_WP_H_LEN]};
        Ptr csr_p, str_p;
        U32 csr_len, str_len;
        W::load_str(csr, x & 63u, p, csr_p, csr_len);
        W::load_str(strided, y & 63u, q, str_p, str_len);

        // the 128-byte line of an address in [128, 640): S keeps a recognisable value where !p
        Q S[8];
#pragma unroll
        for (int j = 0; j < 8; j++) S[j] = W::qxor(W::qzero(), 0x5EED0000u + (uint32_t)j);
        W::gload_line_keep(S, W::ptr_line(W::ptr_add(base, (y & 511u) + 128u)), p, hk);
        W::wait_vm0();

        // LDS: every lane fills its own 36-byte slot, overwrites parts of it under predicates, and reads the slot of lane + 7
        const U32 slot = lane * 36u, nb = ((lane + 7u) & 63u) * 36u;
        W::lds_wave_sync();
#pragma unroll
        for (uint32_t j = 0; j < 9; j++) W::lds_write32(lds, slot + 4u * j, x ^ (0x01010101u * (j + 1u)));
        W::lds_wave_sync();
        W::lds_write32p(lds, slot + 4u, y, p);
        W::lds_write16(lds, slot + 8u + (z & 2u), y);
        W::lds_or32(lds, slot + 12u, z, q);
        W::lds_store16(lds, slot + 16u, qall, p);
        W::lds_wave_sync();
        U32 r64_lo, r64_hi;
        W::lds_read64(lds, nb + ((z >> 8) & 28u), r64_lo, r64_hi);

        // global side effects: a lane-permuted predicated store, and an append list with its counter
        uint32_t *row_store = out + ((uint32_t)TA_WP_OP_store_u32_v * n_cases + c) * 64u;
        W::store_u32(row_store, lane ^ hx, x, p);
        W::append_u32(out + ((uint32_t)TA_WP_OP_append_u32_list * n_cases + c) * 64u,
                      out + ((uint32_t)TA_WP_OP_append_u32_count * n_cases + c) * 64u, x, q);

        // composition 1: the carry chain in a loop whose trip count, exit test and counter are wave-uniform
        U32 cc_a = x, cc_b = y, cc_acc = z;
        uint32_t cc_cnt = hm8, cc_it = 0;
        for (; cc_it < ht; cc_it++) {
            carry_step<0>(lane, x, z, cc_it, cc_a, cc_b, cc_acc, cc_cnt);
            carry_step<1>(lane, x, z, cc_it, cc_a, cc_b, cc_acc, cc_cnt);
            carry_step<2>(lane, x, z, cc_it, cc_a, cc_b, cc_acc, cc_cnt);
            carry_step<3>(lane, x, z, cc_it, cc_a, cc_b, cc_acc, cc_cnt);
            if ((cc_cnt & 7u) == 7u) break;
        }
        // composition 2: the byte test's gather, as an eight-term v_and_or chain and as the seven-node v_bfi tree of step8
        U32 M[8];
#pragma unroll
        for (uint32_t m = 0; m < 8; m++) M[m] = W::ne12((x + y * m) ^ 0x0C0C0C0Cu);
        U32 tree_ao = W::and_or(M[0], 0x01010101u, W::splat(0u));
#pragma unroll
        for (uint32_t m = 1; m < 8; m++) tree_ao = W::and_or(M[m], 0x01010101u << m, tree_ao);
        const U32 q01 = W::bfi_k(0x01010101u, M[0], M[1]), q23 = W::bfi_k(0x04040404u, M[2], M[3]);
        const U32 q45 = W::bfi_k(0x10101010u, M[4], M[5]), q67 = W::bfi_k(0x40404040u, M[6], M[7]);
        const U32 tree_bfi = W::bfi_k(0x0F0F0F0Fu, W::bfi_k(0x03030303u, q01, q23), W::bfi_k(0x30303030u, q45, q67));

#define TA_WP_PUT(prim, variant, expr) W::store_u32(out, lane + ((uint32_t)TA_WP_OP_##prim##_##variant * n_cases + c) * 64u, expr, all);
        TA_WAVE_OPS(TA_WP_PUT)
#undef TA_WP_PUT
        W::lds_wave_sync();
    }
};

}  // namespace ta
