// lev_bits_tab_body.h -- the TABLE form of the bit-parallel band kernel's stride-8 LINE form (lev_bits_body.h): the same band of up to 33
// diagonals, the same line fetch (every 128-byte line of a string requested once and parked in registers), the same
// 12-operation recurrence, bottom diagonal, zero-step count and way down -- but the match vector PM comes out of two per-pair nibble
// tables in LDS instead of 32 byte compares and a gather tree.  Levenshtein only (no transposition term), fixed-length batches.
// The strings never pass through LDS: this form reads them only through the 16 bytes of each that a block of 16 iterations needs, and
// those are taken from the parked lines register to register (run(), "the LINE fetch").  LDS holds the tables and nothing else.
//
// Tables.  Per wavefront TL[16][64] and TH[16][64] dwords, [entry][lane] (8 KB, at the start of the wavefront's LDS): bank = lane for
// any per-lane entry, so no access conflicts.  The window's 32 rows sit in 32 ring SLOTS: the row that iteration t inserts (string
// offset t - ca) owns slot t & 31.  INVARIANT: bit s of TL[v][lane] is set iff the row in slot s has low nibble v; TH likewise for the
// high nibble.  TL[b & 15] & TH[b >> 4] is then the exact match mask in slot coordinates (both bits belong to the same slot, hence the
// same row: nibbles of different rows cannot combine), and the window word -- bit i = the row i below the window's top -- is that
// mask rotated right by the top row's slot, t & 31 at iteration t: a compile-time amount, because the column loop is unrolled over the
// 32 iterations of two 16-column spans (T0 is a multiple of 64).
// Sliding.  After column t's lookup the top row leaves and the row iteration t inserts (this column's bottom diagonal, still a byte
// compare) takes its slot: bit t & 31 is flipped (ds_xor, one data register) in TL[lo(old)], TH[hi(old)], TL[lo(new)], TH[hi(new)];
// equal nibbles cancel.  `old` is the very dword `new` was 32 iterations ago: the eight dwords of `a` read for the last 32 iterations
// stay in registers (F, a ring of names: no moves), so the byte that clears a slot is the byte that set it whatever the fetch delivered --
// rows above row 1 and below row a_len included, which need no masking here either (lev_bits_body.h, header).
// Ordering.  A wavefront's LDS operations execute in order and every lane touches only its own column of the tables: lookup t, four
// flips, lookup t + 1 needs no barrier.  All of them depend on string bytes only, so column t + 1's lookup is issued before column t's
// recurrence and its latency sits under VALU work -- which the compiler has to be held to: left alone, hipcc lifts the next column's
// `mL & mH` into the current recurrence and every column waits for the whole queue, lgkmcnt(0), a third of a column behind its lookup.
// column() PINS the point where a lookup is consumed (W::opaque on the two table words), span() puts the next column's flips, its lookup
// and the addresses of the column after in front of that point, and the wait becomes a counted one that leaves those operations
// outstanding: lgkmcnt(6).  DEPTH = the lookups in flight inside a span: 1 ships; 2 issues flips t + 1 and lookup t + 2 in front of
// column t (lgkmcnt(12)) and measured slower (profiles/r13/ab_band_tab_waits.md).  tests/test_lev_bits_tab_waits_cpu.py reads the waits
// out of the assembly.
// Addresses.  lane * 4 | nibble << 8 (+ 4096 as the instruction's offset for TH): ONE SDWA instruction per address writes the nibble of the selected
// byte into byte 1 of a register that holds lane * 4 (T::nib_to_byte1, both addresses of a byte in one call; T = the table form's own operations, wave_tab.h).  They are ABSOLUTE LDS addresses
// (T::lds_abs_read32 / lds_abs_xor32): `lds` must be the start of the block's LDS, address 0 -- one wavefront per block, no static LDS.
// Per column: 6 address instructions, 1 AND, 1 rotate, 12 of the recurrence and the bottom diagonal's 2 VALU; 2 LDS reads, 4 LDS xors.
#pragma once
#include <type_traits>

#include "bitop3.h"
#include "lev_band_body.h"

namespace ta {

// what the host emulation's driver hooks in to check the invariant (tests/emu_tab); the kernels take this one: nothing
struct TabNoProbe {
    template <class U32> static TA_HD inline void block(const uint8_t *, const U32 (&)[8], uint32_t) {}
};

constexpr uint32_t LEV_TAB_TABLE_BYTES = 8192u;                                  // TL at 0, TH at 4096
constexpr uint32_t LEV_TAB_LDS_PER_WAVE = LEV_TAB_TABLE_BYTES;                   // the tables and nothing else: LDS leaves room for more wavefronts than the registers do

// how far the LDS stream runs ahead of the recurrence inside a span (span(), "Ordering" above): the depth the kernel ships with.  The other
// one is lev_bits_tab_alt.hip's (TA_TAB_DEPTH under TA_TUNING)
constexpr int LEV_TAB_DEPTH = 1;
constexpr int LEV_TAB_ALT_DEPTH = 3 - LEV_TAB_DEPTH;

template <class W, class T, class PROBE = TabNoProbe, int DEPTH = LEV_TAB_DEPTH>
struct LevBitsTab {
    static_assert(DEPTH == 1 || DEPTH == 2, "one or two lookups in flight");
    using U32 = typename W::U32;
    using Bool = typename W::Bool;
    using Ptr = typename W::Ptr;
    using Q = typename W::Q;
    static constexpr int WB = 33;

    struct State {
        U32 VP, VN;             // vertical +1 / -1 differences of the previous column, window bits 0..31 (the 33rd diagonal: lev_bits_body.h, ONEBIT)
        U32 acc;                // D0 of the window's top diagonal, the last columns' bits from bit 31 down
        U32 F[8];               // the dwords of `a` of the last 32 iterations: dword (t >> 2) & 7 holds iteration t's byte in byte t & 3
        U32 aLL, aLH;           // table addresses (byte 0 = lane * 4, byte 1 = the nibble): the lookup's,
        U32 aOL, aOH, aNL, aNH; // the leaving row's and the entering row's
        U32 bit;
        U32 mL[DEPTH + 1], mH[DEPTH + 1];   // the lookups: TL[b & 15], TH[b >> 4] of column J (of its span) in [J % (DEPTH + 1)] -- DEPTH in flight and the one its column runs on
    };

    // the addresses of column J's table entries (byte J & 3 of b_dw), then the two reads
    template <int J>
    static TA_HD inline __attribute__((always_inline)) void lookup_addr(State &st, const U32 &b_dw) {
        T::template nib_to_byte1<J & 3>(st.aLL, st.aLH, b_dw);
    }
    template <int J>
    static TA_HD inline __attribute__((always_inline)) void lookup_read(State &st, const uint8_t *lds) {
        st.mL[J % (DEPTH + 1)] = T::lds_abs_read32(lds, st.aLL);
        st.mH[J % (DEPTH + 1)] = T::lds_abs_read32(lds, st.aLH + 4096u);
    }

    // Iteration t with t & 31 == S in three parts, so that a span can order them (span()).
    // flip_addr: the addresses of the four flips -- byte S & 3 of a_new enters slot S, and (COLUMN) byte S & 3 of F[S >> 2] leaves it.
    template <int S, bool COLUMN>
    static TA_HD inline __attribute__((always_inline)) void flip_addr(State &st, const U32 &a_new) {
        if (COLUMN) T::template nib_to_byte1<S & 3>(st.aOL, st.aOH, st.F[S >> 2]);
        T::template nib_to_byte1<S & 3>(st.aNL, st.aNH, a_new);
    }
    // flips: the four of them, and a_new takes its place in F behind its last byte.
    // The slot bit is made HERE, opaque to the compiler: the flips take their data from a VGPR, and left as a plain constant all 32 of them
    // are hoisted in front of the column loop and parked for the life of the wavefront -- 32 registers and the fourth wavefront per SIMD
    // (157 against 125 VGPRs) for one v_mov_b32 per column.
    template <int S, bool COLUMN, bool OWN_BIT>
    static TA_HD inline __attribute__((always_inline)) void flips(State &st, uint8_t *lds, const U32 &a_new) {
        const U32 bit = OWN_BIT ? W::opaque(W::splat(1u << S)) : st.bit;
        if (COLUMN) {
            T::lds_abs_xor32(lds, st.aOL, bit);
            T::lds_abs_xor32(lds, st.aOH + 4096u, bit);
        }
        T::lds_abs_xor32(lds, st.aNL, bit);
        T::lds_abs_xor32(lds, st.aNH + 4096u, bit);
        if ((S & 3) == 3) st.F[S >> 2] = a_new;
    }
    // column: column t - T0 + 1 on its lookup, which was issued DEPTH steps ago.  THE PIN: the two table words pass through W::opaque right
    // here, so the lookup is consumed at this point of the instruction stream and no earlier -- behind the issue of everything span() puts
    // in front of this call, and the wait that hipcc puts here is a counted one that leaves those operations outstanding.  Without the pin
    // the scheduler lifts `mL & mH` into the middle of the column before and waits there for the whole queue, lgkmcnt(0), in every column.
    template <int S>
    static TA_HD inline __attribute__((always_inline)) void column(State &st, const U32 &a_new, const U32 &b_dw) {
        constexpr int C = S & 3;
        const U32 mH = W::opaque(st.mH[(S & 15) % (DEPTH + 1)]);        // (the later of the two reads first: one wait serves both)
        const U32 mL = W::opaque(st.mL[(S & 15) % (DEPTH + 1)]);
        if constexpr ((S & 15) + DEPTH < 16) st.bit = W::opaque(W::splat(1u << (S + DEPTH)));
        const U32 m = mL & mH;
        U32 PM;
        if constexpr (S == 0) PM = m; else PM = W::template alignbit<(S ? S : 1)>(m, m);
        // the recurrence of lev_bits_body.h, step8 (no transposition term), operation by operation
        const U32 pv = PM & st.VP;
        U32 sum;
        const typename W::Mask cm = W::add_carry_mask(pv, st.VP, sum);
        const U32 X = bitop3<0xBE>(sum, st.VP, PM);                 // (sum ^ VP) | PM
        const U32 D0 = X | st.VN;
        const U32 d0_bot = W::template byte_eq_or<C>(a_new, b_dw, cm);   // the 33rd diagonal: match | carry, in bit 0
        const U32 HP = bitop3<0xF1>(st.VN, X, st.VP);               // VN | ~(X | VP)
        const U32 HN = X & st.VP;
        st.acc = W::template alignbit<1>(D0, st.acc);
        const U32 D0s = W::template alignbit<1>(d0_bot, D0);
        st.VP = bitop3<0xF1>(HN, D0s, HP);                          // HN | ~(D0s | HP)
        st.VN = D0s & HP;
    }

    // 16 iterations tb .. tb + 15, tb & 31 == 16 PH; r[g] / bw[g] = the dwords of `a` / `b` of iterations tb + 4 g .. + 3.  TAIL: only the
    // first `left` (1..16) of them run (the columns end inside the span); nothing is issued for the others.  Warm-up spans (!COLUMN) leave
    // out their first `skip` (0..16) iterations: rows in front of the string, which run() has put into the tables already.
    // A column span finds lookup 0 issued (block()).  Its LDS stream is lookup 0, flips 0, lookup 1, flips 1, ... whatever the depth; the
    // depth says where the recurrences stand in it.  Step I issues flips I + DEPTH - 1 and lookup I + DEPTH, makes the addresses of the
    // step after, and then runs column I: at depth 1 on a lookup that has had one column's time and waits with 6 operations outstanding,
    // at depth 2 two columns' and 12.  The lead is built in front of step 0 and runs out in the last DEPTH steps: at the span's end every
    // flip below tb + 16 is issued and nothing beyond.
    template <int PH, bool COLUMN, bool TAIL>
    static TA_HD inline __attribute__((always_inline)) void span(State &st, uint8_t *lds, const U32 (&r)[4], const U32 (&bw)[4], uint32_t left, uint32_t skip) {
        if constexpr (!COLUMN) {
#define TA_TAB_WARM(I)                                                                                                   \
            if (skip <= (uint32_t)(I)) { flip_addr<16 * PH + (I), false>(st, r[(I) >> 2]); flips<16 * PH + (I), false, true>(st, lds, r[(I) >> 2]); }
            TA_TAB_WARM(0) TA_TAB_WARM(1) TA_TAB_WARM(2) TA_TAB_WARM(3) TA_TAB_WARM(4) TA_TAB_WARM(5) TA_TAB_WARM(6) TA_TAB_WARM(7)
            TA_TAB_WARM(8) TA_TAB_WARM(9) TA_TAB_WARM(10) TA_TAB_WARM(11) TA_TAB_WARM(12) TA_TAB_WARM(13) TA_TAB_WARM(14) TA_TAB_WARM(15)
#undef TA_TAB_WARM
        } else {
            // iteration J's LDS operations, J = 0..15 (nothing for J >= left in a tail): the four flips and column J + 1's lookup; then
            // the addresses of iteration J + 1's
#define TA_TAB_ADDR(J)                                                                                                   \
            if ((J) < 16) {                                                                                              \
                flip_addr<16 * PH + ((J) & 15), true>(st, r[((J) & 15) >> 2]);                                           \
                if ((J) + 1 < 16) lookup_addr<((J) + 1) & 15>(st, bw[(((J) + 1) & 15) >> 2]);                            \
            }
#define TA_TAB_ISSUE(J)                                                                                                  \
            if ((J) < 16 && (!TAIL || left > (uint32_t)(J))) {                                                           \
                flips<16 * PH + ((J) & 15), true, ((J) < DEPTH)>(st, lds, r[((J) & 15) >> 2]);                                          \
                if ((J) + 1 < 16 && (!TAIL || left > (uint32_t)(J) + 1u)) lookup_read<((J) + 1) & 15>(st, lds);          \
                TA_TAB_ADDR((J) + 1)                                                                                     \
            }
#define TA_TAB_STEP(I)                                                                                                   \
            if (!TAIL || left > (uint32_t)(I)) {                                                                         \
                TA_TAB_ISSUE((I) + DEPTH - 1)                                                                            \
                column<16 * PH + (I)>(st, r[(I) >> 2], bw[(I) >> 2]);                                                    \
            }
            TA_TAB_ADDR(0)
            if constexpr (DEPTH == 2) { TA_TAB_ISSUE(0) }
            TA_TAB_STEP(0) TA_TAB_STEP(1) TA_TAB_STEP(2) TA_TAB_STEP(3) TA_TAB_STEP(4) TA_TAB_STEP(5) TA_TAB_STEP(6) TA_TAB_STEP(7)
            TA_TAB_STEP(8) TA_TAB_STEP(9) TA_TAB_STEP(10) TA_TAB_STEP(11) TA_TAB_STEP(12) TA_TAB_STEP(13) TA_TAB_STEP(14) TA_TAB_STEP(15)
#undef TA_TAB_STEP
#undef TA_TAB_ISSUE
#undef TA_TAB_ADDR
        }
    }

    // r[g] = the four bytes from byte 4 (D + g) + sh of the eight dwords p[0..3], c[0..3] (sh = 0..3, one value per wavefront)
    template <int D>
    static TA_HD inline __attribute__((always_inline)) void window(U32 (&r)[4], const U32 (&p)[4], const U32 (&c)[4], const U32 &sh) {
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int i = D + g;
            r[g] = W::alignbyte_v(i + 1 < 4 ? p[(i + 1) & 3] : c[(i + 1) & 3], i < 4 ? p[i & 3] : c[i & 3], sh);
        }
    }

    static TA_HD inline void run(const LevParams &P, uint32_t wave_index, uint8_t *lds) {
        const U32 lane = W::lane();
        const U32 slot_idx = lane + wave_index * 64u;
        const Bool valid = slot_idx < P.n;
        const U32 pair = P.subset ? W::load_u32(P.subset, slot_idx, valid, 0u) : slot_idx;
        const Bool active = (lane == lane);

        // the batch's band (lev_plan.h): diagonals d = j - i in [-nlo, d_hi]; window bit i <-> diagonal d_hi - i.  One geometry per wavefront.
        const uint32_t alen_u = (uint32_t)P.a.len, blen_u = (uint32_t)P.b.len;
        const uint32_t diff_u = blen_u >= alen_u ? blen_u - alen_u : alen_u - blen_u;
        const bool inband = diff_u <= P.u;                  // else None (src/levenshtein.rs:426-428)
        const uint32_t nlo_u = inband ? ((P.u - diff_u) >> 1) + (blen_u >= alen_u ? 0u : diff_u) : 0u;
        const uint32_t dhi_u = (uint32_t)WB - 1u - nlo_u;
        const uint32_t idx_ans = inband ? (dhi_u + alen_u) - blen_u : 0u;   // row a_len at column b_len

        State st;
        {
            // column 0, D[r][0] = |r|: rows r = 1 - d_hi + i >= 1 step up (+1), rows <= 0 step down (-1)
            const uint32_t below = dhi_u >= 32u ? 0xFFFFFFFFu : ((1u << dhi_u) - 1u);
            st.VN = W::splat(below);
            st.VP = W::splat(~below);
        }
        st.acc = W::splat(0);
#pragma unroll
        for (int i = 0; i <= DEPTH; i++) st.mL[i] = st.mH[i] = W::splat(0);
#pragma unroll
        for (int i = 0; i < 8; i++) st.F[i] = W::splat(0);
        st.aLL = st.aLH = st.aOL = st.aOH = st.aNL = st.aNH = lane << 2;
        U32 cnt = W::splat(0);
        uint32_t nacc = 0;                                     // columns whose bits (the top nacc of st.acc) are not counted yet, <= 32
        auto flush = [&]() { cnt = W::bcnt(st.acc >> (32u - nacc), cnt); nacc = 0; };      // (nacc >= 1)

        // iteration tp inserts a[tp - T0 + nlo] into the window and, from tp = T0 on, runs column tp - T0 + 1 with b[tp - T0]
        const uint32_t T0 = P.Tw;                              // a multiple of 64 (lev_plan.h)
        const uint32_t iters = T0 + blen_u;

        // ---- the LINE fetch of lev_bits_body.h: every 128-byte line of a string requested once, whole, and parked in registers.  The strings
        // never pass through LDS: a block takes its 16 bytes of each string out of the parked line, a wave-uniform eight-way choice of the
        // piece.  Pieces in front of a string are zeros; the loads deliver zeros at and past its end
        Ptr aptr, bptr;
        U32 alen, blen;
        W::load_str(P.a, pair, valid, aptr, alen);     // rows (a lane without a pair points at the batch's first pair; its bytes go nowhere)
        W::load_str(P.b, pair, valid, bptr, blen);     // columns (a fixed-length batch: blen is blen_u in every lane)
        Q SA[8], SB[8];
        auto fetch_a = [&](int32_t m) {
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const uint32_t off = 128u * (uint32_t)m + 16u * (uint32_t)c;
                const Bool ok = off < alen_u ? active : W::bfalse();
                SA[c] = W::gload16(W::ptr_add(aptr, W::splat(off)), ok);
            }
        };
        auto fetch_b = [&](int32_t m) {
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const uint32_t off = 128u * (uint32_t)m + 16u * (uint32_t)c;
                const Bool ok = off < blen_u ? active : W::bfalse();
                SB[c] = W::gload16(W::ptr_add(bptr, W::splat(off)), ok);
            }
        };
        auto take = [&](const Q (&S)[8], int32_t piece, U32 (&d)[4]) {
            // (case_tag, LAST in every case: lev_bits_body.h, vput -- eight cases that differ only in the index of S would be sunk into one block
            // that reads S through a pointer, and S would move to scratch memory)
            switch (piece & 7) {                                   // wave-uniform: one of eight pieces
#define TA_TAKE(c) case c: { d[0] = W::qword(S[c], 0); d[1] = W::qword(S[c], 1); d[2] = W::qword(S[c], 2); d[3] = W::qword(S[c], 3); W::template case_tag<c>(); } break;
                TA_TAKE(0) TA_TAKE(1) TA_TAKE(2) TA_TAKE(3) TA_TAKE(4) TA_TAKE(5) TA_TAKE(6) TA_TAKE(7)
#undef TA_TAKE
            }
        };
        // The next line's burst is issued when a line's last piece has been taken: 16 iterations ahead of its first piece.  ONE take per
        // string and block, each in front of the block's branches (take_b serves the warm-up blocks too, with zeros): with a second call
        // site, or with the take inside a branch, hipcc keeps a second set of 32 registers for the line and copies one onto the other in
        // every block (64 v_mov per block and string, and scratch at the cap of 168 registers).
        auto take_a = [&](int32_t piece, U32 (&d)[4]) {
            if (piece < 0) {
                d[0] = d[1] = d[2] = d[3] = W::splat(0);
            } else {
                take(SA, piece, d);
                if ((piece & 7) == 7) fetch_a((piece >> 3) + 1);
            }
        };
        auto take_b = [&](int32_t piece, U32 (&d)[4]) {
            if (piece < 0) {
                d[0] = d[1] = d[2] = d[3] = W::splat(0);
            } else {
                take(SB, piece, d);
                if ((piece & 7) == 7) fetch_b((piece >> 3) + 1);
            }
        };

        // Block tb reads a[16 pa + ao ..+15] (pa = (tb - T0) / 16 + nlo / 16, ao = nlo & 15: one number per launch) and b[tb - T0 ..+15], piece
        // (tb - T0) / 16 exactly.  ao == 0 (cfg2: nlo = 16): the block is piece pa as it stands.  Otherwise it straddles pieces pa and pa + 1:
        // wa keeps piece pa from the block before, the block takes piece pa + 1 and reads its dwords out of the eight.
        const uint32_t tb0 = T0 - 32u;
        const uint32_t ao = nlo_u & 15u;
        const U32 ash = W::splat(ao & 3u);
        int32_t pa = (int32_t)(nlo_u >> 4) - 2;
        U32 wa[4];
        fetch_a(0);
        fetch_b(0);
        if (ao) take_a(pa, wa);
        else wa[0] = wa[1] = wa[2] = wa[3] = W::splat(0);

        // the warm-up: the tables zeroed (eight 16-byte stores per lane cover the 8 KB), then the 32 iterations in front of the first column
        // insert the first window's rows.  The first npre = 32 - nlo of them lie in front of the string: zero bytes in slots 0 .. npre - 1,
        // all of them bits of TL[0] and TH[0].  Those go in as one mask and their iterations are skipped (F stays zero for them).
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) W::lds_store16(lds, (lane << 4) + 1024u * i, W::qzero(), active);
        W::lds_wave_sync();                                    // (a lane's stores zero four lanes' entries)
        const uint32_t npre = 32u - (nlo_u < 32u ? nlo_u : 32u);
        if (npre) {
            const U32 pre = W::splat(npre >= 32u ? 0xFFFFFFFFu : ((1u << npre) - 1u));
            W::lds_write32(lds, lane << 2, pre);
            W::lds_write32(lds, (lane << 2) + 4096u, pre);
        }

        // one block: its dwords of `a` out of the parked line, then its 16 iterations
        auto block = [&](uint32_t tb, auto phase_tag) {
            constexpr int PH = decltype(phase_tag)::value;
            U32 r[4], bw[4];
            U32 w1[4];
            // column 0's lookup first: it needs bw[0] and the flips of the block before, which are issued, and nothing else -- the choice
            // of the block's dwords of `a` runs under it.  Unconditional, like the takes: a warm-up block looks up TL[0] / TH[0] for nobody.
            take_b(((int32_t)tb - (int32_t)T0) >> 4, bw);
            lookup_addr<0>(st, bw[0]);
            lookup_read<0>(st, lds);
            take_a(pa + (ao ? 1 : 0), w1);
            if (ao == 0u) {
#pragma unroll
                for (int g = 0; g < 4; g++) r[g] = w1[g];
            } else {
                switch (ao >> 2) {                             // wave-uniform: the dword the block starts in, then a byte shift
                    case 0: window<0>(r, wa, w1, ash); break;
                    case 1: window<1>(r, wa, w1, ash); break;
                    case 2: window<2>(r, wa, w1, ash); break;
                    default: window<3>(r, wa, w1, ash); break;
                }
#pragma unroll
                for (int g = 0; g < 4; g++) wa[g] = w1[g];
            }
            pa++;
            if (tb < T0) {
                const uint32_t done = tb - tb0;
                span<PH, false, false>(st, lds, r, bw, 16u, npre > done ? npre - done : 0u);
            } else {
                PROBE::block(lds, st.F, tb);
                if (tb + 16u <= iters) {
                    span<PH, true, false>(st, lds, r, bw, 16u, 0u);
                    nacc += 16u;
                } else {
                    span<PH, true, true>(st, lds, r, bw, iters - tb, 0u);
                    nacc += iters - tb;
                }
                if (PH == 1 || tb + 16u >= iters) flush();
            }
        };
        for (uint32_t tb = tb0; tb < iters; tb += 32u) {
            block(tb, std::integral_constant<int, 0>());
            if (tb + 16u >= iters) break;
            block(tb + 16u, std::integral_constant<int, 1>());
        }

        // the way down from the top diagonal's cell to row a_len: idx_ans steps over the last column's vertical differences
        const uint32_t mb = idx_ans >= 32u ? 0xFFFFFFFFu : ((1u << idx_ans) - 1u);
        const U32 tail = W::bcnt(st.VP & mb, W::splat(0)) - W::bcnt(st.VN & mb, W::splat(0));
        const U32 d = W::splat(dhi_u + blen_u) - cnt + tail;   // the top diagonal starts at d_hi; + columns - zero-difference steps + way down
        const Bool some = (d <= P.k) & (W::splat(inband ? 1u : 0u) != 0u);        // :539-541
        W::store_u32(P.out, pair, W::sel(some, d, W::splat(0xFFFFFFFFu)), valid);
    }
};

}  // namespace ta
