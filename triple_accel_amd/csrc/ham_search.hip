// ham_search.hip -- gfx950 kernels for hamming_search over a haystack shard in HBM; the route between them: ham_search_plan.h.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ham_search_body.h"
#include "ham_search_plan.h"
#include "ham_swar_body.h"
#include "hay_line.h"
#include "lds_tab64.h"
#include "ta_internal.h"

namespace ta {

// hamming_search: one lane per aligned group of 4 consecutive haystack offsets.  The lane loads the aligned dwords
// covering its 4 windows once (coalesced), re-aligns them per offset with v_alignbyte, and counts non-zero bytes of
// window ^ needle with the SWAR test + v_bcnt accumulate.  Replaces hamming_search_simd_core_*
// (src/hamming.rs:481-552); contract: mismatches(offset) <= k for every offset 0..=h-n.
__global__ __launch_bounds__(256) void hamming_search_kernel(SearchParams P, uint32_t delta) {
    const uint64_t grp = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // aligned dword index of the group's first byte
    const uint32_t n = P.needle_len;
    const uint64_t h = P.hay_len;
    const uint64_t last = h - n;                                            // last valid offset
    const uint64_t byte0 = grp * 4;                                         // in the aligned-down address space
    if (byte0 > last + delta) return;
    const uint32_t *hw = (const uint32_t *)(P.hay - delta) + grp;
    const uint32_t nwords = (n + 3) >> 2;
    const uint32_t tail_mask = (n & 3) ? (0xFFFFFFFFu >> (8 * (4 - (n & 3)))) : 0xFFFFFFFFu;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    uint32_t lo = hw[0];
    for (uint32_t w = 0; w < nwords; w++) {
        const uint32_t hi = hw[w + 1];
        uint32_t nd;                                                        // needle word w (wave-uniform)
        {
            typedef uint32_t u32u __attribute__((aligned(1)));
            nd = *(const u32u *)(P.needle_dev + 4 * w);                     // needle_dev carries 16 bytes of slack
        }
        // byte test with one v_perm_b32 (wave.h ne12): the needle word carries ^ 0x0C, a window byte then XORs to 12 exactly
        // where it matches; bytes past the needle's end are forced to 12.  Every mismatching byte adds 8 one-bits.
        const uint32_t m = (w + 1 == nwords) ? tail_mask : 0xFFFFFFFFu;
        const uint32_t nd12 = nd ^ 0x0C0C0C0Cu, pad = 0x0C0C0C0Cu & ~m;
        auto nz = [&](uint32_t win) -> uint32_t {
            return __builtin_amdgcn_perm(0xFFFFFFFFu, 0xFFFFFFFFu, ((win ^ nd12) & m) | pad);
        };
        c0 += __builtin_popcount(nz(lo));
        c1 += __builtin_popcount(nz(__builtin_amdgcn_alignbyte(hi, lo, 1)));
        c2 += __builtin_popcount(nz(__builtin_amdgcn_alignbyte(hi, lo, 2)));
        c3 += __builtin_popcount(nz(__builtin_amdgcn_alignbyte(hi, lo, 3)));
        lo = hi;
    }
    const uint32_t cnt[4] = {c0 >> 3, c1 >> 3, c2 >> 3, c3 >> 3};
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint64_t b = byte0 + r;
        if (b < delta) continue;
        const uint64_t pos = b - delta;
        if (pos > last) continue;
        if (cnt[r] <= P.k) {
            unsigned long long idx = atomicAdd(P.count, 1ull);
            if (idx < P.cap) P.hits[idx] = ta_match{P.base + pos, P.base + pos + n, cnt[r], 0u};
        }
    }
}

// needles of up to 64 bytes, SWAR form (ham_swar_body.h): one lane per 16 consecutive offsets, three 16-byte loads per lane in flight
// together, the windows of a lane shifted once and shared by its offsets.  The NUL-byte scan of the SIMD contract (src/lib.rs:237-243)
// rides along: every haystack dword is the first of exactly one lane's four.  delta = hay & 15 (the loads are 16-byte aligned).
template <int NW>
__global__ __launch_bounds__(256) void hamming_search_swar16_kernel(SearchParams P, uint32_t delta, uint32_t *nul_flag) {
    const uint64_t lane_id = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t byte0 = lane_id * 16u;                       // in the address space of hay - delta
    const uint32_t n = P.needle_len, k = P.k;
    const uint64_t h = P.hay_len, last = h - n, end = (uint64_t)delta + h;   // bytes [delta, end) are the haystack; 16 bytes of slack follow
    if (byte0 >= end) return;                                   // (the lanes behind the last offset still check their bytes for NUL)
    uint32_t nd12[NW], tail_mask, tail_pad;
    ham_swar_needle<NW>(P.needle, n, nd12, tail_mask, tail_pad);
    typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(16)));
    const u32x4a *src = (const u32x4a *)(P.hay - delta + byte0);
    constexpr int NQ = (4 + NW + 3) / 4;
    u32x4a q[NQ];
#pragma unroll
    for (int t = 0; t < NQ; t++) q[t] = (byte0 + 16u * (uint64_t)t <= end) ? src[t] : u32x4a{0u, 0u, 0u, 0u};
    uint32_t w[4 + NW];
#pragma unroll
    for (int i = 0; i < 4 + NW; i++) w[i] = q[i >> 2][i & 3];
    if (nul_flag) {                                             // bytes byte0 .. byte0 + 15 are this lane's to check
        bool z;
        if (byte0 >= delta && byte0 + 16u <= end) {
            z = (ham_ne12(w[0] ^ 0x0C0C0C0Cu) & ham_ne12(w[1] ^ 0x0C0C0C0Cu) & ham_ne12(w[2] ^ 0x0C0C0C0Cu) & ham_ne12(w[3] ^ 0x0C0C0C0Cu)) != 0xFFFFFFFFu;
        } else {
            z = false;
            for (uint32_t b = 0; b < 16u; b++) {
                const uint64_t x = byte0 + b;
                if (x >= delta && x < end) z |= ((w[b >> 2] >> (8u * (b & 3u))) & 0xFFu) == 0u;
            }
        }
        if (z) atomicOr(nul_flag, 1u);
    }
    uint32_t cnt[16];
    ham_swar_lane<NW>(w, nd12, tail_mask, tail_pad, cnt);
    // the counts are 8 x the mismatches: one minimum over the sixteen (v_min3) against 8 k + 7 decides whether the lane reports at all
    const uint32_t thr = k >= 0x1FFFFFFFu ? 0xFFFFFFFFu : 8u * k + 7u;
    auto min3 = [](uint32_t a, uint32_t b, uint32_t c) { const uint32_t m = a < b ? a : b; return m < c ? m : c; };
    const uint32_t m0 = min3(cnt[0], cnt[1], cnt[2]), m1 = min3(cnt[3], cnt[4], cnt[5]), m2 = min3(cnt[6], cnt[7], cnt[8]),
                   m3 = min3(cnt[9], cnt[10], cnt[11]), m4 = min3(cnt[12], cnt[13], cnt[14]);
    if (min3(min3(m0, m1, m2), min3(m3, m4, cnt[15]), 0xFFFFFFFFu) > thr) return;
#pragma unroll 1
    for (uint32_t o = 0; o < 16u; o++) {
        const uint64_t x = byte0 + o;
        if (cnt[o] > thr || x < delta || x - delta > last) continue;
        const uint64_t pos = x - delta;
        unsigned long long idx = atomicAdd(P.count, 1ull);
        if (idx < P.cap) P.hits[idx] = ta_match{P.base + pos, P.base + pos + n, cnt[o] >> 3, 0u};
    }
}

// needles of 9..32 bytes with a small k, bit-sliced counters (ham_bits_body.h): one lane per tile of P.tile bytes (a multiple of 128), the
// 256-entry Mis table once per lane in LDS (64 KB, 512 threads: two workgroups per CU), a whole 128-byte line per lane per burst one line
// ahead.  The NUL-byte scan rides along (the lane checks the bytes of its own tile).
template <int B>
__global__ __launch_bounds__(512) void hamming_search_bits_kernel(SearchParams P, uint32_t *nul_flag) {
    __shared__ __attribute__((aligned(16))) uint32_t mis[256 * 64];
    tab64_fill(mis, ham_bits_mis(P.needle, P.needle_len, threadIdx.x >> 1));
    __syncthreads();
    const uint32_t lane_off = (threadIdx.x & 63u) * 4u;
    auto lookup = [&](uint32_t v, int b) -> uint32_t { return tab64_lookup(mis, lane_off, v, b); };
    const uint32_t n = P.needle_len, k = P.k;
    const uint64_t h = P.hay_len, last = h - n;
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t b0 = tile * P.tile;                             // this lane reports the alignments that END at bytes [b0, b1)
    if (b0 >= h) return;
    const uint64_t b1 = b0 + P.tile < h ? b0 + P.tile : h;
    const uint8_t *hay = P.hay;
    HamBitsState<B> st;
    ham_bits_reset<B>(st, n);
    uint32_t bias[B];
    ham_bits_bias<B>(k, n, bias);
    for (uint64_t i = b0 > n - 1u ? b0 - (n - 1u) : 0; i < b0; i++) ham_bits_step<B>(st, lookup(hay[i], 0), bias);   // the n - 1 bytes in front
    auto report = [&](uint64_t x) {                                // the alignment ending at byte x has at most k mismatches
        if (x < n - 1u) return;                                    // (no alignment ends there: the verdict bits of a haystack's first bytes)
        const uint64_t pos = x - (n - 1u);
        if (pos > last) return;
        uint32_t cnt = 0;
        for (uint32_t j = 0; j < n; j++) cnt += hay[pos + j] != P.needle[j];           // (n <= 32: the kernarg copy)
        const unsigned long long idx = atomicAdd(P.count, 1ull);
        if (idx < P.cap) P.hits[idx] = ta_match{P.base + pos, P.base + pos + n, cnt, 0u};
    };
    uint64_t i = b0;
    const uint64_t full_end = b0 + ((b1 - b0) & ~(uint64_t)127);
    uint32_t nz = 0xFFFFFFFFu;                                     // AND of the byte tests: 0xFF per byte that is not NUL
    u32x4u nxt[8], cur[8];
    // (hay_line.h's loader written out: through hay_line_prime / hay_line_turn the prologue is scheduled in another order and this kernel
    // measured 0.2-0.5 % slower than before, outside the earlier build's two runs: profiles/r17/README.md)
#pragma unroll
    for (int q = 0; q < 8; q++) nxt[q] = (i + 16u * q < b1) ? *(const u32x4u *)(hay + i + 16u * q) : u32x4u{0, 0, 0, 0};
    while (i < full_end) {                                         // whole lines
#pragma unroll
        for (int q = 0; q < 8; q++) cur[q] = nxt[q];
#pragma unroll
        for (int q = 0; q < 8; q++)                                // blobs carry 16 bytes of slack
            if (i + 128u + 16u * q < b1) nxt[q] = *(const u32x4u *)(hay + i + 128u + 16u * q);
#pragma unroll 1
        for (int part = 0; part < 4; part++) {                     // 32 bytes = 32 verdicts per register
            uint32_t acc = 0;
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const u32x4u v = part == 0 ? cur[q] : part == 1 ? cur[2 + q] : part == 2 ? cur[4 + q] : cur[6 + q];
#pragma unroll
                for (int b = 0; b < 16; b++) {
                    const uint32_t ov = ham_bits_step<B>(st, lookup(v[b >> 2], b & 3), bias);
                    acc = __builtin_amdgcn_alignbit(acc, ov, 31);   // (acc << 1) | (ov >> 31)
                }
                if (nul_flag) nz &= ham_ne12(v[0] ^ 0x0C0C0C0Cu) & ham_ne12(v[1] ^ 0x0C0C0C0Cu) & ham_ne12(v[2] ^ 0x0C0C0C0Cu) & ham_ne12(v[3] ^ 0x0C0C0C0Cu);
            }
            if (acc != 0xFFFFFFFFu)                                // bit 31 - t = the verdict of byte i + 32 part + t
                for (uint32_t t = 0; t < 32u; t++)
                    if (!((acc >> (31u - t)) & 1u)) report(i + 32u * (uint32_t)part + t);
        }
        i += 128;
    }
    for (; i < b1; i++) {                                          // the tile's last, partial line
        const uint32_t c = hay[i];
        if (!(ham_bits_step<B>(st, lookup(c, 0), bias) >> 31)) report(i);
        if (nul_flag && c == 0u) nz = 0;
    }
    if (nul_flag && nz != 0xFFFFFFFFu) atomicOr(nul_flag, 1u);
}

// Bit-sliced counters over a subset of the needle's positions, Q phases per dword (ham_phase_body.h): any needle length; one lane per tile of
// P.tile bytes (a multiple of 128), the 256-entry phase-0 Mis table once per lane in LDS (64 KB, 512 threads), a whole 128-byte line per
// lane per burst one line ahead.  A 16-byte piece is 16 / Q steps whose verdict words are AND-ed: only a piece that holds a candidate looks
// at them one by one, and a candidate is recounted over the whole needle.  The NUL-byte scan rides along.
template <int Q, int B>
__global__ __launch_bounds__(512) void hamming_search_phase_kernel(SearchParams P, HamPhaseGeom G, uint32_t *nul_flag) {
    __shared__ __attribute__((aligned(16))) uint32_t mis[256 * 64];
    tab64_fill(mis, ham_phase_mis(P.needle_len <= 64u ? P.needle : P.needle_dev, G, threadIdx.x >> 1));   // (up to 64 bytes: the kernarg copy, no upload)
    __syncthreads();
    constexpr uint32_t W = 32u / Q, STEPS = 16u / Q;
    const uint32_t lane_off = (threadIdx.x & 63u) * 4u;
    auto lookup = [&](uint32_t v, int b) -> uint32_t { return tab64_lookup(mis, lane_off, v, b); };
    const uint32_t n = P.needle_len, k = P.k, keep = G.keep, span = G.span;
    const uint64_t h = P.hay_len, last = h - n;
    const uint64_t tile = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t b0 = tile * P.tile;                             // this lane reports the alignments whose VERDICT byte is in [b0, b1)
    if (b0 >= h) return;
    const uint64_t b1 = b0 + P.tile < h ? b0 + P.tile : h;
    const uint8_t *hay = P.hay;
    HamBitsState<B> st;
    ham_phase_reset<B>(st, G);
    uint32_t bias[B];
    ham_phase_bias<B>(k, G, bias);
    auto bytes_step = [&](uint64_t i) -> uint32_t {                // one step from single bytes (warm-up, the last partial line)
        uint32_t m = 0;
#pragma unroll
        for (int r = Q - 1; r >= 0; r--) {
            const uint32_t c = i + (uint32_t)r < h ? hay[i + (uint32_t)r] : 0u;
            const uint32_t t = lookup(c, 0);
            m = Q == 1 ? t : ((m << (W & 31u)) | t);
        }
        return ham_phase_step<B, (Q > 1)>(st, m, bias, keep);
    };
    for (uint64_t i = b0 > span ? b0 - span : 0; i < b0; i += Q) bytes_step(i);   // the span bytes in front (b0 and span are multiples of Q)
    auto verify = [&](uint64_t x) {                                // the alignment whose verdict byte is x passed the filter
        if (x < span) return;                                      // (no alignment ends there: the verdict bits of a haystack's first bytes)
        const uint64_t pos = x - span;
        if (pos > last) return;
        uint32_t cnt = 0;
        const uint8_t *nd = n <= 64u ? P.needle : P.needle_dev;
        for (uint32_t j = 0; j < n; j++) cnt += hay[pos + j] != nd[j];
        if (cnt > k) return;
        const unsigned long long idx = atomicAdd(P.count, 1ull);
        if (idx < P.cap) P.hits[idx] = ta_match{P.base + pos, P.base + pos + n, cnt, 0u};
    };
    uint64_t i = b0;
    const uint64_t full_end = b0 + ((b1 - b0) & ~(uint64_t)127);
    uint32_t nz = 0xFFFFFFFFu;                                     // AND of the byte tests: 0xFF per byte that is not NUL
    u32x4u nxt[8], cur[8];
    // (hay_line.h's loader written out: through hay_line_prime / hay_line_turn the prologue is scheduled in another order and this kernel
    // measured 0.2-0.5 % slower than before, outside the earlier build's two runs: profiles/r17/README.md)
#pragma unroll
    for (int q = 0; q < 8; q++) nxt[q] = (i + 16u * q < b1) ? *(const u32x4u *)(hay + i + 16u * q) : u32x4u{0, 0, 0, 0};
    while (i < full_end) {                                         // whole lines
#pragma unroll
        for (int q = 0; q < 8; q++) cur[q] = nxt[q];
#pragma unroll
        for (int q = 0; q < 8; q++)                                // blobs carry 16 bytes of slack
            if (i + 128u + 16u * q < b1) nxt[q] = *(const u32x4u *)(hay + i + 128u + 16u * q);
#pragma unroll 1
        for (int part = 0; part < 4; part++) {
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const u32x4u v = part == 0 ? cur[q] : part == 1 ? cur[2 + q] : part == 2 ? cur[4 + q] : cur[6 + q];
                // windows of at most 8 steps: their verdict words are kept (8 registers) and AND-ed; only a window that holds a candidate
                // looks at them one by one
                constexpr uint32_t WIN = STEPS > 8u ? 8u : STEPS;
#pragma unroll
                for (uint32_t w0 = 0; w0 < STEPS; w0 += WIN) {
                    uint32_t ov[WIN];
#pragma unroll
                    for (uint32_t s = 0; s < WIN; s++) {
                        uint32_t m = 0;
#pragma unroll
                        for (int r = Q - 1; r >= 0; r--) {
                            const uint32_t b = Q * (w0 + s) + (uint32_t)r;
                            const uint32_t t = lookup(v[b >> 2], b & 3);
                            m = Q == 1 ? t : ((m << (W & 31u)) | t);
                        }
                        ov[s] = ham_phase_step<B, (Q > 1)>(st, m, bias, keep);
                    }
                    uint32_t all = ov[0];
#pragma unroll
                    for (uint32_t s = 1; s < WIN; s++) all &= ov[s];
                    if ((all | keep) != 0xFFFFFFFFu) {              // a phase top that is clear: a candidate somewhere in this window
                        uint32_t cm = 0;                           // bit Q s + r: the verdict of byte Q (w0 + s) + r of the piece
#pragma unroll
                        for (uint32_t s = 0; s < WIN; s++) {
                            uint32_t o = ov[s];
                            asm volatile("" : "+v"(o));             // (keeps the sorting of the verdicts inside the rare branch: hipcc hoists it otherwise)
#pragma unroll
                            for (uint32_t r = 0; r < (uint32_t)Q; r++)
                                cm |= ((~o >> (r * W + W - 1u)) & 1u) << (Q * s + r);
                        }
                        const uint64_t first = i + 32u * (uint32_t)part + 16u * (uint32_t)q + Q * w0;
                        while (cm) {
                            const uint32_t t = (uint32_t)__builtin_ctz(cm);
                            cm &= cm - 1u;
                            verify(first + t);
                        }
                    }
                }
                if (nul_flag) nz &= ham_ne12(v[0] ^ 0x0C0C0C0Cu) & ham_ne12(v[1] ^ 0x0C0C0C0Cu) & ham_ne12(v[2] ^ 0x0C0C0C0Cu) & ham_ne12(v[3] ^ 0x0C0C0C0Cu);
            }
        }
        i += 128;
    }
    for (; i < b1; i += Q) {                                       // the tile's last, partial line, step by step
        const uint32_t ov = bytes_step(i);
#pragma unroll
        for (uint32_t r = 0; r < (uint32_t)Q; r++) {
            if (!((ov >> (r * W + W - 1u)) & 1u)) verify(i + r);
            if (nul_flag && i + r < h && hay[i + r] == 0u) nz = 0;
        }
    }
    if (nul_flag && nz != 0xFFFFFFFFu) atomicOr(nul_flag, 1u);
}

// needles of up to 32 bytes: shift-add scan (ham_search_body.h), one lane per tile of P.tile offsets, table in LDS,
// haystack requested 64 bytes per lane one block ahead
template <int NWS>
__global__ __launch_bounds__(256) void hamming_search_sa_kernel(SearchParams P) {
    __shared__ uint32_t tab[256 * NWS];
    for (int w = 0; w < NWS; w++) tab[threadIdx.x * NWS + w] = ham_sa_table_word(P.needle, P.needle_len, threadIdx.x, w);
    __syncthreads();
    const uint32_t n = P.needle_len, k = P.k;
    const uint64_t offsets = P.hay_len - n + 1;
    const uint64_t ob = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * P.tile;
    if (ob >= offsets) return;
    const uint64_t oe = ob + P.tile < offsets ? ob + P.tile : offsets;
    const uint8_t *hay = P.hay;
    HamSaState<NWS> st;
#pragma unroll
    for (int w = 0; w < NWS; w++) st.S[w] = 0;
    auto stepc = [&](uint32_t c) -> uint32_t {
        uint32_t Tc[NWS];
#pragma unroll
        for (int w = 0; w < NWS; w++) Tc[w] = tab[c * NWS + w];
        return ham_sa_step<NWS>(st, Tc, n);
    };
    auto emit = [&](uint64_t p, uint32_t cnt) {
        unsigned long long idx = atomicAdd(P.count, 1ull);
        if (idx < P.cap) P.hits[idx] = ta_match{P.base + p, P.base + p + n, cnt, 0u};
    };
    uint64_t i = ob;
    for (; i < ob + (n - 1); i++) stepc(hay[i]);                  // the first n-1 bytes complete no offset
    const uint64_t end = oe + (n - 1);                            // one past the last byte this tile reads
    const uint64_t full_end = i + ((end - i) & ~(uint64_t)63);
    u32x4u nxt[4], cur[4];
    hay_line_prime<4>(nxt, hay, i, end);
    while (i < full_end) {
        hay_line_turn<4>(cur, nxt, hay, i, end);
#pragma unroll 1
        for (int q = 0; q < 4; q++) {
#pragma unroll
            for (int b = 0; b < 16; b++) {
                const uint32_t cnt = stepc((cur[q][b >> 2] >> (8 * (b & 3))) & 0xffu);
                if (cnt <= k) emit(i + 16u * q + b - (n - 1), cnt);
            }
        }
        i += 64;
    }
    for (; i < end; i++) {
        const uint32_t cnt = stepc(hay[i]);
        if (cnt <= k) emit(i - (n - 1), cnt);
    }
}

// f(integral constant B) for the B = 1..5 counter planes of the bits and phase forms (ham_bits_planes stops at 5)
template <class F>
static void with_planes(int B, F f) {
    switch (B) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: f(std::integral_constant<int, 5>{}); break;
    }
}

// Dispatch only: which kernel, and whether it needs P.needle_dev or scans for NUL, is ham_search_route's to say (ham_search_plan.h).
hipError_t hamming_search_launch(const SearchParams &P0, const HamSearchRoute &R, hipStream_t s, uint32_t *nul_flag) {
    SearchParams P = P0;
    const uint32_t n = P.needle_len;
    char name[64];
    ham_search_kernel_name(R, name, sizeof(name));
    set_last_kernel_name("%s", name);
    switch (R.kind) {
        case HAM_SEARCH_PHASE:
        case HAM_SEARCH_BITS: {
            P.tile = ham_search_line_tile(P.hay_len);
            const uint64_t lanes = (P.hay_len + P.tile - 1) / P.tile;
            const dim3 grid((uint32_t)((lanes + 511) / 512)), block(512);
            with_planes(R.B, [&](auto b) {
                constexpr int B = decltype(b)::value;
                if (R.kind == HAM_SEARCH_BITS) {
                    hipLaunchKernelGGL(hamming_search_bits_kernel<B>, grid, block, 0, s, P, nul_flag);
                    return;
                }
                const HamPhaseGeom G = ham_phase_geom(R.Q, R.L);
                if (R.Q == 4u) hipLaunchKernelGGL((hamming_search_phase_kernel<4, B>), grid, block, 0, s, P, G, nul_flag);
                else if (R.Q == 2u) hipLaunchKernelGGL((hamming_search_phase_kernel<2, B>), grid, block, 0, s, P, G, nul_flag);
                else hipLaunchKernelGGL((hamming_search_phase_kernel<1, B>), grid, block, 0, s, P, G, nul_flag);
            });
            break;
        }
        case HAM_SEARCH_SWAR16: {
            const uint32_t delta = (uint32_t)((uintptr_t)P.hay & 15u);
            const uint64_t lanes = (P.hay_len + delta + 15) / 16;
            const dim3 grid((uint32_t)((lanes + 255) / 256)), block(256);
            switch (R.NW) {
#define TA_HS(NW) case NW: hipLaunchKernelGGL(hamming_search_swar16_kernel<NW>, grid, block, 0, s, P, delta, nul_flag); break;
                TA_HS(1) TA_HS(2) TA_HS(3) TA_HS(4) TA_HS(5) TA_HS(6) TA_HS(7) TA_HS(8)
                TA_HS(9) TA_HS(10) TA_HS(11) TA_HS(12) TA_HS(13) TA_HS(14) TA_HS(15) TA_HS(16)
#undef TA_HS
            }
            break;
        }
        case HAM_SEARCH_SA: {
            const uint64_t offsets = P.hay_len - n + 1;
            P.tile = ham_search_sa_tile(offsets, n);
            const uint64_t lanes = (offsets + P.tile - 1) / P.tile;
            const dim3 grid((uint32_t)((lanes + 255) / 256)), block(256);
            if (R.NW == 2u) hipLaunchKernelGGL(hamming_search_sa_kernel<2>, grid, block, 0, s, P);
            else if (R.NW == 4u) hipLaunchKernelGGL(hamming_search_sa_kernel<4>, grid, block, 0, s, P);
            else hipLaunchKernelGGL(hamming_search_sa_kernel<8>, grid, block, 0, s, P);
            break;
        }
        case HAM_SEARCH_ROUND1: {
            const uint32_t delta = (uint32_t)((uintptr_t)P.hay & 3u);
            const uint64_t groups = (P.hay_len - n + delta) / 4 + 1;
            hipLaunchKernelGGL(hamming_search_kernel, dim3((uint32_t)((groups + 255) / 256)), dim3(256), 0, s, P, delta);
            break;
        }
    }
    return hipGetLastError();
}

}  // namespace ta
