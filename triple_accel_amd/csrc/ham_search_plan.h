// ham_search_plan.h -- which kernel a single-haystack hamming_search takes, as a pure rule (ham_search.hip dispatches on it, ta_search.hip
// uploads the needle by it; tests/cpp/ham_route_check.cpp checks it with plain g++), and the tiles of the lane-per-tile forms.
#pragma once
#include <stdio.h>

#include "ham_phase_body.h"

namespace ta {

enum HamSearchKind : uint32_t {
    HAM_SEARCH_PHASE,        // hamming_search_phase_kernel<Q, B>: bit-sliced counters over a subset of the positions (ham_phase_body.h)
    HAM_SEARCH_BITS,         // hamming_search_bits_kernel<B>: bit-sliced counters over every position (ham_bits_body.h)
    HAM_SEARCH_SWAR16,       // hamming_search_swar16_kernel<NW>: 16 offsets per lane (ham_swar_body.h)
    HAM_SEARCH_SA,           // hamming_search_sa_kernel<NW>: the shift-add scan (ham_search_body.h)
    HAM_SEARCH_ROUND1,       // hamming_search_kernel: 4 offsets per lane, any needle length
};

// the A/B switches (TA_HAMMING_SEARCH_SWAR, _SA, _NO_BITS, _NO_PHASE, TA_HAMMING_PHASE_Q), read by the caller: all clear without TA_TUNING
struct HamSearchSwitches {
    bool swar, sa, no_bits, no_phase;
    uint32_t phase_q;        // tests: 1 or 2 forces fewer phases where the plan has more
};

struct HamSearchRoute {
    HamSearchKind kind;
    uint32_t Q, L;           // phase: phases per dword, positions counted per phase
    int B;                   // phase, bits: counter planes
    uint32_t NW;             // swar16: needle dwords; shift-add: dwords of the state (2, 4 or 8)
    bool needs_needle_dev;   // the kernel reads SearchParams::needle_dev (the others: the kernarg copy)
    bool scans_nul;          // the kernel reads every haystack byte and checks it for NUL on the way
};

// 1 <= n <= hay_len.  phase: where the subset is selective for k and, up to 64 bytes, costs fewer instructions per byte than swar16's 3 per
// needle dword + 4; bits: 9..32 bytes whose k needs few planes, 3 B + 3 per byte against swar16's 3 per needle dword + 1
TA_HD inline HamSearchRoute ham_search_route(uint32_t n, uint32_t k, const HamSearchSwitches &sw) {
    HamSearchRoute r{};
    const uint32_t nw = (n + 3u) / 4u;
    const bool ab = sw.swar || sw.sa || sw.no_bits;
    uint32_t Q = 0, L = 0; int B = 0;
    if (!ab && !sw.no_phase && ham_phase_plan(n, k, Q, L, B) && (n > 64u || ham_phase_cost_x4(Q, B) < 4u * (3u * nw + 4u))) {
        if ((sw.phase_q == 1u || sw.phase_q == 2u) && sw.phase_q < Q) {
            Q = sw.phase_q;
            L = (n + Q - 1u) / Q;
            if (L > 32u / Q) L = 32u / Q;
        }
        r.kind = HAM_SEARCH_PHASE; r.Q = Q; r.L = L; r.B = B;
        r.needs_needle_dev = n > 64u; r.scans_nul = true;
        return r;
    }
    const int planes = ham_bits_planes(k);
    if (!ab && n >= 9u && n <= 32u && planes && k < n && 3 * planes + 3 < 3 * (int)nw + 1) {
        r.kind = HAM_SEARCH_BITS; r.B = planes; r.scans_nul = true;
    } else if (n <= 64u && !sw.swar && !sw.sa) {
        r.kind = HAM_SEARCH_SWAR16; r.NW = nw; r.scans_nul = true;
    } else if (n <= 32u && !sw.swar) {
        r.kind = HAM_SEARCH_SA; r.NW = nw <= 2u ? 2u : nw <= 4u ? 4u : 8u;
    } else {
        r.kind = HAM_SEARCH_ROUND1; r.needs_needle_dev = true;
    }
    return r;
}

// bytes per lane of the phase and bits forms: two sets of resident lanes over the haystack, whole 128-byte lines, at least two of them
TA_HD inline uint32_t ham_search_line_tile(uint64_t hay_len) {
    uint64_t tile = (hay_len + 262143) / 262144;
    tile = (tile + 127) & ~(uint64_t)127;
    if (tile < 256) tile = 256;
    return (uint32_t)(tile > 0x7FFFFF80ull ? 0x7FFFFF80ull : tile);
}
// offsets per lane of the shift-add form (each lane warms up on n - 1 bytes: at least 8 n offsets)
TA_HD inline uint32_t ham_search_sa_tile(uint64_t offsets, uint32_t n) {
    uint64_t tile = (offsets + 262143) / 262144;
    if (tile < 8ull * n) tile = 8ull * n;
    if (tile < 64) tile = 64;
    return (uint32_t)(tile > 0x7FFFFFFFull ? 0x7FFFFFFFull : tile);
}

// the kernel's name as a profiler prints it (ta_last_kernel_name)
inline void ham_search_kernel_name(const HamSearchRoute &r, char *buf, size_t size) {
    switch (r.kind) {
        case HAM_SEARCH_PHASE: snprintf(buf, size, "hamming_search_phase_kernel<%u,%d>", r.Q, r.B); break;
        case HAM_SEARCH_BITS: snprintf(buf, size, "hamming_search_bits_kernel<%d>", r.B); break;
        case HAM_SEARCH_SWAR16: snprintf(buf, size, "hamming_search_swar16_kernel<%u>", r.NW); break;
        case HAM_SEARCH_SA: snprintf(buf, size, "hamming_search_sa_kernel<%u>", r.NW); break;
        default: snprintf(buf, size, "hamming_search_kernel"); break;
    }
}

}  // namespace ta
