// emu_hsearch_cross_w2.cpp -- host emulation driver of the two-word Hamming search cross body (ham_search_cross_w2_body.h,
// ham_bits2_body.h).  TESTS ONLY: the whole call as the kernel of ham_search_cross_w2.hip runs it -- per workgroup the 512-thread build of
// the [256][32] table of two-word entries (lanes l and l + 32 one column, a word each), per wavefront 64 emulated lanes at every group
// size with 64 / G >= 2 haystacks per step and a ragged last step, the per-wavefront stage filled in ballot order and its flushes, the
// per-haystack count with its NUL mark, the packed minimum word and the finish pass.  The emulation takes the two-word route for every
// panel of needles up to 64 bytes (the library routes a panel of needles up to 32 bytes to the one-word kernel): a short needle's low
// words must stay zero, which the lanes check.  Plus the counters alone against a caller's byte loop (emu_ham_bits2_windows).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "emu_wave.h"
#include "ham_search_cross_w2_body.h"

using namespace ta;

namespace {

struct Side {
    const uint8_t *blob;
    const uint64_t *off;
    const uint8_t *ptr(uint32_t i) const { return blob + off[i]; }
    uint64_t len(uint32_t i) const { return off[i + 1] - off[i]; }
};

struct Call {
    Side nd, hs;
    uint32_t nn, nh, kc, hpw;
    ta_search_cross_hit *hits;
    uint64_t *count, cap;
    uint64_t *packed;
    uint32_t *per_haystack, *seen;
    uint32_t max_steps, flushes;
};

// the lane's read: both words of its column of row (byte b of w), as the one 8-byte read at byte c * 256 + column * 8
template <int B>
void scan_lane(const uint8_t *hay, uint32_t h, const uint32_t *mis, uint32_t column, uint32_t n, uint32_t kc, HsxBest &r, bool &lo_dirty) {
    hsx2_scan_pair<B>(hay, h, [&](uint32_t w, int b) {
        const uint32_t a = (((w >> (8 * b)) & 0xFFu) << 8) | (column * 8u);
        HamBits2Word m;
        memcpy(&m, (const uint8_t *)mis + a, 8);
        if (n <= 32u && m.lo) lo_dirty = true;
        return m;
    }, n, kc, [](bool p) { return p; }, r);
}

// a wavefront's stage goes out: one add to the counter, the records behind it below cap
void flush(Call &c, const ta_search_cross_hit *stage, uint32_t cnt) {
    const uint64_t base = *c.count;
    *c.count += cnt;
    c.flushes++;
    for (uint32_t lane = 0; lane < cnt; lane++)
        if (base + lane < c.cap) c.hits[base + lane] = stage[lane];
}

// one workgroup: blockIdx = (bx, group).  Returns 0, or what went wrong.
int workgroup(Call &c, int planes, uint32_t bx, uint32_t group) {
    static uint32_t mis[256 * HSX2_GROUP * 2];
    const uint32_t g0 = group * HSX2_GROUP, size = hsx2_group_size(c.nn, group), G = sx_group_cols(size), S = 64u / G;
    if (G < size || G > HSX2_GROUP || (G & (G - 1)) || (G > 1 && G / 2 >= size) || S < 2) return 10;
    const uint8_t *np[64];
    uint32_t n[64];
    bool has[64], scans[64];
    for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t col = lane & (G - 1);
        has[lane] = col < size;
        np[lane] = has[lane] ? c.nd.ptr(g0 + col) : nullptr;
        const uint64_t nl = has[lane] ? c.nd.len(g0 + col) : 0;
        n[lane] = nl < HSX2_MAX_NEEDLE + 1u ? (uint32_t)nl : HSX2_MAX_NEEDLE + 1u;
        scans[lane] = has[lane] && hsx2_scans(n[lane]);
    }
    // the table, thread by thread as the kernel fills it: "every position mismatches", (barrier), the needles' bytes clear their bits
    memset(mis, 0xA5, sizeof mis);
    for (uint32_t wave = 0; wave < SX_WAVES; wave++)
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t column = lane & (HSX2_GROUP - 1), half = lane >> 5;
            for (uint32_t ch = wave * 32; ch < wave * 32 + 32; ch++) mis[hsx2_mis_at(ch, column, half)] = scans[lane] ? hsx2_mis_full(n[lane], half) : 0u;
        }
    for (uint32_t wave = 0; wave < SX_WAVES; wave++)
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t column = lane & (HSX2_GROUP - 1), half = lane >> 5;
            if (scans[lane])
                for (uint32_t j = wave * 2u + half; j < n[lane]; j += 2u * SX_WAVES) {
                    uint32_t w;
                    const uint32_t bit = hsx2_mis_bit(n[lane], j, w);
                    mis[hsx2_mis_at((uint32_t)np[lane][j], column, w)] &= ~bit;
                }
        }
    for (uint32_t lane = 0; lane < 64; lane++) {                  // column l mod 32 = ham_bits2_mis of lane l's needle, row by row
        const uint32_t column = lane & (HSX2_GROUP - 1);
        for (uint32_t ch = 0; ch < 256; ch++) {
            HamBits2Word want = {0u, 0u};
            if (scans[lane]) want = ham_bits2_mis(np[lane], n[lane], ch);
            if (mis[hsx2_mis_at(ch, column, 0)] != want.lo || mis[hsx2_mis_at(ch, column, 1)] != want.hi) return 11;
        }
    }

    const uint64_t wg0 = (uint64_t)bx * c.hpw, wg1 = wg0 + c.hpw < c.nh ? wg0 + c.hpw : c.nh;
    for (uint32_t wave = 0; wave < SX_WAVES; wave++) {
        ta_search_cross_hit stage[HSX_STAGE];                     // the wavefront's staged records
        uint32_t staged = 0;
        for (uint32_t it = 0;; it++) {
            if (wg0 + sx_local_hay(it, wave, S, 0) >= wg1) break;
            if (it + 1 > c.max_steps) c.max_steps = it + 1;
            HsxBest r[64];
            bool live[64], hit[64];
            uint32_t n_hit = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint64_t hi = wg0 + sx_local_hay(it, wave, S, lane / G);
                r[lane] = HsxBest{TA_NONE, 0u, 0u, false};
                live[lane] = false;
                if (has[lane] && hi < wg1 && c.seen) {
                    uint32_t &s = c.seen[(uint64_t)hi * c.nn + g0 + (lane & (G - 1))];
                    if (s) return 12;                             // a pair the scan meets twice
                    s = 1;
                }
                if (scans[lane] && hi < wg1) {
                    const uint8_t *hay = c.hs.ptr((uint32_t)hi);
                    const uint64_t h = c.hs.len((uint32_t)hi);
                    live[lane] = (uint64_t)n[lane] <= h;
                    if (live[lane]) {
                        const uint32_t column = lane & (HSX2_GROUP - 1);
                        bool lo_dirty = false;
                        switch (planes) {
                            case 1: scan_lane<1>(hay, (uint32_t)h, mis, column, n[lane], c.kc, r[lane], lo_dirty); break;
                            case 2: scan_lane<2>(hay, (uint32_t)h, mis, column, n[lane], c.kc, r[lane], lo_dirty); break;
                            case 3: scan_lane<3>(hay, (uint32_t)h, mis, column, n[lane], c.kc, r[lane], lo_dirty); break;
                            case 4: scan_lane<4>(hay, (uint32_t)h, mis, column, n[lane], c.kc, r[lane], lo_dirty); break;
                            case 5: scan_lane<5>(hay, (uint32_t)h, mis, column, n[lane], c.kc, r[lane], lo_dirty); break;
                            case 6: scan_lane<6>(hay, (uint32_t)h, mis, column, n[lane], c.kc, r[lane], lo_dirty); break;
                            case 7: scan_lane<7>(hay, (uint32_t)h, mis, column, n[lane], c.kc, r[lane], lo_dirty); break;
                            default: return 13;
                        }
                        if (lo_dirty) return 17;                  // a needle of up to 32 bytes with a bit in its low word
                    }
                }
                hit[lane] = live[lane] && !r[lane].nul && r[lane].count != 0u;
                if (live[lane] && r[lane].nul && c.per_haystack) c.per_haystack[hi] = TA_NONE;
                n_hit += hit[lane];
            }
            if (!n_hit) continue;
            if (staged + n_hit > HSX_STAGE) { flush(c, stage, staged); staged = 0; }
            for (uint32_t lane = 0; lane < 64; lane++) {          // (lane order = the ballot's prefix order)
                if (!hit[lane]) continue;
                const uint32_t hi = (uint32_t)(wg0 + sx_local_hay(it, wave, S, lane / G)), needle = g0 + (lane & (G - 1));
                if (r[lane].d > c.kc || r[lane].d > 64u) return 14;
                if (staged >= HSX_STAGE) return 16;                                  // the stage overflows
                stage[staged++] = ta_search_cross_hit{hi, needle, r[lane].start, r[lane].start + n[lane], r[lane].d, r[lane].count};
                if (c.per_haystack) {
                    if (c.per_haystack[hi] == TA_NONE) return 15;                    // a hit in a haystack marked NUL
                    c.per_haystack[hi]++;
                }
                const uint64_t w = hsx_word(r[lane].d, needle, r[lane].start);
                if (c.packed && w < c.packed[hi]) c.packed[hi] = w;
            }
        }
        if (staged) flush(c, stage, staged);
    }
    return 0;
}

template <int B>
void windows(const uint8_t *needle, uint32_t n, const uint8_t *hay, uint32_t h, uint32_t k, uint8_t *over, uint32_t *count) {
    HamBits2State<B> st;
    ham_bits2_reset<B>(st, n);
    HamBits2Word bias[B];
    ham_bits2_bias<B>(k, n, bias);
    const uint32_t base = ((1u << B) - 1u) - k;
    for (uint32_t i = 0; i < h; i++) {
        const uint32_t ov = ham_bits2_step<B>(st, ham_bits2_mis(needle, n, hay[i]), bias);
        uint32_t top[B];
        ham_bits2_top<B>(st, top);
        over[i] = (uint8_t)(ov >> 31);
        count[i] = ham_bits2_count<B>(top) - base;
    }
}

}  // namespace

// The counters alone: for every byte i of the haystack, over[i] = bit 63 of OV after the byte (1 also while fewer than n bytes have
// been consumed) and count[i] = the planes' counter minus the bias (meaningful where over[i] = 0).  Returns the plane count taken.
extern "C" int emu_ham_bits2_windows(const uint8_t *needle, uint32_t n, const uint8_t *hay, uint32_t h, uint32_t k, uint8_t *over, uint32_t *count) {
    const int B = ham_bits2_planes(k);
    switch (B) {
        case 1: windows<1>(needle, n, hay, h, k, over, count); break;
        case 2: windows<2>(needle, n, hay, h, k, over, count); break;
        case 3: windows<3>(needle, n, hay, h, k, over, count); break;
        case 4: windows<4>(needle, n, hay, h, k, over, count); break;
        case 5: windows<5>(needle, n, hay, h, k, over, count); break;
        case 6: windows<6>(needle, n, hay, h, k, over, count); break;
        case 7: windows<7>(needle, n, hay, h, k, over, count); break;
        default: return 0;
    }
    return B;
}

// The whole call over CSR sides (n + 1 offsets each).  forced_hpw: TA_HSEARCH_CROSS_HPW, 0 = the plan's.  nearest / best / per_haystack:
// nh entries or NULL.  seen: nn nh words preset to zero -- [i nn + p] = 1 once the scan has met the pair -- or NULL.  *planes: the plane
// count taken, *max_steps: the most steps a wavefront walked.  Returns 0, or a code that names what the emulation caught.
extern "C" int emu_hsearch_cross_w2(const uint8_t *nblob, const uint64_t *noff, uint32_t nn, const uint8_t *hblob, const uint64_t *hoff, uint32_t nh,
                                    uint32_t k, uint32_t forced_hpw, ta_search_cross_hit *hits, uint64_t *count, uint64_t cap, uint64_t *nearest,
                                    ta_match *best, uint32_t *per_haystack, uint32_t *seen, uint32_t *planes, uint32_t *max_steps) {
    Call c;
    c.nd = Side{nblob, noff}; c.hs = Side{hblob, hoff};
    c.nn = nn; c.nh = nh;
    c.hits = hits; c.count = count; c.cap = cap; c.per_haystack = per_haystack; c.seen = seen;
    c.max_steps = 0; c.flushes = 0;
    *count = 0;
    *planes = 0;
    *max_steps = 0;
    for (uint32_t i = 0; i < nh; i++)
        if (per_haystack) per_haystack[i] = 0;
    if (nn == 0 || nh == 0) {
        for (uint32_t i = 0; i < nh; i++) {
            if (nearest) nearest[i] = ~0ull;
            if (best) best[i] = ta_match{0, 0, TA_NONE, 0u};
        }
        return 0;
    }
    uint32_t max_needle = 0;
    for (uint32_t p = 0; p < nn; p++)
        if (c.nd.len(p) > max_needle) max_needle = (uint32_t)c.nd.len(p);
    if (max_needle > HSX2_MAX_NEEDLE) return 1;
    c.kc = hsx_threshold(k, max_needle);
    const int B = hsx2_planes(c.kc);
    if (B < 1 || B > 7 || ((1u << B) - 1u) < c.kc || (B > 1 && ((1u << (B - 1)) - 1u) >= c.kc)) return 2;
    *planes = (uint32_t)B;
    std::vector<uint64_t> packed;
    if (nearest || best) packed.assign(nh, ~0ull);
    c.packed = packed.empty() ? nullptr : packed.data();
    c.hpw = hsx2_hpw(nn, nh, forced_hpw);
    if (c.hpw == 0 || c.hpw > nh) return 3;
    const uint32_t groups = (nn + HSX2_GROUP - 1) / HSX2_GROUP, gx = (nh + c.hpw - 1) / c.hpw;
    for (uint32_t group = 0; group < groups; group++)
        for (uint32_t bx = 0; bx < gx; bx++)
            if (const int rc = workgroup(c, B, bx, group)) return rc;
    *max_steps = c.max_steps;
    if (c.packed)                                                 // the finish kernel: one lane per haystack
        for (uint32_t i = 0; i < nh; i++) {
            const uint64_t w = c.packed[i];
            if (nearest) nearest[i] = hsx_nearest(w);
            if (best) best[i] = hsx_best(w, w == ~0ull ? 0u : (uint32_t)c.nd.len(hsx_word_needle(w)));
        }
    return 0;
}
