// emu_tab_depth.cpp -- host emulation driver of the table form of the band kernel (lev_bits_tab_body.h) at BOTH depths of its LDS
// stream (LevBitsTab's DEPTH: 1 and 2 lookups in flight).  TESTS ONLY, after tests/emu_tab: wavefronts of 64 emulated lanes run the body
// over a fixed-length batch, and in front of every 16th column a probe rebuilds the nibble tables from the window's rows and compares them
// with the incrementally kept ones -- at a span's end the tables must hold exactly the rows below it, however far the stream ran ahead
// inside the span.  With EMU_TAB_DEPTH_MAIN the file is a program of its own (the sanitizer build): it makes its batches itself and checks
// the answers against a plain scalar recurrence.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "emu_tab_ops.h"
#include "emu_wave.h"
#include "lev_bits_tab_body.h"
#include "lev_plan.h"

using namespace ta;

static uint64_t g_blocks = 0, g_bad_words = 0;
static int g_raw_reads = 0;         // 1 (the sanitizer program): global loads read memory as it is; 0 (the library): bytes outside the blobs read as 0xA5

// (tests/emu_tab/emu_tab.cpp, TabProbe: the rows of iterations tb - 32 .. tb - 1 are byte t & 3 of F[(t >> 2) & 7], in slot t & 31)
struct TabProbe {
    static void block(const uint8_t *lds, const V32 (&F)[8], uint32_t tb) {
        g_blocks++;
        for (int lane = 0; lane < 64; lane++) {
            uint32_t tl[16] = {0}, th[16] = {0};
            for (uint32_t t = tb - 32u; t != tb; t++) {
                const uint32_t byte = (F[(t >> 2) & 7u].v[lane] >> (8u * (t & 3u))) & 0xFFu;
                tl[byte & 15u] |= 1u << (t & 31u);
                th[byte >> 4] |= 1u << (t & 31u);
            }
            for (uint32_t v = 0; v < 16u; v++) {
                uint32_t got_l, got_h;
                memcpy(&got_l, lds + 256u * v + 4u * (uint32_t)lane, 4);
                memcpy(&got_h, lds + 4096u + 256u * v + 4u * (uint32_t)lane, 4);
                if (got_l != tl[v]) g_bad_words++;
                if (got_h != th[v]) g_bad_words++;
            }
        }
    }
};

// A fixed-length batch of n pairs under unit costs at depth 1 or 2.  probe_out[0] = blocks checked, probe_out[1] = table words that
// differed.  0: ran; 1: outside the table form's domain; 2: no such depth.
extern "C" int emu_lev_bits_tab_depth(const uint8_t *a_blob, uint64_t a_len, const uint8_t *b_blob, uint64_t b_len, uint32_t n, uint32_t k,
                                      uint32_t depth, uint32_t *out, uint64_t *probe_out) {
    const uint64_t max_len = a_len > b_len ? a_len : b_len;
    if (depth != 1u && depth != 2u) return 2;
    const LevBitsPlan pl = lev_bits_make_plan(k, 1, 1, 0, false, 0, max_len);
    if (!lev_bits_tab_in_domain(pl, false, true, max_len)) return 1;
    LevParams P;
    P.a = StrView{a_blob, nullptr, a_len, a_len};
    P.b = StrView{b_blob, nullptr, b_len, b_len};
    P.subset = nullptr; P.trace = nullptr; P.out = out; P.n = n; P.k = k;
    P.mc = 1; P.gc = 1; P.sg = 0; P.tc = 0;
    P.u = pl.u; P.o = 0; P.L = 1; P.PW = 64; P.lds_per_wave = LEV_TAB_LDS_PER_WAVE; P.Tw = pl.Tw; P.ch = pl.ch;
    g_blocks = 0; g_bad_words = 0;
    struct RangeGuard { ~RangeGuard() { EmuWave::clear_ranges(); } } range_guard;
    EmuWave::clear_ranges();
    if (!g_raw_reads) {
        EmuWave::add_range(a_blob, (uint64_t)n * a_len);
        EmuWave::add_range(b_blob, (uint64_t)n * b_len);
    }
    uint8_t *lds = (uint8_t *)malloc(LEV_TAB_LDS_PER_WAVE);
    for (uint32_t w = 0; w < (n + 63u) / 64u; w++) {
        memset(lds, 0xA5, LEV_TAB_LDS_PER_WAVE);             // LDS starts out as garbage on the device
        if (depth == 1u) LevBitsTab<EmuWave, EmuTab, TabProbe, 1>::run(P, w, lds);
        else LevBitsTab<EmuWave, EmuTab, TabProbe, 2>::run(P, w, lds);
    }
    free(lds);
    if (probe_out) { probe_out[0] = g_blocks; probe_out[1] = g_bad_words; }
    return 0;
}

#ifdef EMU_TAB_DEPTH_MAIN
static uint32_t lev_scalar(const uint8_t *a, size_t n, const uint8_t *b, size_t m) {
    std::vector<uint32_t> row(m + 1);
    for (size_t j = 0; j <= m; j++) row[j] = (uint32_t)j;
    for (size_t i = 1; i <= n; i++) {
        uint32_t diag = row[0];
        row[0] = (uint32_t)i;
        for (size_t j = 1; j <= m; j++) {
            const uint32_t sub = diag + (a[i - 1] != b[j - 1] ? 1u : 0u), del = row[j] + 1u, ins = row[j - 1] + 1u;
            diag = row[j];
            row[j] = sub < del ? (sub < ins ? sub : ins) : (del < ins ? del : ins);
        }
    }
    return row[m];
}

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (uint32_t)(g_seed >> 32); }

// the shapes of tests/tab_depth_cases.py: column counts whose last span is a tail of 1, 2, 3, 15 or 16 columns in either phase, or full
// spans only; `a` as long as `b`, 6 shorter, 5 longer (the window starts at a piece's edge or inside one); 24 and 32 diagonals a side
int main() {
    static const uint32_t blens[] = {129, 130, 131, 143, 144, 145, 146, 160, 161, 175, 176, 177, 255, 256};
    static const int32_t dlen[] = {0, -6, 5};
    static const uint32_t ks[] = {24, 32};
    const uint32_t n = 101;
    int failures = 0;
    uint64_t checks = 0, within = 0, total = 0;
    g_raw_reads = 1;
    for (uint32_t lb : blens) for (int32_t dl : dlen) for (uint32_t k : ks) {
        const uint32_t la = (uint32_t)((int32_t)lb + dl);
        if (la <= 128u) continue;
        // blobs with the API's 16 bytes of read slack and not a byte more: a read beyond is the sanitizer's to report
        std::vector<uint8_t> a((size_t)n * la + 16, 0xA5), b((size_t)n * lb + 16, 0xA5);
        for (uint32_t i = 0; i < n; i++) {
            uint8_t *pa = &a[(size_t)i * la], *pb = &b[(size_t)i * lb];
            for (uint32_t x = 0; x < la; x++) pa[x] = (uint8_t)(33u + rnd() % 94u);
            // b = a shifted by 0..3 places with 10..17 substitutions (every fifth pair: unrelated)
            const uint32_t shift = rnd() % 4u, subs = 10u + rnd() % 8u;
            for (uint32_t x = 0; x < lb; x++) pb[x] = (i % 5u == 4u || x + shift >= la) ? (uint8_t)(33u + rnd() % 94u) : pa[x + shift];
            for (uint32_t s = 0; s < subs; s++) pb[rnd() % lb] = (uint8_t)(33u + rnd() % 94u);
        }
        std::vector<uint32_t> want(n);
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t d = lev_scalar(&a[(size_t)i * la], la, &b[(size_t)i * lb], lb);
            want[i] = d <= k ? d : 0xFFFFFFFFu;
            total++;
            if (want[i] != 0xFFFFFFFFu) within++;
        }
        for (uint32_t depth = 1; depth <= 2; depth++) {
            std::vector<uint32_t> out(n, 0x12345678u);
            uint64_t probe[2] = {0, 0};
            const int rc = emu_lev_bits_tab_depth(a.data(), la, b.data(), lb, n, k, depth, out.data(), probe);
            if (rc != 0) { printf("FAIL rc=%d at %u x %u k=%u depth %u\n", rc, la, lb, k, depth); failures++; continue; }
            if (probe[0] != 2u * ((lb + 15u) / 16u) || probe[1] != 0) {
                printf("FAIL tables at %u x %u k=%u depth %u: %llu blocks, %llu words differ\n", la, lb, k, depth, (unsigned long long)probe[0], (unsigned long long)probe[1]);
                failures++;
            }
            checks += probe[0];
            for (uint32_t i = 0; i < n; i++)
                if (out[i] != want[i]) { if (failures < 20) printf("FAIL %u x %u k=%u depth %u pair %u: got %u want %u\n", la, lb, k, depth, i, out[i], want[i]); failures++; }
        }
    }
    printf("%llu answers per depth, %llu within k, %llu table checks\n", (unsigned long long)total, (unsigned long long)within, (unsigned long long)checks);
    printf(failures ? "emu_tab_depth: %d FAILURES\n" : "emu_tab_depth: ok\n", failures);
    return failures ? 1 : 0;
}
#endif
