// emu_tab.cpp -- host emulation driver of the table form of the band kernel (lev_bits_tab_body.h).  TESTS ONLY: wavefronts of 64 emulated
// lanes run the body over a fixed-length batch as lev_bits_tab_kernel does, with a probe that rebuilds the nibble tables from the window's
// rows in front of every 16th column and compares them with the incrementally kept ones.  With EMU_TAB_MAIN the file is a program of its
// own (the sanitizer build): it makes its batches itself and checks the answers against a plain scalar recurrence.
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
// 1 (the sanitizer program): global loads read memory as it is -- the blobs carry the API's 16 bytes of read slack and a read beyond that
// is the sanitizer's to report.  0 (the library, called from Python): bytes outside the blobs read as 0xA5 without touching memory.
static int g_raw_reads = 0;

// in front of the column of iteration tb the window's rows are the bytes of iterations tb - 32 .. tb - 1: byte t & 3 of F[(t >> 2) & 7],
// in slot t & 31.  The tables rebuilt from them must be the tables in LDS, word for word, in every lane.
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

// A fixed-length batch of n pairs (a_len / b_len bytes per string, packed) under EditCosts(g, g, 0, None), g >= 1: the unit-cost pass with
// k / g and the answers times g, as the library's pass does for the multiples of the unit costs.  Bytes outside the blobs read as 0xA5
// (the device reads up to 15 bytes past a string's last 16-byte piece; what they hold must not matter).
// probe_out[0] = blocks checked, probe_out[1] = table words that differed.  0: ran; 1: outside the table form's domain.
extern "C" int emu_lev_bits_tab(const uint8_t *a_blob, uint64_t a_len, const uint8_t *b_blob, uint64_t b_len, uint32_t n, uint32_t k,
                                uint32_t g, uint32_t *out, uint64_t *probe_out) {
    const uint64_t max_len = a_len > b_len ? a_len : b_len;
    if (g == 0 || (g > 1 && lev_unit_scale(g, g, 0, false, 0) != g)) return 1;
    const uint32_t ku = k / g;
    const LevBitsPlan pl = lev_bits_make_plan(ku, 1, 1, 0, false, 0, max_len);
    if (!lev_bits_tab_in_domain(pl, false, true, max_len)) return 1;
    LevParams P;
    P.a = StrView{a_blob, nullptr, a_len, a_len};
    P.b = StrView{b_blob, nullptr, b_len, b_len};
    P.subset = nullptr; P.trace = nullptr; P.out = out; P.n = n; P.k = ku;
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
        LevBitsTab<EmuWave, EmuTab, TabProbe>::run(P, w, lds);
    }
    free(lds);
    if (g > 1) for (uint32_t i = 0; i < n; i++) if (out[i] != 0xFFFFFFFFu) out[i] *= g;
    if (probe_out) { probe_out[0] = g_blocks; probe_out[1] = g_bad_words; }
    return 0;
}

#ifdef EMU_TAB_MAIN
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

int main() {
    static const uint8_t A0[] = {0x00}, A1[] = {0x0C, 0x0D}, A2[] = {0x11, 0x12, 0x21, 0x22}, A3[] = {0x0F, 0xF0, 0xFF, 0x00};
    struct Alpha { const uint8_t *s; uint32_t n; } alphas[] = {{A0, 1}, {A1, 2}, {A2, 4}, {A3, 4}, {nullptr, 256}};
    struct Geo { uint32_t la, lb, k, g, n; } geos[] = {{129, 129, 32, 1, 65}, {160, 160, 32, 1, 209}, {256, 256, 32, 1, 64}, {256, 250, 32, 1, 65}, {257, 257, 32, 1, 1}, {288, 256, 32, 1, 63},
                                                       {256, 288, 32, 1, 65}, {250, 256, 32, 1, 65}, {256, 224, 32, 1, 65}, {256, 256, 24, 1, 65},
                                                       {256, 256, 25, 1, 65}, {256, 256, 31, 1, 65}, {256, 256, 64, 2, 65}};
    int failures = 0;
    for (const Geo &ge : geos) {
        // blobs with the 16 bytes of read slack the API asks for (a string's last 16-byte piece is loaded whole) and not a byte more; the
        // loads go to memory unchecked by the emulation, so a read past the slack or in front of a blob is the sanitizer's to report
        g_raw_reads = 1;
        std::vector<uint8_t> a((size_t)ge.n * ge.la + 16, 0xA5), b((size_t)ge.n * ge.lb + 16, 0xA5);
        for (uint32_t i = 0; i < ge.n; i++) {
            const Alpha &al = alphas[i % 5u];
            auto sym = [&]() -> uint8_t { return al.s ? al.s[rnd() % al.n] : (uint8_t)rnd(); };
            uint8_t *pa = &a[(size_t)i * ge.la], *pb = &b[(size_t)i * ge.lb];
            for (uint32_t x = 0; x < ge.la; x++) pa[x] = sym();
            // b = a shifted by 0..3 places with some substitutions (every third pair: unrelated)
            const uint32_t shift = rnd() % 4u, subs = rnd() % (ge.k / ge.g + 2u);
            for (uint32_t x = 0; x < ge.lb; x++) pb[x] = (i % 3u == 2u || x + shift >= ge.la) ? sym() : pa[x + shift];
            for (uint32_t s = 0; s < subs; s++) pb[rnd() % ge.lb] = sym();
        }
        std::vector<uint32_t> out(ge.n, 0x12345678u);
        uint64_t probe[2] = {0, 0};
        const int rc = emu_lev_bits_tab(a.data(), ge.la, b.data(), ge.lb, ge.n, ge.k, ge.g, out.data(), probe);
        if (rc != 0) { printf("FAIL rc=%d at %u x %u\n", rc, ge.la, ge.lb); failures++; continue; }
        if (probe[0] == 0 || probe[1] != 0) { printf("FAIL tables: %llu blocks, %llu words differ\n", (unsigned long long)probe[0], (unsigned long long)probe[1]); failures++; }
        uint32_t some = 0;
        for (uint32_t i = 0; i < ge.n; i++) {
            const uint32_t d = lev_scalar(&a[(size_t)i * ge.la], ge.la, &b[(size_t)i * ge.lb], ge.lb) * ge.g;
            const uint32_t want = d <= ge.k ? d : 0xFFFFFFFFu;
            if (want != 0xFFFFFFFFu) some++;
            if (out[i] != want) { if (failures < 20) printf("FAIL %u x %u k=%u g=%u pair %u: got %u want %u\n", ge.la, ge.lb, ge.k, ge.g, i, out[i], want); failures++; }
        }
        printf("%u x %u k=%u g=%u n=%u: %u within k, %llu table checks\n", ge.la, ge.lb, ge.k, ge.g, ge.n, some, (unsigned long long)probe[0]);
    }
    printf(failures ? "emu_tab: %d FAILURES\n" : "emu_tab: ok\n", failures);
    return failures ? 1 : 0;
}
#endif
