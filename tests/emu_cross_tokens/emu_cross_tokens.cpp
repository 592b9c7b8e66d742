// emu_cross_tokens.cpp -- host emulation driver of the token cross body (lev_cross_tok_body.h).  TESTS ONLY: a wavefront of 64 emulated
// lanes runs the body for ONE query of 32-bit tokens against up to 64 targets, as one step of lev_cross_tok_kernel's query loop does.
#include <stdint.h>
#include <string.h>

#include "emu_wave.h"
#include "lev_cross_tok_body.h"

using namespace ta;

// The wavefront's hash table, one per NW, kept ACROSS calls as the kernel keeps it across the queries of its tile: zeroed once, every
// query has to leave it zero again.
static uint8_t g_lds[2][LevCrossTok<EmuWave, 2, false>::LDS_BYTES];
static bool g_cleared[2] = {false, false};

template <int NW, bool TRANS>
static int run(const uint32_t *q, uint32_t m, const uint32_t *tdata, const uint64_t *toff, uint32_t nt, uint32_t k, uint32_t *res, uint32_t *skip) {
    using B = LevCrossTok<EmuWave, NW, TRANS>;
    static_assert(B::LDS_BYTES <= sizeof(g_lds[0]), "table size");
    uint8_t *lds = g_lds[NW - 1];
    if (!g_cleared[NW - 1]) { B::clear(lds); g_cleared[NW - 1] = true; }
    const V32 lane = EmuWave::lane();
    const VB live = lane < V32(nt);
    VP tp;
    V32 tl;
    for (uint32_t i = 0; i < 64; i++) {                          // lane i's target: element offsets, as the kernel's walk reads them
        tp.v[i] = (const uint8_t *)(tdata + (i < nt ? toff[i] : 0));
        tl.v[i] = i < nt ? (uint32_t)(toff[i + 1] - toff[i]) : 0u;
    }
    const auto first = B::first_piece(tp, tl, live);
    V32 r;
    VB s;
    const bool ran = B::query(lds, q, m, tp, tl, live, first, k, r, s);
    for (int i = 0; i < 64; i++) { res[i] = r.v[i]; skip[i] = s.v[i] ? 1u : 0u; }
    return ran ? 1 : 0;
}

// One query q[0 .. m) against targets tdata[toff[i] .. toff[i + 1]), i < nt <= 64 (ELEMENT offsets; nothing outside the items is read).
// res[64]: the distance, 0xFFFFFFFF for None and for the lanes at and above nt; skip[64]: 1 where the length prefilter answered.
// Returns 1 when the body ran the query, 0 when the prefilter answered every live lane (no table, no column), -1 for bad arguments.
extern "C" int emu_cross_tok_query(const uint32_t *q, uint32_t m, const uint32_t *tdata, const uint64_t *toff, uint32_t nt, uint32_t k, int nw,
                                   int trans, uint32_t *res, uint32_t *skip) {
    if (nt > 64 || (nw != 1 && nw != 2) || m > 32u * (uint32_t)nw) return -1;
    if (nw == 1) return trans ? run<1, true>(q, m, tdata, toff, nt, k, res, skip) : run<1, false>(q, m, tdata, toff, nt, k, res, skip);
    return trans ? run<2, true>(q, m, tdata, toff, nt, k, res, skip) : run<2, false>(q, m, tdata, toff, nt, k, res, skip);
}

// 1 when the table of that NW is all zero (as every query must leave it)
extern "C" int emu_cross_tok_table_clean(int nw) {
    if (nw != 1 && nw != 2) return -1;
    const uint32_t bytes = nw == 1 ? LevCrossTok<EmuWave, 1, false>::LDS_BYTES : LevCrossTok<EmuWave, 2, false>::LDS_BYTES;
    for (uint32_t i = 0; i < bytes; i++) if (g_lds[nw - 1][i]) return 0;
    return 1;
}

// the slot at which the probe of each of n tokens starts, and the number of slots (the same for both NW)
extern "C" uint32_t emu_cross_tok_slots(void) { return LevCrossTok<EmuWave, 1, false>::H; }
extern "C" void emu_cross_tok_home(const uint32_t *x, uint32_t n, uint32_t *out) {
    for (uint32_t i = 0; i < n; i++) out[i] = LevCrossTok<EmuWave, 1, false>::home(V32(x[i])).v[0];
}
