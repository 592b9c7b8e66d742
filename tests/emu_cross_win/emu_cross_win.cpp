// emu_cross_win.cpp -- host emulation driver of the window cross body (lev_cross_win_body.h).  TESTS ONLY: a wavefront of 64 emulated
// lanes runs the body for ONE query of up to 256 bytes against up to 64 targets, as one step of lev_cross_win_kernel's query loop does.
#include <stdint.h>
#include <string.h>

#include "emu_wave.h"
#include "lev_cross_win_body.h"

using namespace ta;

// The wavefront's table, kept ACROSS calls as the kernel keeps it across the queries of its tile: zeroed once, every query has to leave
// it zero again.  (Every WW has the same table.)
static uint8_t g_lds[256 * 4 * WIN_ROW_DWORDS];
static bool g_cleared = false;

template <int WW, bool TRANS>
static int run(const uint8_t *q, uint32_t m, const uint8_t *tblob, const uint64_t *toff, uint32_t nt, uint32_t k, uint32_t *res, uint32_t *skip) {
    using B = LevCrossWin<EmuWave, WW, TRANS>;
    static_assert(B::LDS_BYTES == sizeof(g_lds), "table size");
    if (!g_cleared) { B::clear(g_lds); g_cleared = true; }
    const StrView tv = {tblob, toff, 0, 0};
    const V32 lane = EmuWave::lane();
    const VB live = lane < V32(nt);
    VP tp;
    V32 tl;
    EmuWave::load_str(tv, lane, live, tp, tl);
    const auto first = B::first_piece(tp, tl, live);
    V32 r;
    VB s;
    const bool ran = B::query(g_lds, q, m, tp, tl, live, first, k, r, s);
    for (int i = 0; i < 64; i++) { res[i] = r.v[i]; skip[i] = s.v[i] ? 1u : 0u; }
    return ran ? 1 : 0;
}

template <int WW>
static int run_t(int trans, const uint8_t *q, uint32_t m, const uint8_t *tblob, const uint64_t *toff, uint32_t nt, uint32_t k, uint32_t *res, uint32_t *skip) {
    return trans ? run<WW, true>(q, m, tblob, toff, nt, k, res, skip) : run<WW, false>(q, m, tblob, toff, nt, k, res, skip);
}

// the window the entry picks for unit threshold k
extern "C" int emu_cross_win_ww(uint32_t k) { return win_ww(k); }

// One query q[0 .. m) against targets tblob[toff[i] .. toff[i + 1]), i < nt <= 64 (the blob readable 16 bytes past its end), with a
// window of ww blocks (ww >= emu_cross_win_ww(k)).  res[64]: the distance, 0xFFFFFFFF for None and for the lanes at and above nt;
// skip[64]: 1 where the length prefilter answered.  Returns 1 when the body ran the query, 0 when the prefilter answered every live
// lane (no table, no column), -1 for bad arguments.
extern "C" int emu_cross_win_query(const uint8_t *q, uint32_t m, const uint8_t *tblob, const uint64_t *toff, uint32_t nt, uint32_t k, int ww,
                                   int trans, uint32_t *res, uint32_t *skip) {
    if (nt > 64 || m > WIN_MAX_QUERY || ww < win_ww(k)) return -1;
    switch (ww) {
    case 2: return run_t<2>(trans, q, m, tblob, toff, nt, k, res, skip);
    case 3: return run_t<3>(trans, q, m, tblob, toff, nt, k, res, skip);
    case 4: return run_t<4>(trans, q, m, tblob, toff, nt, k, res, skip);
    case 8: return run_t<8>(trans, q, m, tblob, toff, nt, k, res, skip);
    }
    return -1;
}

// 1 when the table is all zero (as every query must leave it)
extern "C" int emu_cross_win_table_clean(void) {
    for (uint32_t i = 0; i < sizeof(g_lds); i++) if (g_lds[i]) return 0;
    return 1;
}
