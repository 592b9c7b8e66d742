// emu_hcross.cpp -- host emulation driver of the Hamming cross body (ham_cross_body.h).  TESTS ONLY: a wavefront of 64 emulated lanes
// loads up to 64 targets, stages ONE chunk of queries through its slice of LDS and compares every query of the chunk with every target,
// as one round of ham_cross_kernel's chunk loop does.
#include <stdint.h>
#include <string.h>

#include "emu_wave.h"
#include "ham_cross_body.h"

using namespace ta;

template <int NW>
static int run(const uint8_t *qblob, const uint64_t *qoff, uint32_t nq, const uint8_t *tblob, const uint64_t *toff, uint32_t nt, uint32_t k8,
               uint32_t *res, uint32_t *ran) {
    using B = HamCross<EmuWave, NW>;
    if (nq > B::CHUNK) return -1;
    uint8_t lds[B::LDS_BYTES];
    memset(lds, 0xA5, sizeof lds);                                 // (what an earlier chunk left behind must not matter)
    const StrView qv = {qblob, qoff, 0, 0}, tv = {tblob, toff, 0, 0};
    const V32 lane = EmuWave::lane();
    const VB live = lane < V32(nt);
    VP tp;
    V32 tl;
    EmuWave::load_str(tv, lane, live, tp, tl);
    V32 t[NW];
    const VB usable = B::load_target(tp, tl, live, t);
    B::stage(lds, qv, 0, nq);
    for (uint32_t i = 0; i < nq; i++) {
        VB hit;
        V32 d;
        ran[i] = B::compare(lds, i, t, tl, usable, k8, hit, d) ? 1u : 0u;
        for (int l = 0; l < 64; l++) res[64 * i + l] = hit.v[l] ? d.v[l] : 0xFFFFFFFFu;
    }
    return 0;
}

// Queries qblob[qoff[i] .. qoff[i + 1]), i < nq <= 256 / nw (one chunk, every one at most 4 nw bytes), against targets
// tblob[toff[j] .. toff[j + 1]), j < nt <= 64 (both blobs readable 16 bytes past their ends).  k8 = 8 min(k, 64) + 7, as the host entry
// passes it.  res[64 i + j]: the mismatch count of a hit, 0xFFFFFFFF otherwise and for the lanes at and above nt; ran[i]: 1 when the body
// compared query i, 0 when no usable lane had its length.  Returns 0, or -1 for bad arguments.
extern "C" int emu_hcross_chunk(const uint8_t *qblob, const uint64_t *qoff, uint32_t nq, const uint8_t *tblob, const uint64_t *toff, uint32_t nt,
                                uint32_t k8, int nw, uint32_t *res, uint32_t *ran) {
    if (nt > 64 || (nw != 4 && nw != 8 && nw != 16)) return -1;
    for (uint32_t i = 0; i < nq; i++) if (qoff[i + 1] - qoff[i] > 4u * (uint32_t)nw) return -1;
    if (nw == 4) return run<4>(qblob, qoff, nq, tblob, toff, nt, k8, res, ran);
    if (nw == 8) return run<8>(qblob, qoff, nq, tblob, toff, nt, k8, res, ran);
    return run<16>(qblob, qoff, nq, tblob, toff, nt, k8, res, ran);
}
