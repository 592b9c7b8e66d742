// wave_parity_emu.cpp -- WaveOps<EmuWave> (wave_ops_body.h) on the host: libta_wave_parity_emu.so, TESTS ONLY.  Same entry as
// wave_parity_dev.hip over host pointers (`stream` is ignored).
#include <stdint.h>
#include <string.h>

#include "emu_wave.h"
#include "wave_ops_body.h"

using namespace ta;

TA_WP_DEFINE_OP_NAMES()

// 0 = done, 1 = `in` or `hdr` not aligned as wave_ops_body.h asks (the pointer pieces mask absolute addresses)
extern "C" int ta_wave_parity_run(const uint32_t *in, const uint32_t *hdr, uint32_t *out, uint32_t n_cases, void *) {
    if (((uintptr_t)in & 255u) || ((uintptr_t)hdr & 7u)) return 1;
    static uint8_t lds[TA_WP_LDS_BYTES];
    memset(lds, 0xA5, sizeof lds);
    EmuWave::clear_ranges();
    EmuWave::add_range((const uint8_t *)in, (uint64_t)n_cases * TA_WP_CASE_BYTES);      // a load outside the cases reads 0xA5, not the heap
    for (uint32_t c = 0; c < n_cases; c++) WaveOps<EmuWave>::run_case(in, hdr, out, n_cases, c, lds);
    EmuWave::clear_ranges();
    return 0;
}
