// tab_parity_emu.cpp -- TabOps<EmuWave, EmuTab> (tab_ops_body.h) on the host: libta_tab_parity_emu.so, TESTS ONLY.
#include <stdint.h>
#include <string.h>

#include "emu_tab_ops.h"
#include "emu_wave.h"
#include "tab_ops_body.h"

using namespace ta;

extern "C" int ta_tab_parity_run(const uint32_t *in, uint32_t *out, uint32_t n_cases, void *) {
    static uint8_t lds[TA_TP_LDS_BYTES];
    memset(lds, 0xA5, sizeof lds);
    for (uint32_t c = 0; c < n_cases; c++) TabOps<EmuWave, EmuTab>::run_case(in, out, n_cases, c, lds);
    return 0;
}
extern "C" int ta_tab_parity_n_ops(void) { return (int)TA_TP_N_OPS; }
