// emu_hsearch_batch.cpp -- host emulation driver of the Hamming search batch body (ham_search_batch_body.h).  TESTS ONLY: one pair as
// one lane of the batch kernels runs it, in the form the caller names.
#include <stdint.h>
#include <string.h>

#include "emu_wave.h"
#include "ham_search_batch_body.h"

using namespace ta;

template <int B>
static uint32_t bits_form(const uint8_t *needle, uint32_t n, const uint8_t *hay, uint64_t h, uint32_t k, bool best, ta_match *out, uint64_t cap) {
    uint32_t mis[256];
    for (uint32_t c = 0; c < 256; c++) mis[c] = ham_bits_mis(needle, n, c);      // (the kernel keeps this table in LDS)
    auto lk = [&](uint32_t w, int b) { return mis[(w >> (8 * b)) & 0xffu]; };
    return ham_batch_pair_bits<B>(needle, n, hay, h, k, best, lk, out, cap);
}

// One pair.  form: 2 / 4 / 8 / 16 = the register form with that many needle dwords (needs n <= 4 form); 0 = the memory form;
// 1 = the bit-sliced form (needs 1 <= n <= 32, k < n).  Returns the pair's count word (TA_NONE: the NUL verdict), 0xFFFFFFFE for a
// form the pair cannot take; out gets min(count, cap) matches.
extern "C" uint32_t emu_hsearch_batch_pair(const uint8_t *needle, uint64_t n, const uint8_t *hay, uint64_t h, uint32_t k, int best, int form,
                                           ta_match *out, uint64_t cap) {
    const bool b = best != 0;
    switch (form) {
        case 0: return ham_batch_pair_mem(needle, n, hay, h, k, b, out, cap);
        case 1:
            if (n < 1 || n > 32 || k >= n) return 0xFFFFFFFEu;
            switch (ham_bits_planes(k)) {
                case 1: return bits_form<1>(needle, (uint32_t)n, hay, h, k, b, out, cap);
                case 2: return bits_form<2>(needle, (uint32_t)n, hay, h, k, b, out, cap);
                case 3: return bits_form<3>(needle, (uint32_t)n, hay, h, k, b, out, cap);
                case 4: return bits_form<4>(needle, (uint32_t)n, hay, h, k, b, out, cap);
                case 5: return bits_form<5>(needle, (uint32_t)n, hay, h, k, b, out, cap);
            }
            return 0xFFFFFFFEu;
        case 2: if (n <= 8) return ham_batch_pair_regs<2>(needle, n, hay, h, k, b, out, cap); break;
        case 4: if (n <= 16) return ham_batch_pair_regs<4>(needle, n, hay, h, k, b, out, cap); break;
        case 8: if (n <= 32) return ham_batch_pair_regs<8>(needle, n, hay, h, k, b, out, cap); break;
        case 16: if (n <= 64) return ham_batch_pair_regs<16>(needle, n, hay, h, k, b, out, cap); break;
    }
    return 0xFFFFFFFEu;
}

// the online fold alone over a given hit list (increasing start): what HamBatchSink keeps
extern "C" uint32_t emu_hsearch_batch_fold(const ta_match *hits, uint64_t n_hits, uint32_t k, int best, ta_match *out, uint64_t cap) {
    HamBatchSink sink;
    sink.init(out, cap, best != 0, k, 0);
    for (uint64_t i = 0; i < n_hits; i++) {
        sink.n = (uint32_t)(hits[i].end - hits[i].start);
        sink.put((uint32_t)hits[i].start, hits[i].k);
    }
    return sink.count;
}
