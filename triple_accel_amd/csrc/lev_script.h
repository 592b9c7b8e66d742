// lev_script.h -- the host half of a traceback, stated once: the walk from (n, m) back to (0, 0) turns step codes into the reference's
// run-length edit script (src/levenshtein.rs:561-606), and the records of the two DP kernels are decoded into step codes.  A step code
// names the predecessor cell: 0 = (i-1, j-1), 1 = (i, j-1), 2 = (i-1, j), 3 = (i-2, j-2); the kernels decide it (the tie order of
// :493-532).  x is the shorter string (the rows), y the longer one; `swap`: the caller's a went to the columns (:386-390), which swaps
// the two gaps' names.  Plain C++ (the tests walk lists of their own); the forward replays on the device are lev_trace_emit.h.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <vector>

#include "../../include/triple_accel_amd.h"

namespace ta {

template <class Item>   // uint8_t: bytes, uint32_t: tokens
struct ScriptBuilder {
    std::vector<ta_edit> runs;
    ScriptBuilder(const Item *x, size_t n, const Item *y, size_t m, bool swap) : x_(x), y_(y), i_(n), j_(m), swap_(swap) {}
    size_t i() const { return i_; }
    size_t j() const { return j_; }
    void step(uint32_t code) {
        uint32_t e;
        switch (code) {
            case 0: i_--; j_--; e = (x_[i_] == y_[j_]) ? TA_EDIT_MATCH : TA_EDIT_MISMATCH; break;
            case 1: j_--; e = swap_ ? TA_EDIT_BGAP : TA_EDIT_AGAP; break;
            case 2: i_--; e = swap_ ? TA_EDIT_AGAP : TA_EDIT_BGAP; break;
            default: i_ -= 2; j_ -= 2; e = TA_EDIT_TRANSPOSE; break;
        }
        if (!runs.empty() && runs.back().edit == e) runs.back().count++;
        else runs.push_back(ta_edit{e, 0u, 1u});
    }
    void finish() { for (size_t a = 0, b = runs.size(); a + 1 < b; a++, b--) { const ta_edit t = runs[a]; runs[a] = runs[b - 1]; runs[b - 1] = t; } }   // :605 reverse
    // the finished script as the malloc'ed array of the single-call ABI (ta_free); an empty script leaves *edits as it is (nullptr)
    int release(ta_edit **edits, size_t *n_edits) const {
        *n_edits = 0;
        if (runs.empty()) return TA_OK;
        if (!(*edits = (ta_edit *)malloc(runs.size() * sizeof(ta_edit)))) return TA_ERR_ARG;
        for (size_t t = 0; t < runs.size(); t++) (*edits)[t] = runs[t];
        *n_edits = runs.size();
        return TA_OK;
    }
private:
    const Item *x_, *y_;
    size_t i_, j_;
    bool swap_;
};

// The DP wide kernel's records (lev_wide.hip): per stripe of 2048 rows and column, 64 lanes x 2 words of sixteen 2-bit codes.  Row 0 is
// one a_gap run and column 0 one b_gap run: the kernel stores nothing for them.
static inline uint32_t wide_trace_code(const uint32_t *tr, uint64_t tcols, size_t i, size_t j) {
    if (i == 0) return 1;
    if (j == 0) return 2;
    const size_t q = (i - 1) / 2048, r = (i - 1) % 2048, lane = r / 32, rr = r % 32;
    return (tr[((q * tcols + j) * 64 + lane) * 2 + (rr >> 4)] >> (2 * (rr & 15))) & 3u;
}

// The DP band kernel's records (lev_band_body.h): per step tau and phase, 64 lanes x tw words; a lane holds D diagonals, the even
// ones in one phase's words and the odd ones in the other's.  o_pair: the pair's band offset (lev_pair_offset).
static inline uint32_t band_trace_code(const uint32_t *tr, uint32_t D, uint32_t tw, uint32_t o_pair, size_t i, size_t j) {
    const uint32_t s = (uint32_t)(i + j), p = (uint32_t)(j + o_pair - i);
    const uint32_t g = p / D, q = p % D, par = q & 1u, c = q >> 1, tau = (s - 1) >> 1;
    return (tr[(((size_t)tau * 2 + par) * 64 + g) * tw + ((2 * c) >> 5)] >> ((2 * c) & 31)) & 3u;
}

}  // namespace ta
