// emu_sym.cpp -- host emulation driver of the token compaction body (sym_compact_body.h).  TESTS ONLY (see emu_wave.h).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "emu_wave.h"
#include "sym_compact_body.h"

namespace ta {

// the operations the body needs beyond the wave policy, lane by lane (atomics in lane order: one legal serialisation)
template <> struct SymOps<EmuWave> {
    using U32 = V32;
    using Bool = VB;
    static uint32_t readlane(const U32 &v, uint32_t l) { return v.v[l & 63]; }
    static void store_u8(uint8_t *p, const U32 &idx, const U32 &v, const Bool &pred) {
        for (int l = 0; l < 64; l++) if (pred.v[l]) p[idx.v[l]] = (uint8_t)v.v[l];
    }
    static void fence() {}
    static Bool claim(uint64_t *tab, const U32 &h, const U32 &x, const Bool &pred) {
        VB r;
        for (int l = 0; l < 64; l++) {
            r.v[l] = false;
            if (!pred.v[l]) continue;
            const uint64_t key = (1ull << 32) | x.v[l], old = tab[h.v[l]];
            if (old == 0) tab[h.v[l]] = key;
            r.v[l] = old == 0 || old == key;
        }
        return r;
    }
    static Bool holds(const uint64_t *tab, const U32 &h, const U32 &x, const Bool &pred, Bool &empty) {
        VB r;
        for (int l = 0; l < 64; l++) {
            const uint64_t e = pred.v[l] ? tab[h.v[l]] : 0ull;
            empty.v[l] = pred.v[l] && e == 0;
            r.v[l] = pred.v[l] && e == ((1ull << 32) | x.v[l]);
        }
        return r;
    }
    static void store_u64(uint64_t *p, const U32 &idx, uint64_t v, const Bool &pred) {
        for (int l = 0; l < 64; l++) if (pred.v[l]) p[idx.v[l]] = v;
    }
    static uint64_t ballot(const Bool &c) {
        uint64_t m = 0;
        for (int l = 0; l < 64; l++) if (c.v[l]) m |= 1ull << l;
        return m;
    }
    static U32 bits_below(uint64_t m) {
        V32 r;
        for (int l = 0; l < 64; l++) r.v[l] = (uint32_t)__builtin_popcountll(m & ((1ull << l) - 1ull));
        return r;
    }
    static void append(uint32_t *list, uint32_t *count, uint32_t v) { list[(*count)++] = v; }
};

}  // namespace ta

using namespace ta;

// the compaction of a batch as the launcher sets it up (table_cap: 0 or a power of two >= 2 x the longest shorter side, >= 64);
// the codes go to ca / cb (CSR: at the element offsets, strided: byte stride = len), the overflow list to ovf (n entries)
extern "C" int emu_sym_compact(const uint32_t *a, const uint64_t *a_off, uint64_t a_stride, uint64_t a_len,
                               const uint32_t *b, const uint64_t *b_off, uint64_t b_stride, uint64_t b_len, uint32_t n,
                               uint32_t table_cap, uint32_t waves, uint8_t *ca, uint8_t *cb, uint32_t *ovf, uint32_t *n_ovf) {
    SymCompactParams P;
    P.a_data = a; P.b_data = b; P.a_off = a_off; P.b_off = b_off;
    P.a_stride = a_stride; P.a_len = a_len; P.b_stride = b_stride; P.b_len = b_len;
    P.ca = ca; P.cb = cb; P.n = n;
    std::vector<uint64_t> table((size_t)waves * table_cap + 1);
    std::vector<uint32_t> flags((size_t)waves * table_cap + 1);
    P.table = table.data(); P.flags = flags.data(); P.table_cap = table_cap;
    *n_ovf = 0;
    P.ovf_list = ovf; P.ovf_count = n_ovf;
    for (uint32_t w = 0; w < waves; w++) SymCompact<EmuWave>::run(P, w, waves);
    return 0;
}
