// san_main.cpp -- stand-alone driver of the token cross body's emulation for `make san` (AddressSanitizer + UBSan, host code only): the
// collision cases once over the emulated LDS, every sequence in a heap block of exactly its size, so that a read outside a sequence's
// items or a table access outside the wavefront's slice is reported.  Answers are checked against a plain DP.  Never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

extern "C" int emu_cross_tok_query(const uint32_t *q, uint32_t m, const uint32_t *tdata, const uint64_t *toff, uint32_t nt, uint32_t k, int nw,
                                   int trans, uint32_t *res, uint32_t *skip);
extern "C" int emu_cross_tok_table_clean(int nw);
extern "C" void emu_cross_tok_home(const uint32_t *x, uint32_t n, uint32_t *out);

typedef std::vector<uint32_t> Seq;

static uint32_t dp(const Seq &a, const Seq &b, bool trans) {
    const size_t n = a.size(), m = b.size();
    std::vector<std::vector<uint32_t>> d(n + 1, std::vector<uint32_t>(m + 1));
    for (size_t i = 0; i <= n; i++) d[i][0] = (uint32_t)i;
    for (size_t j = 0; j <= m; j++) d[0][j] = (uint32_t)j;
    for (size_t i = 1; i <= n; i++)
        for (size_t j = 1; j <= m; j++) {
            uint32_t v = std::min({d[i - 1][j - 1] + (a[i - 1] != b[j - 1]), d[i - 1][j] + 1, d[i][j - 1] + 1});
            if (trans && i > 1 && j > 1 && a[i - 1] == b[j - 2] && a[i - 2] == b[j - 1]) v = std::min(v, d[i - 2][j - 2] + 1);
            d[i][j] = v;
        }
    return d[n][m];
}

static uint32_t home(uint32_t x) { uint32_t h; emu_cross_tok_home(&x, 1, &h); return h; }

// `count` distinct tokens from `from` on whose probes start at `slot`
static Seq colliding(uint32_t slot, size_t count, uint32_t from) {
    Seq out;
    for (uint32_t x = from; out.size() < count; x += 7919u) if (home(x) == slot) out.push_back(x);
    return out;
}

static int run_case(const char *name, const Seq &q, const std::vector<Seq> &targets) {
    int bad = 0;
    std::vector<uint64_t> off(targets.size() + 1, 0);
    for (size_t i = 0; i < targets.size(); i++) off[i + 1] = off[i] + targets[i].size();
    uint32_t *data = (uint32_t *)malloc(off.back() * 4 + (off.back() ? 0 : 4));    // exactly the items
    for (size_t i = 0; i < targets.size(); i++) if (!targets[i].empty()) memcpy(data + off[i], targets[i].data(), targets[i].size() * 4);
    uint32_t *qq = (uint32_t *)malloc(q.size() * 4 + (q.empty() ? 4 : 0));
    if (!q.empty()) memcpy(qq, q.data(), q.size() * 4);
    for (int nw = 1; nw <= 2; nw++) {
        if (q.size() > 32u * (uint32_t)nw) continue;
        for (int trans = 0; trans < 2; trans++)
            for (uint32_t k : {0u, 1u, 3u, 64u, 0xFFFFFFFFu}) {
                uint32_t res[64], skip[64];
                emu_cross_tok_query(qq, (uint32_t)q.size(), data, off.data(), (uint32_t)targets.size(), k, nw, trans, res, skip);
                if (emu_cross_tok_table_clean(nw) != 1) { printf("%s: table not clean (nw %d)\n", name, nw); bad++; }
                for (size_t i = 0; i < targets.size(); i++) {
                    const uint32_t d = dp(q, targets[i], trans != 0), want = d <= k ? d : 0xFFFFFFFFu;
                    if (res[i] != want) { printf("%s: target %zu nw %d trans %d k %u: %u, expected %u\n", name, i, nw, trans, k, res[i], want); bad++; }
                }
            }
    }
    free(data);
    free(qq);
    return bad;
}

int main() {
    int bad = 0;
    // (a) 64 distinct tokens on one home slot; targets: the query, its reverse, pieces of it, tokens absent from it on the same slot
    const Seq a = colliding(home(1), 64, 1), more = colliding(home(1), 8, 0x40000001u);
    std::vector<Seq> ta = {a, Seq(a.rbegin(), a.rend()), Seq(a.begin() + 1, a.end()), Seq(a.begin(), a.begin() + 31), more, Seq(), Seq(1, a[63]),
                           Seq(a.begin(), a.begin() + 3), Seq(a.begin() + 2, a.begin() + 7)};
    Seq sub = a; sub[40] = more[0]; ta.push_back(sub);
    bad += run_case("a", a, ta);
    // (b) / (c) a short query with two tokens on one slot; targets swap them and replace tokens by absent ones that start at their slots
    Seq b = colliding(5, 2, 3);
    for (uint32_t x = 100; b.size() < 20; x += 104729u) if (home(x) != 5 && std::find(b.begin(), b.end(), x) == b.end()) b.push_back(x);
    std::vector<Seq> tb = {b};
    { Seq t = b; std::swap(t[0], t[1]); tb.push_back(t); }
    for (size_t p : {0u, 7u, 19u}) { Seq t = b; t[p] = colliding(home(b[p]), 3, 0x20000003u)[2]; tb.push_back(t); }
    bad += run_case("bc", b, tb);
    // (d) duplicates in lanes 32 and above
    Seq d = a;
    for (size_t i = 0; i < 64; i++) d[i] = 1000u + 977u * (uint32_t)i;
    d[40] = d[50] = d[5]; d[60] = d[45];
    std::vector<Seq> td = {d, Seq(d.begin() + 32, d.end()), Seq(3, d[5]), Seq(2, d[45]), Seq(d.begin(), d.begin() + 41)};
    bad += run_case("d", d, td);
    printf(bad ? "FAILED: %d\n" : "ok (%d mismatches)\n", bad);
    return bad ? 1 : 0;
}
