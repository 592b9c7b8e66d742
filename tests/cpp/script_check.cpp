// script_check.cpp -- the host half of a traceback (triple_accel_amd/csrc/lev_script.h: ScriptBuilder, wide_trace_code, band_trace_code)
// against its definition, written out here independently: one edit per step walking back from (n, m), reversed, equal neighbours
// grouped; and the two record layouts filled by the inverse addressing and read back cell by cell.  Plain g++, no GPU.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

#include "lev_script.h"

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond) && failures++ < 10) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {                       // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % below);
}

typedef std::vector<std::pair<uint32_t, uint64_t>> Script;   // (edit, count)

// The definition: `steps` lists the walk from (n, m) to (0, 0).  Edit values as include/triple_accel_amd.h numbers them:
// 0 Match, 1 Mismatch, 2 AGap, 3 BGap, 4 Transpose.
template <class Item>
static Script expected(const Item *x, size_t n, const Item *y, size_t m, bool swap, const std::vector<uint32_t> &steps, bool *legal) {
    std::vector<uint32_t> one;                              // one edit per step, back to front
    long i = (long)n, j = (long)m;
    for (uint32_t s : steps) {
        if (s == 0) { i -= 1; j -= 1; if (i >= 0 && j >= 0) one.push_back(x[i] == y[j] ? 0u : 1u); }
        else if (s == 1) { j -= 1; one.push_back(swap ? 3u : 2u); }
        else if (s == 2) { i -= 1; one.push_back(swap ? 2u : 3u); }
        else { i -= 2; j -= 2; one.push_back(4u); }
        if (i < 0 || j < 0) { *legal = false; return Script(); }
    }
    *legal = i == 0 && j == 0;
    Script out;
    for (size_t t = one.size(); t-- > 0;) {                 // front to back
        if (!out.empty() && out.back().first == one[t]) out.back().second++;
        else out.push_back({one[t], 1});
    }
    return out;
}

template <class Item>
static void check_walk(const char *what, const std::vector<Item> &x, const std::vector<Item> &y, bool swap, const std::vector<uint32_t> &steps,
                       const Script *by_hand = nullptr) {
    bool legal = false;
    const Script want = expected(x.data(), x.size(), y.data(), y.size(), swap, steps, &legal);
    CHECK(legal, "%s: the test's own walk does not end at (0, 0)", what);
    if (!legal) return;
    if (by_hand) CHECK(want == *by_hand, "%s: the definition disagrees with the script written by hand", what);
    ta::ScriptBuilder<Item> sb(x.data(), x.size(), y.data(), y.size(), swap);
    CHECK(sb.i() == x.size() && sb.j() == y.size(), "%s: cursor starts at (%zu, %zu)", what, sb.i(), sb.j());
    for (uint32_t s : steps) sb.step(s);
    CHECK(sb.i() == 0 && sb.j() == 0, "%s: cursor ends at (%zu, %zu)", what, sb.i(), sb.j());
    sb.finish();
    CHECK(sb.runs.size() == want.size(), "%s: %zu runs, want %zu", what, sb.runs.size(), want.size());
    for (size_t t = 0; t < want.size() && t < sb.runs.size(); t++)
        CHECK(sb.runs[t].edit == want[t].first && sb.runs[t].count == want[t].second && sb.runs[t].pad_ == 0,
              "%s: run %zu is (%u, %llu), want (%u, %llu)", what, t, sb.runs[t].edit, (unsigned long long)sb.runs[t].count, want[t].first,
              (unsigned long long)want[t].second);
    ta_edit *edits = nullptr;
    size_t n_edits = 12345;
    CHECK(sb.release(&edits, &n_edits) == TA_OK, "%s: release", what);
    CHECK(n_edits == want.size(), "%s: release gives %zu runs, want %zu", what, n_edits, want.size());
    CHECK((edits == nullptr) == want.empty(), "%s: an empty script leaves the pointer alone, any other one sets it", what);
    for (size_t t = 0; edits && t < want.size() && t < n_edits; t++)
        CHECK(edits[t].edit == want[t].first && edits[t].count == want[t].second && edits[t].pad_ == 0, "%s: released run %zu", what, t);
    free(edits);
}

// a random legal path over random strings of a small alphabet, built FORWARDS from (0, 0); the walk is its reverse
template <class Item>
static void random_walk(uint32_t max_len, Item high) {
    const size_t n = rnd(max_len + 1), m = rnd(max_len + 1);
    const uint32_t letters = 1 + rnd(3);
    std::vector<Item> x(n), y(m);
    for (auto &v : x) v = (Item)(high + rnd(letters));
    for (auto &v : y) v = (Item)(high + rnd(letters));
    std::vector<uint32_t> fwd;
    size_t i = 0, j = 0;
    while (i < n || j < m) {
        uint32_t moves[4], nm = 0;
        if (i < n && j < m) moves[nm++] = 0;
        if (j < m) moves[nm++] = 1;
        if (i < n) moves[nm++] = 2;
        if (i + 2 <= n && j + 2 <= m) moves[nm++] = 3;
        const uint32_t s = moves[rnd(nm)];
        fwd.push_back(s);
        if (s == 0) { i++; j++; } else if (s == 1) j++; else if (s == 2) i++; else { i += 2; j += 2; }
    }
    const std::vector<uint32_t> steps(fwd.rbegin(), fwd.rend());
    for (int swap = 0; swap < 2; swap++) check_walk("random walk", x, y, swap != 0, steps);
}

template <class Item>
static void check_by_hand(Item high) {
    typedef std::vector<Item> V;
    const Item a = (Item)(high + 1), b = (Item)(high + 2), c = (Item)(high + 3);
    const Script none;
    check_walk<Item>("both sides empty", V{}, V{}, false, {}, &none);
    const Script agap3 = {{2, 3}}, bgap3 = {{3, 3}};
    check_walk<Item>("empty rows", V{}, V{a, b, c}, false, {1, 1, 1}, &agap3);
    check_walk<Item>("empty rows, swapped", V{}, V{a, b, c}, true, {1, 1, 1}, &bgap3);
    check_walk<Item>("empty columns", V{a, b, c}, V{}, false, {2, 2, 2}, &bgap3);
    check_walk<Item>("empty columns, swapped", V{a, b, c}, V{}, true, {2, 2, 2}, &agap3);
    // a Match run next to a Mismatch run: both come from step 0 and stay two runs
    const Script mm = {{0, 1}, {1, 1}, {0, 2}};
    check_walk<Item>("match / mismatch neighbours", V{a, b, c, c}, V{a, c, c, c}, false, {0, 0, 0, 0}, &mm);
    // the walk reaches row 0 with columns left (front of the script: a_gap), or column 0 with rows left (b_gap)
    const Script row0 = {{2, 2}, {0, 2}}, row0s = {{3, 2}, {0, 2}};
    check_walk<Item>("ends on row 0", V{a, b}, V{c, c, a, b}, false, {0, 0, 1, 1}, &row0);
    check_walk<Item>("ends on row 0, swapped", V{a, b}, V{c, c, a, b}, true, {0, 0, 1, 1}, &row0s);
    const Script col0 = {{3, 2}, {1, 1}}, col0s = {{2, 2}, {1, 1}};
    check_walk<Item>("ends on column 0", V{a, b, c}, V{a}, false, {0, 2, 2}, &col0);
    check_walk<Item>("ends on column 0, swapped", V{a, b, c}, V{a}, true, {0, 2, 2}, &col0s);
    // a transposition as the walk's first step (the script's last run) and as its last step (the script's first run)
    const Script t_last = {{0, 1}, {4, 1}}, t_first = {{4, 1}, {0, 1}}, t_both = {{4, 2}};
    check_walk<Item>("transposition first", V{c, a, b}, V{c, b, a}, false, {3, 0}, &t_last);
    check_walk<Item>("transposition last", V{a, b, c}, V{b, a, c}, false, {0, 3}, &t_first);
    check_walk<Item>("transpositions only, swapped", V{a, b, a, b}, V{b, a, b, a}, true, {3, 3}, &t_both);
    // every step code in one walk, both labellings
    const Script all = {{4, 1}, {3, 1}, {2, 1}, {1, 1}, {0, 1}}, alls = {{4, 1}, {2, 1}, {3, 1}, {1, 1}, {0, 1}};
    check_walk<Item>("every code", V{a, b, c, a, c}, V{b, a, c, b, c}, false, {0, 0, 1, 2, 3}, &all);
    check_walk<Item>("every code, swapped", V{a, b, c, a, c}, V{b, a, c, b, c}, true, {0, 0, 1, 2, 3}, &alls);
    // one run of more than 2^16 equal edits: the count is 64 bits wide
    const size_t big = 70000;
    const Script long_match = {{0, big}}, long_gap = {{2, big}};
    check_walk<Item>("70000 matches", V(big, a), V(big, a), false, std::vector<uint32_t>(big, 0u), &long_match);
    check_walk<Item>("70000 gaps", V{}, V(big, a), false, std::vector<uint32_t>(big, 1u), &long_gap);
}

// The code the test stores at (i, j): every bit of i and of j reaches the two bits taken (the splitmix64 finaliser), so two cells a
// power of two of rows or columns apart -- a word half, a lane, a stripe -- do not hold the same code by construction.
static uint32_t cell_code(size_t i, size_t j) {
    uint64_t z = ((uint64_t)i << 32 | (uint64_t)j) + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 62);
}

// The DP wide kernel's layout: stripes of 2048 rows (64 lanes x 32 rows); per stripe, column and lane two words, the lane's rows
// 0..15 in the first and 16..31 in the second, two bits each from bit 0 up.
static void check_wide_records() {
    const size_t n = 2049, m = 37;                           // two stripes: row 2049 is the second stripe's first
    const uint64_t tcols = m + 64;
    std::vector<uint32_t> tr(((n + 2047) / 2048) * tcols * 64 * 2, 0u);
    for (size_t i = 1; i <= n; i++) for (size_t j = 1; j <= m; j++) {
        const size_t stripe = (i - 1) >> 11, within = (i - 1) & 2047, lane = within >> 5, row = within & 31;
        const size_t word = ((stripe * tcols + j) * 64 + lane) * 2 + (row >= 16 ? 1 : 0);
        tr[word] |= cell_code(i, j) << (2 * (row & 15));
    }
    for (size_t i = 1; i <= n; i++) for (size_t j = 1; j <= m; j++)
        CHECK(ta::wide_trace_code(tr.data(), tcols, i, j) == cell_code(i, j), "wide records, cell (%zu, %zu)", i, j);
    for (size_t j = 0; j <= m; j++) CHECK(ta::wide_trace_code(tr.data(), tcols, 0, j) == 1, "wide records, row 0 is an a_gap run (column %zu)", j);
    for (size_t i = 1; i <= n; i++) CHECK(ta::wide_trace_code(tr.data(), tcols, i, 0) == 2, "wide records, column 0 is a b_gap run (row %zu)", i);
}

// The DP band kernel's layout: the cell (i, j) lies on diagonal p = j - i + o_pair and anti-diagonal s = i + j.  A lane holds D
// consecutive diagonals; the even ones of a lane are computed in one phase and the odd ones in the other, two anti-diagonals per
// step tau = (s - 1) / 2.  Per (tau, phase): 64 lanes x ceil(D / 32) words, the lane's diagonal pair c at bits 2 c, 2 c + 1.
// o_pair (odd, as lev_pair_offset makes it, and above n: p >= 1 for every cell) places the 171 diagonals of the pair in the lanes.
static void check_band_records(uint32_t D, uint32_t o_pair, std::vector<uint8_t> *lanes_read) {
    const size_t n = 80, m = 90;
    const uint32_t tw = (D + 31) / 32;
    std::vector<uint32_t> tr(((n + m + 1) / 2 + 1) * 2 * 64 * tw, 0u);
    std::vector<uint8_t> used(tr.size() * 16, 0);
    for (size_t i = 0; i <= n; i++) for (size_t j = 0; j <= m; j++) {
        if (i + j == 0) continue;
        const size_t p = j + o_pair - i, lane = p / D, within = p - lane * D, phase = within % 2, pair = within / 2, tau = (i + j - 1) / 2;
        if (lane >= 64) continue;
        const size_t bit = ((tau * 2 + phase) * 64 + lane) * tw * 32 + 2 * pair;
        CHECK(!used[bit / 2], "band records D=%u: two cells share a slot at (%zu, %zu)", D, i, j);
        used[bit / 2] = 1;
        tr[bit / 32] |= cell_code(i, j) << (bit % 32);
    }
    size_t read = 0, second_word = 0;
    for (size_t i = 0; i <= n; i++) for (size_t j = 0; j <= m; j++) {
        if (i + j == 0 || (j + o_pair - i) / D >= 64) continue;
        CHECK(ta::band_trace_code(tr.data(), D, tw, o_pair, i, j) == cell_code(i, j), "band records D=%u, cell (%zu, %zu)", D, i, j);
        read++;
        (*lanes_read)[(j + o_pair - i) / D] = 1;
        if (((j + o_pair - i) % D) / 2 >= 16) second_word++;
    }
    CHECK(read == (n + 1) * (m + 1) - 1, "band records D=%u o_pair=%u: every cell is inside the 64 lanes", D, o_pair);
    CHECK((second_word > 0) == (D > 32), "band records D=%u: cells beyond a lane's first word", D);
}
// the band moved through the lanes in steps of its own width, the last position ending on lane 63's last diagonal
static void check_band_records(uint32_t D) {
    std::vector<uint8_t> lanes_read(64, 0);
    const uint32_t last = 64 * D - 91;                       // (odd; the largest p is then 64 D - 1)
    for (uint32_t o_pair = 81; ; o_pair += 170) {
        if (o_pair > last) o_pair = last;
        check_band_records(D, o_pair, &lanes_read);
        if (o_pair == last) break;
    }
    for (size_t l = 0; l < 64; l++) CHECK(lanes_read[l], "band records D=%u: lane %zu was never read", D, l);
}

int main() {
    check_by_hand<uint8_t>(0);
    check_by_hand<uint32_t>(0xFFFFFF00u);                    // items that differ only above the low byte's reach
    for (int t = 0; t < 2000; t++) { random_walk<uint8_t>(12, 'a'); random_walk<uint32_t>(12, 0x10000u); }
    for (int t = 0; t < 200; t++) random_walk<uint32_t>(60, 1u << 31);
    check_wide_records();
    for (uint32_t D : {16u, 34u, 66u}) check_band_records(D);
    if (failures) { printf("script: %d failures\n", failures); return 1; }
    printf("script: ok\n");
    return 0;
}
