// ham_rules_check.cpp -- ham_wants_slices (triple_accel_amd/csrc/lev_plan.h): which Hamming batches take the sliced form, against the rule
// written out here independently, and the shapes that must stay on hamming_batch_kernel pinned by name.  Plain g++, no GPU.
#include <stdint.h>
#include <stdio.h>

#include "lev_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                                          \
    do {                                                                          \
        if (!(cond) && failures++ < 10) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    } while (0)

// The rule in words.  A batch is sliced when its strings are at least 64 KiB long (the measured crossover of the two kernels, at every
// pair count).  A CSR batch is judged by its length hint; without one it is sliced up to 8,192 pairs; beyond 65,536 pairs never.
static bool restated(uint64_t n, bool strided, uint64_t len, uint64_t hint) {
    if (n == 0 || n >= (1ull << 32)) return false;
    uint64_t judged = len;
    if (!strided) {
        if (n > 65536) return false;
        if (hint == 0) return n <= 8192;
        judged = hint;
    }
    return judged >= 64 * 1024;
}

int main() {
    static const uint64_t NS[] = {0, 1, 2, 3, 16, 64, 300, 1024, 2000, 4096, 8191, 8192, 8193, 10000, 65535, 65536, 65537, 1000000, 0xFFFFFFFFull, 1ull << 32};
    static const uint64_t LENS[] = {0, 1, 16, 255, 256, 512, 1023, 1024, 1025, 2048, 5000, 65535, 65536, 65537, 200000, 1u << 20, 1ull << 30, 0xFFFFFFFEull, 1ull << 33};
    for (uint64_t n : NS) for (uint64_t len : LENS) for (uint64_t hint : LENS) for (int s = 0; s < 2; s++)
        CHECK(ta::ham_wants_slices(n, s != 0, len, hint) == restated(n, s != 0, len, hint), "n=%llu strided=%d len=%llu hint=%llu",
              (unsigned long long)n, s, (unsigned long long)len, (unsigned long long)hint);
    // the shapes of bench.py and of the GPU tests from before the sliced form: exactly where they were
    CHECK(!ta::ham_wants_slices(10000, true, 1024, 0), "cfg1: 10,000 x 1 KiB");
    CHECK(!ta::ham_wants_slices(1000000, true, 256, 0), "1M x 256 B");
    CHECK(!ta::ham_wants_slices(200, true, 1024, 0), "200 x 1,024 (test_gpu_layouts)");
    CHECK(!ta::ham_wants_slices(1500, true, 100, 0) && !ta::ham_wants_slices(1500, true, 300, 0), "1,500 x 100 / 300, one side shared");
    CHECK(!ta::ham_wants_slices(500, false, 0, 299), "500 ragged pairs of up to 299 bytes with their hint");
    CHECK(!ta::ham_wants_slices(3, false, 0, 4) && !ta::ham_wants_slices(1, false, 0, 3), "the short CSR lists");
    CHECK(!ta::ham_wants_slices(1, true, 3, 0) && !ta::ham_wants_slices(1, true, 1024, 0), "single short pairs");
    CHECK(!ta::ham_wants_slices(100000, false, 0, 0) && !ta::ham_wants_slices(65537, false, 0, 1 << 20), "CSR beyond 65,536 pairs");
    // and the ones the form was built for
    CHECK(ta::ham_wants_slices(1, true, 1ull << 30, 0), "one pair of 1 GiB");
    CHECK(ta::ham_wants_slices(16, true, 64u << 20, 0), "16 x 64 MiB");
    CHECK(ta::ham_wants_slices(2000, true, 65536, 0), "2,000 x 64 KiB");
    CHECK(ta::ham_wants_slices(1000000, true, 65536, 0), "64 KiB strings at any pair count");
    CHECK(ta::ham_wants_slices(4096, false, 0, 4u << 20) && ta::ham_wants_slices(4096, false, 0, 0), "4,096 ragged pairs, with and without a hint");
    CHECK(!ta::ham_wants_slices(1, true, 65535, 0) && ta::ham_wants_slices(1, true, 65536, 0), "the crossover");
    CHECK(!ta::ham_wants_slices(300, true, 5000, 0) && !ta::ham_wants_slices(1024, true, 32768, 0), "below it the old kernel was faster at every pair count");
    CHECK(!ta::ham_wants_slices(7, false, 0, 40000) && ta::ham_wants_slices(7, false, 0, 0) && ta::ham_wants_slices(8192, false, 0, 0) &&
          !ta::ham_wants_slices(8193, false, 0, 0), "CSR: the hint decides; without one, up to 8,192 pairs");
    if (failures) { printf("ham rules: %d failure(s)\n", failures); return 1; }
    printf("ham rules: ok\n");
    return 0;
}
