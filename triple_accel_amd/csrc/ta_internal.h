// ta_internal.h -- host-side plumbing shared by the C-ABI translation units: the error / scratch / stream context, the names of the
// thread-local scratch slots (ScratchSlot), the host rules over ta_edit_costs and ta_strings that every batch entry shares (defined once
// in ta_api.hip; their pure halves live in lev_plan.h), and the launchers' prototypes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/triple_accel_amd.h"
#include "lev_band_body.h"
#include "lev_plan.h"
#include "lev_route.h"

namespace ta {

void set_last_error(const char *what, hipError_t e);
void set_last_error_msg(const char *msg);
// the dominant kernel of this thread's last pass as a profiler prints it, without "void ta::" and the parameter list
// (ta_last_kernel_name: bench.py refuses to splice committed counter figures recorded for another kernel)
void set_last_kernel_name(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

#define TA_HIP(expr)                                        \
    do {                                                    \
        hipError_t e__ = (expr);                            \
        if (e__ != hipSuccess) {                            \
            ::ta::set_last_error(#expr, e__);               \
            return TA_ERR_HIP;                              \
        }                                                   \
    } while (0)

// Thread-local grow-only device scratch.
struct Scratch {
    void *dev = nullptr;
    size_t cap = 0;
    bool bins_clean = false;    // order_pairs' histogram slots: the last pass over this slot ran to its end (the histogram is zero)
    int ensure(size_t bytes);   // TA_OK / TA_ERR_HIP
    void release();
    ~Scratch();
};
// The thread-local scratch slots.  Everything a call enqueues goes to ONE stream, and a later call of the thread on another stream first
// waits for the earlier one (StreamGuard): two users of a slot that enqueue one after the other never meet.  A slot may therefore be shared
// by entry points that never call each other, and inside one call by buffers of which the first is dead (its last kernel enqueued, or its
// value read back under a synchronisation) before the second is ensured.  What must NOT share a slot: two buffers live in the same call,
// and anything that keeps its CONTENT from one call to the next (marked "persists").  The numbers are baked into captured graphs through
// the buffers' addresses and are part of nothing else.
enum ScratchSlot {
    SLOT_PAIR_STAGE = 0,     // stage_pair (ta_api.hip): a single call's long pair and its result word, live until the call's fetch.  Alone.
    SLOT_SEARCH_HITS = 1,    // ta_search.hip: the host search entries' hit buffer (run_search_host, first_hit_windows).  Alone.
    SLOT_SEARCH_CTL = 2,     // ta_search.hip: the SearchCtl / counters of one search pass; best_hits_of reuses its first words once the pass's
                             // count has been read back.  Search entries only.
    SLOT_COUNT = 3,          // ta_api.hip: side_max_len's word (read back under a synchronisation before anything else is enqueued), then the
                             // list counters of the same call: the unit prefilter's, the exp loop's (two per round).
    SLOT_SUBSET_A = 4,       // the exp loop's ping-pong subset lists (4 and 5) / the unit prefilter's survivor list (4): ta_levenshtein_exp_batch
    SLOT_SUBSET_B = 5,       // and ta_levenshtein_k_batch never call each other.  5 is also the search filter's list of flagged blocks (ta_search.hip,
                             // search_dev_core): no search entry runs a distance pass.
    SLOT_LINES = 6,          // what ONE kernel of a pass needs beside its inputs: the stripe boundary lines of lev_wide.hip / lev_widebits.hip (every
                             // launcher there; lev_pass runs one of them per pass, the exp loop's passes follow each other on the stream), those of
                             // trace_widebits (ta_trace.hip), the memory-backed columns of ta_search.hip (needles beyond 32 bytes) and the DP band kernel's
                             // traceback records (ta_trace.hip: ta_levenshtein_trace, the record route of ta_levenshtein_trace_batch: neither runs a lev_wide /
                             // lev_widebits launcher; the token entries' wide pass follows the byte pass on the stream).
    SLOT_AUX_A = 7,          // ta_search.hip: the needle's device copy (needles beyond 32 / 64 bytes) | ta_trace.hip, trace_bits_batch: the run counts.
    SLOT_AUX_B = 8,          // lev_widebits.hip: the tiled form's stripe states (4 and 5 hold the exp loop's subsets while it runs) | trace_bits_batch:
                             // the run lists -- ensured after its distance pass (lev_pass, which may take the tiled form) has been enqueued.
    SLOT_TRACE = 9,          // traceback records of one pair (ta_trace.hip: trace_widebits, trace_wide; ta_tokens.hip: wide_pair_u32) | trace_bits_batch: the
                             // checkpoints | the record route of ta_levenshtein_trace_batch: the walked paths.  One route per call; the packed form's
                             // sub-batches are calls of their own, one after the other.
    SLOT_EXP_BOUND = 10,     // ta_levenshtein_exp_batch: the bag lower bounds ...
    SLOT_EXP_WORK = 11,      // ... and the list of pairs a bounded round takes.  Alone.
    SLOT_SELECT = 12,        // ta_search.hip: a Best pass's SearchSlots, then (after the pass's synchronisation) best_hits_of's selection |
                             // ta_trace.hip, ta_levenshtein_trace_batch_packed: the ta_edit records of a sub-batch, live across the inner record-route call
                             // (which uses 6 and 9).
    SLOT_ORDER = 13,         // order_pairs for the distance entries (ta_levenshtein_k_batch, _exp_batch; ta_trace.hip: trace_bits_batch): the length-ordered list,
    SLOT_ORDER_BINS = 14,    // read until the call's last pass, and its histogram -- persists (zero between complete passes; Scratch::bins_clean).
    SLOT_ALPHA_BAD = 15,     // ta_levenshtein_k_batch_alphabet: the pairs with a byte outside the alphabet ...
    SLOT_ALPHA_COUNT = 16,   // ... and the two counters taken in turn -- persists.  Alone.
    SLOT_SEARCH_HAY = 17,    // ta_search.hip: the host search entries' haystack staging -- persists (ta_levenshtein_search_resume); nothing else writes it.
    SLOT_TOK_CA = 18,        // ta_tokens.hip: the byte codes of both sides, live across the byte entry point the token entry calls,
    SLOT_TOK_CB = 19,
    SLOT_TOK_TABLE = 20,     // the compaction's hash tables,
    SLOT_TOK_OVF = 21,       // tok_side's word (read back under a synchronisation), then the overflow count and list, live until the overflow pass,
    SLOT_TOK_STAGE = 22,     // one host pair of u32 items and its result word (wide_pair_u32).  18..22: the token entries alone.
    SLOT_SB_ORDER = 23,      // ta_search_batch.hip: order_pairs for both search-batch entries -- its own list and histogram (24 persists like 14), so a
    SLOT_SB_BINS = 24,       // search batch and a distance batch enqueued back to back never share an order.
    SLOT_SB_CTL = 25,        // word 0: Route S's candidate count; words 4..7 (two 64-bit words at offset 2): measure_max_lens.
    SLOT_SB_LIST = 26,       // Route S: the candidate pairs ...
    SLOT_SB_SPAN = 27,       // ... and their spans.
    SLOT_SB_COL = 28,        // the memory-backed columns (needles beyond 32 bytes).  23..28: the search batch alone.
    SLOT_CROSS_CTL = 30,     // ta_cross.hip: measure_max_lens' two 64-bit words.  Alone.
    SLOT_SX_CTL = 31,        // ta_levenshtein_search_cross: word 0 the candidate count of the sub-batch in flight; words 4..7: measure_max_lens.
    SLOT_SX_REC = 32,        // ... the candidate / result records of one sub-batch (at most SX_BUDGET bytes),
    SLOT_SX_NEAR = 33,       // ... and the nearest words when the caller asks for best_dev without nearest_dev.  31..33: that entry and
                             // ta_levenshtein_search_cross_with_opts (one host path; neither calls the other).
    SLOT_HSX_CTL = 34,       // ta_hamming_search_cross: measure_max_lens' two 64-bit words ...
    SLOT_HSX_WORD = 35,      // ... and the packed nearest words (d << 48 | needle << 32 | start), one per haystack, live from the fill to the
                             // finish kernel.  34, 35: that entry and ta_hamming_search_cross_with_opts (one host path; neither calls
                             // the other).
    SLOT_HAM_LONG = 36,      // ham_long.hip: the plan of a CSR batch and the per-slice counts, dead once the finish kernel has run (ta_hamming_batch,
                             // ta_hamming_dev, the chunked ta_hamming).  Alone.
    SLOT_SX_COL = 37,        // ta_levenshtein_search_cross_with_opts, needles beyond 32 bytes: the exact pass's memory-backed columns, one per
                             // resident lane (at most SX_BUDGET bytes), dead once a sub-batch's exact kernel has run.  That entry alone.
    TA_SCRATCH_SLOTS
};
Scratch &tls_scratch(ScratchSlot which);

// ---- host rules over the C structs, stated once (the pure halves: lev_plan.h)
static inline bool costs_ok(const ta_edit_costs *c) {       // EditCosts::new, src/levenshtein.rs:44-52
    return c && lev_costs_valid(c->mismatch_cost, c->gap_cost, c->has_transpose != 0, c->transpose_cost);
}
static inline bool costs_unit(const ta_edit_costs *c) {     // LEVENSHTEIN_COSTS / RDAMERAU_COSTS
    return lev_is_unit(c->mismatch_cost, c->gap_cost, c->start_gap_cost, c->has_transpose != 0, c->transpose_cost);
}
static inline uint32_t costs_scale(const ta_edit_costs *c) {   // 1: unit family, g: g times one, 0: neither (lev_cost_scale)
    return lev_cost_scale(c->mismatch_cost, c->gap_cost, c->start_gap_cost, c->has_transpose != 0, c->transpose_cost);
}
static inline StrView view_of(const ta_strings *s) { return StrView{s->blob, s->off, s->stride, s->len}; }
// the strings lo.. of a batch side as a side of their own (sub-batches); max_len: the whole side's bound, as the CSR form's
static inline ta_strings strings_slice(const ta_strings *s, uint64_t lo, uint64_t max_len) {
    return s->off ? ta_strings{s->blob, s->off + lo, 0, 0, max_len} : ta_strings{s->blob + lo * s->stride, nullptr, s->stride, s->len, s->len};
}
static inline ta_edit_costs unit_costs(bool trans) {       // LEVENSHTEIN_COSTS, or RDAMERAU_COSTS with the transposition term
    return ta_edit_costs{1, 1, 0, (uint8_t)(trans ? 1 : 0), (uint8_t)(trans ? 1 : 0)};
}
static inline LevCosts costs_of(const ta_edit_costs *c) {   // as the planners take them: no transposition, no cost
    return LevCosts{c->mismatch_cost, c->gap_cost, c->start_gap_cost, c->has_transpose != 0, c->has_transpose ? (uint32_t)c->transpose_cost : 0u};
}
static inline uint32_t launch_cell_bits(uint64_t max_len, uint32_t k, const ta_edit_costs *c) {   // ta_launch_info.cell_bits of a batch
    return lev_select(max_len, max_len, k, c->mismatch_cost, c->gap_cost, c->start_gap_cost).cell_bits;
}
// the length bound of a batch side: known without measuring (strided, or CSR with max_len given), and its value
static inline bool side_bound_known(const ta_strings *s) { return !s->off || s->max_len; }
static inline uint64_t side_bound(const ta_strings *s) { return s->off ? s->max_len : s->len; }
// the longest string of two sides of na / nb strings: side_bound where it is known, else measured on the device into dst[0] (a) and dst[1]
// (b) -- the caller's two 64-bit words of scratch -- with one copy and one synchronisation for both; no launch for a known side
int measure_max_lens(const ta_strings *a, uint32_t na, const ta_strings *b, uint32_t nb, unsigned long long *dst, hipStream_t st,
                     uint64_t *ma, uint64_t *mb);
// The pairs of a ragged batch in length order (util_kernels.hip: length_order_launch) into the caller's slots; *order_out = the list.
// The histogram must be zero on entry and every complete pass leaves it zero: Scratch::bins_clean of `bins_slot` says this thread's last
// pass over it was complete -- after one that failed midway the histogram is zeroed again (by the graph-safe fill kernel) instead of trusted.
int order_pairs(const ta_strings *a, const ta_strings *b, uint32_t n, uint32_t u, uint64_t max_len, bool by_steps, bool exact,
                ScratchSlot order_slot, ScratchSlot bins_slot, hipStream_t st, const uint32_t **order_out, bool *exact_columns);
// the pointer and size checks every pair-batch entry starts with (bytes: `what` = "null blob", tokens: "null data")
int check_batch_args(const void *a, const void *b, const void *a_data, const void *b_data, size_t n, const void *out, const char *what);
static inline int check_batch_args(const ta_strings *a, const ta_strings *b, size_t n, const void *out) {
    return check_batch_args(a, b, a ? a->blob : nullptr, b ? b->blob : nullptr, n, out, "null blob");
}

// Per-thread context of the single-call host API: its own non-blocking stream (concurrent callers never meet on the null
// stream) and a pinned, device-mapped staging buffer -- a short pair is memcpy'd there, the kernel reads it in place and
// writes the answer back into it: one launch and one stream synchronisation per call, no staging copies.
struct CallCtx {
    static constexpr size_t PIN_BYTES = 64 * 1024, RESULT_OFF = PIN_BYTES - 64;
    hipStream_t st = nullptr;
    uint8_t *pin = nullptr;       // host address
    uint8_t *pin_dev = nullptr;   // the same bytes as the device addresses them
    int ensure();                 // TA_OK / TA_ERR_HIP
    void release();
};
CallCtx &call_ctx();

// What the traceback entries (ta_trace.hip) share with the distance entries (ta_api.hip, where the comments are).  Staged: one (a, b)
// pair of a single call as stage_pair leaves it and fetch_u32 reads its answer back.
constexpr uint32_t TA_SLOT_EMPTY = 0xFFFFFFFEu;    // "no answer yet": distances stay below 0xFFFFFFF0, None is 0xFFFFFFFF
struct Staged {
    ta_strings sa, sb;
    uint32_t *out_dev;             // where the kernel writes
    volatile uint32_t *out_host;   // host view of out_dev (pinned case) or nullptr
    hipStream_t st;
};
int stage_pair(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, Staged *S);
int fetch_u32(const Staged &S, uint32_t *out, bool single_store = false);
int lev_pass(const ta_strings *a, const ta_strings *b, uint32_t n_work, const uint32_t *subset, uint32_t k, const ta_edit_costs *c,
             uint64_t max_len, uint32_t *out_dev, hipStream_t st, bool columns_ordered = false, const uint32_t *n_dev = nullptr);
int batch_max_len(const ta_strings *a, const ta_strings *b, uint32_t n, hipStream_t st, uint64_t *out);
bool stream_is_capturing(hipStream_t s);
ta_launch_info &last_launch();     // the calling thread's record behind ta_last_launch_info

// The batch / *_dev entry points run on the CALLER's stream but keep state in thread-local scratch that their kernels may
// still be using when the call returns.  A later call from the same thread on a DIFFERENT stream first makes that stream
// wait (device-side, hipStreamWaitEvent) for the event recorded at the end of the previous call; calls that stay on one
// stream -- the normal case -- are ordered by the stream itself and cost nothing extra.
struct StreamGuard {
    hipStream_t st;
    bool capturing = false, was_capturing = false;     // the stream is being captured into a graph (Scratch::ensure refuses to grow then)
    explicit StreamGuard(hipStream_t s);
    ~StreamGuard();
};

// test / tuning switches: nullptr / 0 unless TA_TUNING was set when the library was loaded (no getenv on the call path)
bool tuning_enabled();
const char *env_str(const char *name);
int env_int(const char *name);
// the switches of the distance path (lev_route.h), read in this one place; all clear at once without TA_TUNING
LevSwitches lev_switches();

// The table form's host rule (its pure half: lev_bits_tab_applies, lev_plan.h): a launch of the stride-8 line form without transposition
// term, checkpoints, early out or a device-side pair count, of at least LEV_BITS_TAB_MIN_PAIRS pairs.  Under TA_TUNING,
// TA_FORCE_TAB_FORM=1 takes it at any pair count inside its domain and TA_NO_TAB_FORM=1 never takes it.
static inline bool tab_form_wanted(const LevParams &P, const LevBitsPlan &pl, bool trans, bool line_form, bool early, uint64_t max_len) {
    if (early || P.ckpt || P.n_dev) return false;
    return lev_bits_tab_applies(pl, trans, line_form, max_len, P.n, env_int("TA_FORCE_TAB_FORM") != 0, env_int("TA_NO_TAB_FORM") != 0);
}

// ta_set_option(TA_OPT_EARLY_OUT) of the calling thread
bool early_out_enabled();
bool unit_prefilter_enabled();
// true when a HIP device is usable (lazy, cached)
bool device_ready();

// kernels (defined in the .hip files)
// trans: 0 none, 1 dot4-penalty form (2*mc <= 255 + tc), 2 select form
hipError_t lev_band_launch(const LevParams &P, const LevPlan &pl, bool affine, int trans, hipStream_t s,
                           uint32_t *grid_out, uint32_t *lds_out);
hipError_t lev_band_trace_launch(const LevParams &P, const LevPlan &pl, bool affine, bool trans, hipStream_t s);
// batch tracebacks (lev_band.hip): trace kernel over the pairs [P.pair_base, P.pair_base + P.n), then the device-side walk
// (path: n x path_words u32 of scratch, path_words >= (a_len + b_len) / 16 + 1 for every pair)
hipError_t lev_band_trace_batch_launch(const LevParams &P, const LevPlan &pl, bool affine, bool trans, ta_edit *edits, uint32_t *n_edits,
                                       uint64_t cap, uint32_t *path, uint32_t path_words, hipStream_t s);
hipError_t lev_bits_launch(const LevParams &P, const LevBitsPlan &pl, bool trans, uint64_t max_len, hipStream_t s,
                           uint32_t *grid_out, uint32_t *lds_out);
// the table form of the stride-8 line form (lev_bits_tab.hip): what lev_bits_launch hands the batches tab_form_wanted() names
hipError_t lev_bits_tab_launch(const LevParams &P, hipStream_t s, uint32_t *grid_out, uint32_t *lds_out);
// the same at the depth that does not ship (lev_bits_tab_alt.hip): lev_bits_tab_launch's, under TA_TUNING with TA_TAB_DEPTH
hipError_t lev_bits_tab_alt_launch(const LevParams &P, uint32_t grid, uint32_t lds, hipStream_t s);
// the VLINE fetch form (lev_bits_vline.hip): CSR batches through the stride-8 window
hipError_t lev_bits_vline_launch(const LevParams &P, const LevBitsPlan &pl, bool trans, hipStream_t s, uint32_t *grid_out, uint32_t *lds_out);
hipError_t lev_bitsq_launch(const LevParams &P, bool trans, hipStream_t s, uint32_t *grid_out, uint32_t *lds_out);
hipError_t lev_bitsqw_launch(const LevParams &P, bool trans, hipStream_t s, uint32_t *grid_out, uint32_t *lds_out);
hipError_t lev_bits2_launch(const LevParams &P, const LevBits2Plan &pl, bool trans, hipStream_t s, uint32_t *grid_out, uint32_t *lds_out);
hipError_t lev_one_launch(const LevParams &P, bool trans, uint64_t max_len, hipStream_t s, uint32_t *lds_out);
bool lev_sliced_applies(const StrView &a, const StrView &b, uint32_t unit_k, uint32_t *strips_out);
hipError_t lev_sliced_launch(const StrView &a, const StrView &b, uint32_t n, uint32_t k, uint32_t unit_k, uint32_t *out,
                             hipStream_t st, uint32_t *grid_out, uint32_t *lds_out, uint32_t *pairs_per_wave);
hipError_t lev_widebits_launch(const LevParams &P, int rows_per_lane, uint64_t max_len, bool trans, hipStream_t s,
                               uint32_t *grid_out, uint32_t *lds_out);
hipError_t lev_widebits_huge_launch(const uint8_t *a, uint32_t a_len, const uint8_t *b, uint32_t b_len, uint32_t u, uint32_t k,
                                    int rows_per_lane, bool trans, uint32_t *out, hipStream_t s, uint32_t *launches_out);
hipError_t lev_wide_trace_launch(const LevParams &P, bool trans, hipStream_t s);
hipError_t lev_widebits_trace_launch(const LevParams &P, bool trans, hipStream_t s);
hipError_t lev_wide_launch(const LevParams &P, bool trans, hipStream_t s, uint32_t *grid_out, uint32_t *lds_out,
                           uint32_t *threads_out, uint32_t *dpt_out);
// the DP wide kernel over 32-bit items (token batches' overflow pairs): P.subset / P.n_dev as a list, or P.n pairs; trace: one pair
hipError_t lev_wide_u32_launch(const LevParams &P, bool trans, bool trace, hipStream_t s);
struct SymCompactParams;
hipError_t sym_compact_launch(const SymCompactParams &P, uint32_t waves, hipStream_t s);
hipError_t hamming_batch_launch(const StrView &a, const StrView &b, uint32_t n, uint32_t *out, hipStream_t s);
// hamming of long strings (ham_long.hip): every pair cut into slices, one wavefront per slice; scratch = ham_long_scratch_words() u32
// (0: the batch has more than 2^31 slices and stays on hamming_batch_kernel).  The chunk / sum pair serves a host pair that is staged piece by piece.
uint64_t ham_long_scratch_words(const StrView &a, const StrView &b, uint32_t n, uint32_t S0);
hipError_t ham_long_launch(const StrView &a, const StrView &b, uint32_t n, uint32_t S0, uint32_t *scratch, uint32_t *out, hipStream_t st);
hipError_t ham_long_chunk_launch(const uint8_t *a, const uint8_t *b, uint64_t len, uint32_t S, uint32_t *partial, hipStream_t st);
hipError_t ham_long_sum_launch(const uint32_t *partial, uint32_t n_partial, uint32_t *out, hipStream_t st);
uint32_t ham_slice_setting();      // HAM_LONG_SLICE, or TA_HAM_SLICE under TA_TUNING
constexpr size_t HAM_HOST_CHUNK = 64ull << 20;     // ta_hamming: bytes of each host string on the device at a time
hipError_t strings_maxlen_launch(const StrView &s, uint32_t n, uint32_t *out_max /*device, pre-zeroed*/, hipStream_t st);
hipError_t compact_none_launch(const uint32_t *out, const uint32_t *subset_in, uint32_t n_in, const uint32_t *n_in_dev /*optional: the list's length on the device*/,
                               uint32_t *subset_out, uint32_t *count, hipStream_t st);
// batch tracebacks of the unit-cost families by checkpoints + recomputation (lev_bits_trace.hip; bands of up to 33 diagonals)
uint32_t lev_bits_trace_ckpt_words(bool trans);
uint32_t lev_bits_trace_tile();
hipError_t lev_bits_trace_launch(const LevBitsTraceParams &P, bool trans, bool have_ckpt, ta_edit *edits, uint32_t *n_edits, uint64_t cap, hipStream_t s,
                                 uint32_t *grid_out, uint32_t *lds_out);
hipError_t fill_u32_launch(uint32_t *p, uint32_t v, uint32_t n, hipStream_t st);   // p[0..n) = v, as a kernel (graph-safe)
hipError_t compact_some_launch(const uint32_t *out, const uint32_t *subset_in, uint32_t n_in, uint32_t *subset_out, uint32_t *count /*device, pre-zeroed*/, hipStream_t st);
hipError_t scale_results_launch(uint32_t *out, const uint32_t *list /*pairs, or nullptr: 0..n*/, uint32_t n, const uint32_t *n_dev, uint32_t g, hipStream_t st);
hipError_t pack_edits_launch(const ta_edit *edits, const uint32_t *n_edits, uint32_t n, uint64_t cap_in, uint32_t *packed, uint64_t cap_out, hipStream_t st);
hipError_t compact_bound_launch(const uint32_t *out, const uint32_t *bound, uint32_t k, const uint32_t *list_in, uint32_t n_in,
                                const uint32_t *n_in_dev, uint32_t *list_out, uint32_t *count, hipStream_t st);
hipError_t bag_bound_launch(const StrView &a, const StrView &b, uint32_t n, uint32_t mc, uint32_t gc, uint32_t *bound, hipStream_t st);
hipError_t hits_best_launch(const ta_match *hits, uint64_t n, uint32_t *min_k /*device, preset to ~0*/, ta_match *out, uint32_t cap,
                            uint32_t *count /*device, pre-zeroed*/, hipStream_t st);
// counting sort of the pairs of a ragged batch by length class (util_kernels.hip): subset_out = the pairs (of subset_in, or
// 0..n) ordered so that 64 consecutive ones are within a few bytes of each other; bins = 2 x 32768 u32 of device scratch, the
// first half zero on entry (it is zero again on exit); *exact_columns: 64 consecutive pairs of the order share their exact column count
hipError_t length_order_launch(const StrView &a, const StrView &b, const uint32_t *subset_in, uint32_t n, uint32_t u, uint64_t max_len, bool by_steps,
                               uint32_t *bins, uint32_t *subset_out, hipStream_t st, bool exact = false, bool *exact_columns = nullptr);

struct SearchParams {
    const uint8_t *hay;       // device
    uint64_t hay_len;
    uint8_t needle[64];       // by value (kernarg): the lane-per-tile register kernels read it as scalars (needles <= 32), the
                              // wavefront-per-block kernel one byte per lane straight from the kernarg segment (needles <= 64)
    const uint8_t *needle_dev;   // device copy (any length)
    uint32_t *col_scratch;    // memory-backed column (long needles)
    uint32_t needle_len;
    uint32_t k, mc, gc, sg, tc;
    uint32_t anchored;
    uint32_t halo;            // bytes of left context each tile recomputes
    uint32_t tile;            // haystack positions emitted per lane
    uint64_t base, emit_from;
    ta_match *hits;           // device
    uint64_t cap;
    unsigned long long *count;   // device
};
hipError_t lev_search_launch(const SearchParams &P, bool packed, bool trans, hipStream_t s);
hipError_t lev_filter_launch(const SearchParams &P, bool trans, uint32_t *list, uint32_t list_cap, unsigned int *list_count,
                             hipStream_t s);
hipError_t lev_search_list_launch(const SearchParams &P, bool trans, const uint32_t *list, uint32_t n_list, hipStream_t s);

// Device-side control block of one filtered search pass (zeroed by ONE memset) and the report its last wavefront writes
// into host-mapped pinned memory: the host learns everything it needs from one stream synchronisation, with no copy and
// no round trip between the filter and the exact kernel.
constexpr uint32_t SEARCH_DONE_GROUPS = 16;
struct SearchCtl {
    unsigned long long count;     // hits emitted (may exceed the caller's cap)
    uint32_t n_list;              // 64-column blocks the filter flagged
    uint32_t pad0;
    uint32_t done2;               // groups of workgroups that have finished (the last one writes the report)
    uint32_t pad1;
    uint32_t pad[10];             // [0], [1]: timestamps of wavefront 0
    uint32_t done[SEARCH_DONE_GROUPS * 16];   // finished workgroups per group, one counter per 64-byte line: 512 bumps of ONE address
                                  // serialise at the memory side (~70 ns each); 16 lines of 32 run side by side
};
struct SearchReport {             // 64 bytes, followed by up to SEARCH_REPORT_SEL selected ta_match records (Best passes)
    uint64_t count;
    uint32_t n_list;
    uint32_t dense;               // 1: too many flagged blocks -- nothing was searched, the lane-per-tile kernel must run over everything
    uint32_t sel_count;           // Best: hits with the smallest k ...
    uint32_t sel_state;           // ... 1: all of them follow this header, 2: too many to select here (use ta_search_best_hits_dev)
    uint32_t min_k;
    uint32_t n_slots;
    uint32_t t[8];                // 100 MHz timestamps (s_memrealtime, low dword): [0] wavefront 0 enters, [1] it has finished its blocks,
                                  // [2] the last workgroup starts the report, [3] ... has written it   (scripts/measure_search_parts.py)
};
// Best passes: one slot per flagged block
struct SearchSlot {
    uint32_t min_cost, cnt;       // the block's best cost and its number of hits (0: none -- the slot is as the fill left it)
    uint64_t idx0;                // its hits are hits[idx0 .. idx0 + cnt)
};
constexpr uint32_t SEARCH_SLOT_CAP = 1u << 18;                                      // flagged blocks a fused Best pass handles (4 MiB of slots)
constexpr uint32_t SEARCH_REPORT_SEL = 680;                                         // 64 + 680 * 24 = 16 KiB
constexpr size_t SEARCH_REPORT_BYTES = 64 + (size_t)SEARCH_REPORT_SEL * sizeof(ta_match);
// thread-local pinned, device-mapped landing zone of the report
struct PinBox {
    uint8_t *host = nullptr, *dev = nullptr;
    int ensure();                 // TA_OK / TA_ERR_HIP
    void release();
};
PinBox &search_report_box();
void search_resident_reset();        // forget what ta_levenshtein_search_first left in the haystack staging buffer (ta_search.hip)
// one wavefront per flagged block (lev_search_wave_body.h), persistent grid reading n_list on the device; needles <= 64 bytes
hipError_t lev_search_wave_launch(const SearchParams &P, bool trans, bool best, const uint32_t *list, uint32_t cap_list,
                                  SearchCtl *ctl, SearchSlot *slots /* SEARCH_SLOT_CAP of them; Best passes */, uint8_t *report_dev,
                                  hipStream_t s);
// util_kernels.hip: a search's count, NUL flag and (few) hits into the report box; *flag != 0 iff p[0 .. len) holds a zero byte
hipError_t search_report_copy_launch(const unsigned long long *count, const uint32_t *nul_flag, const ta_match *hits, uint64_t cap, uint8_t *box, hipStream_t s);
hipError_t has_zero_byte_launch(const uint8_t *p, uint64_t len, uint32_t *flag, hipStream_t s);
// ham_search.hip: the kernel `route` names (ham_search_plan.h; P.needle_dev set where it needs it).  nul_flag: nullptr = no check wanted
struct HamSearchRoute;
hipError_t hamming_search_launch(const SearchParams &P, const HamSearchRoute &route, hipStream_t s, uint32_t *nul_flag = nullptr);

// ta_levenshtein_search_batch (lev_search_batch.hip): one lane per (needle, haystack) pair
struct SearchBatchParams {
    StrView nd, hs;               // needles (the strided form with stride 0: one shared needle), haystacks
    ta_match *matches;            // device: cap slots per pair
    uint32_t *counts;             // device: the length of each pair's result
    uint64_t cap;
    uint32_t n;                   // pairs (the grid's bound)
    const uint32_t *list;         // the pairs in the order they are taken, or nullptr: 0..n
    const uint32_t *n_list;       // device: the list's length (Route S's candidates), or nullptr: n
    uint32_t *span;               // Route S: [2 pair], [2 pair + 1] = first and last candidate end; nullptr: Route E
    uint32_t *cand_list, *cand_count;   // Route S scan: the pairs with a candidate, their number (pre-zeroed)
    uint32_t k, mc, gc, sg, tc, anchored, best;
    uint32_t kf, halo;            // Route S: the scan's threshold, the exact pass's left context
    uint32_t max_needle;          // bound on every needle's length (the packed form: the needle's length)
    uint32_t *col;                // memory form: 6 (max_needle + 1) u32 per resident lane
};
hipError_t search_batch_maxlen_launch(const StrView &nd, const StrView &hs, uint32_t n, unsigned long long *max /*2, pre-zeroed*/, hipStream_t st);
hipError_t search_batch_exact_launch(const SearchBatchParams &P, bool trans, bool packed, uint32_t mem_lanes, hipStream_t st);
hipError_t search_batch_scan_launch(const SearchBatchParams &P, bool trans, hipStream_t st);

// ta_hamming_search_batch (ham_search_batch.hip): one lane per (needle, haystack) pair
struct HamBatchParams {
    StrView nd, hs;               // needles (the strided form with stride 0: one shared needle), haystacks
    ta_match *matches;            // device: cap slots per pair
    uint32_t *counts;             // device: the length of each pair's result, TA_NONE for a haystack with a NUL byte
    uint64_t cap;
    uint32_t n;                   // pairs
    const uint32_t *list;         // the pairs in the order they are taken, or nullptr: 0..n
    uint32_t k, best;
    uint32_t max_needle;          // bound on every needle's length (the bit-sliced form: the shared needle's length)
};
// bits: the bit-sliced form (a shared needle of 1..32 bytes, 4 k <= its length); else the register form up to 64 bytes, the memory form beyond
hipError_t ham_search_batch_launch(const HamBatchParams &P, bool bits, hipStream_t st);

// ta_levenshtein_cross, ta_levenshtein_cross_with_opts (lev_cross.hip, lev_cross_win.hip): one lane per target, a wavefront walks a
// tile of queries
struct CrossParams {
    StrView q, t;                 // queries (every one at most 32 nw bytes; the window kernel: 256), targets
    uint32_t nq, nt;
    uint32_t k, g;                // the unit threshold; distances are reported times g (lev_cost_scale)
    uint32_t qtile;               // queries per wavefront: ceil(nq / qtile) <= 65535
    uint32_t flags;               // TA_CROSS_UPPER: only pairs with target index > query index
    ta_cross_hit *hits;           // device: cap records, or nullptr with cap = 0
    uint64_t cap;
    unsigned long long *count;    // device, pre-zeroed
    unsigned long long *nearest;  // device: nq words preset to all ones, or nullptr
    uint32_t *per_query;          // device: nq words pre-zeroed, or nullptr
};
constexpr uint32_t CROSS_MIN_QTILE = 16;
hipError_t lev_cross_launch(const CrossParams &P, int nw, bool trans, hipStream_t st);
// queries of up to 256 bytes: a window of ww = 2, 3, 4 blocks of the column, or all 8 (ww >= win_ww(P.k), lev_cross_win_body.h)
hipError_t lev_cross_win_launch(const CrossParams &P, int ww, bool trans, hipStream_t st);
// ta_levenshtein_cross_tokens (lev_cross_tok.hip): P.q / P.t over 32-bit items -- blob = the first item; off, stride and len in ELEMENTS;
// queries of at most 32 nw items
hipError_t lev_cross_tok_launch(const CrossParams &P, int nw, bool trans, hipStream_t st);

// ta_hamming_cross (ham_cross.hip): one lane per target, kept in nw dwords of registers; a wavefront walks a tile of queries, staged
// through LDS a chunk of 256 / nw at a time
struct HamCrossParams {
    StrView q, t;                 // queries (every one at most 4 nw bytes), targets
    uint32_t nq, nt;
    uint32_t k8;                  // 8 min(k, 64) + 7: the compare counts eight per mismatch
    uint32_t upper;               // TA_CROSS_UPPER: only pairs with target index > query index
    uint32_t qtile;               // queries per wavefront: ceil(nq / qtile) <= 65535
    ta_cross_hit *hits;           // device: cap records, or nullptr with cap = 0
    uint64_t cap;
    unsigned long long *count;    // device, pre-zeroed
    unsigned long long *nearest;  // device: nq words preset to all ones, or nullptr
    uint32_t *per_query;          // device: nq words pre-zeroed, or nullptr
};
hipError_t ham_cross_launch(const HamCrossParams &P, int nw, hipStream_t st);

// ta_levenshtein_search_cross and ta_levenshtein_search_cross_with_opts (lev_search_cross.hip; needles beyond 32 bytes:
// lev_search_cross_w2.hip; what the kernels of both share: search_cross_dev.h): every needle of a panel in every haystack, one
// sub-batch of haystacks per launch
struct SxRec;
struct SearchCrossParams {
    StrView nd, hs;               // needles (every one at most 32 bytes; the two-word route: 64), haystacks
    uint32_t nn;
    uint32_t h0, h1;              // the sub-batch: haystacks [h0, h1)
    uint32_t hpw;                 // haystacks per scan workgroup
    uint32_t k, mc, gc, sg, tc, anchored;
    uint32_t kf, halo;            // the scan's threshold, the exact pass's left context
    uint32_t max_needle;          // bound on every needle's length (the packed form: every needle's length)
    SxRec *rec;                   // device: the sub-batch's records (scan: the candidate list; anchored: one per (haystack, needle))
    uint32_t *n_rec;              // device: the list's length (pre-zeroed), or nullptr: anchored, (h1 - h0) * nn records
    ta_search_cross_hit *hits;    // device: cap records, or nullptr with cap = 0
    uint64_t cap;
    unsigned long long *count;    // device, pre-zeroed
    unsigned long long *nearest;  // device: nh words preset to all ones, or nullptr
    uint32_t *per_haystack;       // device: nh words pre-zeroed, or nullptr
    ta_match *best;               // device: nh records preset to {0, 0, TA_NONE, 0}, or nullptr
    uint32_t *col;                // the two-word route: device, col_lanes memory-backed columns of 6 x 65 words (element-major), else nullptr
    uint32_t col_lanes;           // ... the exact pass's grid in lanes, a multiple of 256
};
hipError_t search_cross_init_best_launch(ta_match *best, uint32_t nh, hipStream_t st);
hipError_t search_cross_scan_launch(const SearchCrossParams &P, bool trans, hipStream_t st);
hipError_t search_cross_exact_launch(const SearchCrossParams &P, bool trans, bool packed, hipStream_t st);
hipError_t search_cross_finish_launch(const SearchCrossParams &P, hipStream_t st);
hipError_t search_cross_w2_scan_launch(const SearchCrossParams &P, bool trans, hipStream_t st);
hipError_t search_cross_w2_exact_launch(const SearchCrossParams &P, bool trans, hipStream_t st);

// ta_hamming_search_cross and ta_hamming_search_cross_with_opts (ham_search_cross.hip; needles beyond 32 bytes: ham_search_cross_w2.hip;
// what the two kernels share: search_cross_dev.h): every needle of a panel in every haystack, substitutions only, in one launch
struct HamSearchCrossParams {
    StrView nd, hs;               // needles (every one at most 32 bytes; the two-word route: 64), haystacks
    uint32_t nn, nh;
    uint32_t hpw;                 // haystacks per workgroup
    uint32_t kc;                  // min(k, longest needle): the counters' threshold (ham_search_cross_body.h: hsx_threshold)
    ta_search_cross_hit *hits;    // device: cap records, or nullptr with cap = 0
    uint64_t cap;
    unsigned long long *count;    // device, pre-zeroed
    unsigned long long *packed;   // device: nh packed words preset to all ones, or nullptr: neither nearest nor best is asked for
    uint32_t *per_haystack;       // device: nh words pre-zeroed, or nullptr
    unsigned long long *nearest;  // device: nh words the finish kernel writes, or nullptr
    ta_match *best;               // device: nh records the finish kernel writes, or nullptr
};
hipError_t ham_search_cross_launch(const HamSearchCrossParams &P, hipStream_t st);
hipError_t ham_search_cross_w2_launch(const HamSearchCrossParams &P, hipStream_t st);   // a longest needle of 33..64 bytes (ham_search_cross_w2.hip)
hipError_t ham_search_cross_finish_launch(const HamSearchCrossParams &P, hipStream_t st);

// ta_multi.hip: the device set (one worker thread per entry).  multi_search_shards / multi_pair_shards: over how many of them a host
// haystack / a host batch of that size is spread (1: the calling thread's own device path).  The search forms return the All-mode hits
// sorted by end (best: only those with each shard's smallest k -- all the Best fold can keep), without the end == 0 match.
size_t multi_search_shards(size_t haystack_len);
size_t multi_pair_shards(size_t n);
int multi_levenshtein_search_host(const uint8_t *needle, size_t n, const uint8_t *hay, size_t h, uint32_t k, bool best, const ta_edit_costs *costs,
                                  std::vector<ta_match> &hits);
int multi_hamming_search_host(const uint8_t *needle, size_t n, const uint8_t *hay, size_t h, uint32_t k, bool check_nul, std::vector<ta_match> &hits);
// ta_hamming_search_dev under the scalar routine's contract (NUL bytes are fine, src/hamming.rs:96-146)
int hamming_search_dev_nocheck(const uint8_t *needle_host, size_t needle_len, const uint8_t *haystack_dev, size_t haystack_len, uint32_t k,
                               uint64_t base, ta_match *hits_dev, size_t cap, uint64_t *count_host, void *stream);

}  // namespace ta
