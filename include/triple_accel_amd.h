/*
 * triple_accel_amd.h -- C ABI of the MI355X-native edit-distance engine.
 *
 * Drop-in boundary for triple_accel's hot path.  The reference
 * (Rust, /root/reference) has no FFI of its own; each entry point below names the
 * reference function (file:line) it replaces, and INTEGRATION.md shows the Rust
 * `extern "C"` shim that maps the reference's public signatures onto it.
 *
 * Conventions
 *   - plain pointers + sizes, no C++/torch types; every function returns a ta_status.
 *   - Rust panics become status codes (the shim re-raises them): TA_ERR_LEN_MISMATCH,
 *     TA_ERR_NULL_BYTE, TA_ERR_BAD_COSTS.  Option::None becomes the sentinel TA_NONE
 *     (a real distance never reaches it: the reference clamps k to a true upper bound,
 *     src/levenshtein.rs:734-757).
 *   - `*_dev` / `*_batch` functions take DEVICE (HBM) pointers and a hipStream_t passed as
 *     void*; they enqueue work and return without synchronising unless stated.  The plain
 *     functions take HOST pointers, run on the current HIP device and synchronise -- except
 *     where the DEVICE SET takes over (ta_set_devices below: host batches, the queue, searches
 *     over big haystacks are partitioned over every device of the set inside the library).
 *   - Device string blobs must be readable for TA_BLOB_SLACK bytes past their last byte
 *     (kernels fetch 16-byte pieces).
 *   - There is NO CPU fallback: with no HIP device every compute entry point returns
 *     TA_ERR_HIP.
 */
#ifndef TRIPLE_ACCEL_AMD_H
#define TRIPLE_ACCEL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TA_NONE 0xFFFFFFFFu
#define TA_BLOB_SLACK 16

typedef enum {
    TA_OK = 0,
    TA_ERR_LEN_MISMATCH = 1, /* assert!(a.len() == b.len())     src/hamming.rs:38,318 */
    TA_ERR_NULL_BYTE = 2,    /* check_no_null_bytes panic        src/lib.rs:237-243    */
    TA_ERR_BAD_COSTS = 3,    /* EditCosts::new / check_search    src/levenshtein.rs:44-52,67-71 */
    TA_ERR_HIP = 4,          /* HIP runtime failure / no device (no CPU fallback) */
    TA_ERR_ARG = 5,          /* null pointer, size over the documented limit */
    TA_ERR_UNSUPPORTED = 6,  /* outside what the GPU path covers (e.g. a traceback needing more than 8 GB of records) */
    TA_ERR_CAPACITY = 7,     /* caller-provided match buffer too small; *n_out holds the need */
    TA_ERR_DIV_ZERO = 8      /* "attempt to divide by zero": hamming_search_naive*, empty needle, Best  src/hamming.rs:136 */
} ta_status;

/* EditCosts, src/levenshtein.rs:20-26 (fields are private there; built via new / the consts) */
typedef struct {
    uint8_t mismatch_cost;
    uint8_t gap_cost;
    uint8_t start_gap_cost;
    uint8_t has_transpose;  /* Option<u8>::is_some() */
    uint8_t transpose_cost;
} ta_edit_costs;

/* Match, src/lib.rs:135-142 (start inclusive, end exclusive) */
typedef struct {
    uint64_t start;
    uint64_t end;
    uint32_t k;
    uint32_t pad_;
} ta_match;

/* Edit / EditType, src/lib.rs:148-165 */
typedef enum { TA_EDIT_MATCH = 0, TA_EDIT_MISMATCH = 1, TA_EDIT_AGAP = 2, TA_EDIT_BGAP = 3, TA_EDIT_TRANSPOSE = 4 } ta_edit_type;
typedef struct {
    uint32_t edit;   /* ta_edit_type */
    uint32_t pad_;
    uint64_t count;
} ta_edit;

/* SearchType, src/lib.rs:171-174 */
typedef enum { TA_SEARCH_ALL = 0, TA_SEARCH_BEST = 1 } ta_search_type;

/* LEVENSHTEIN_COSTS / RDAMERAU_COSTS, src/levenshtein.rs:76-89 */
ta_edit_costs ta_levenshtein_costs(void);
ta_edit_costs ta_rdamerau_costs(void);
/* EditCosts::new validation, src/levenshtein.rs:38-60: TA_OK or TA_ERR_BAD_COSTS */
int ta_edit_costs_new(uint8_t mismatch, uint8_t gap, uint8_t start_gap, int has_transpose, uint8_t transpose,
                      ta_edit_costs *out);
/* check_search, src/levenshtein.rs:67-71 */
int ta_edit_costs_check_search(const ta_edit_costs *c);

/* ---- runtime ------------------------------------------------------------------------- */
const char *ta_version(void);
const char *ta_status_str(int status);
/* Options of the calling thread (0 = off, the default).
 *   TA_OPT_EARLY_OUT: the bit-parallel band kernels of fixed-length unit-cost batches (bands of up to 33 diagonals) stop a
 *   wavefront as soon as none of its pairs can still end at or below k (the top cell of the current band column minus the
 *   downward steps below it -- a lower bound of every cell of the column -- exceeds k; checked every 24-32 columns).  The answers are the same -- those pairs are None either way
 *   (src/levenshtein.rs:539-541) -- but the work then depends on the data: batches of dissimilar strings finish after a few
 *   dozen columns.  Off by default: the reference evaluates its whole band, and so does every benchmark figure of this library.
 *   TA_OPT_UNIT_PREFILTER: batches under weighted EditCosts (ta_levenshtein_k_batch, >= 1024 pairs) first run the unit-cost bit-parallel
 *   pass with k' = max(k / min(mc, tc), (k - sg) / min(mc, gc, tc)): a pair whose UNIT distance exceeds k' has a weighted distance above k --
 *   None (src/levenshtein.rs:539-541) -- and only the others are priced by the DP band kernel with the real costs.  Same answers; the work
 *   depends on the data (dissimilar batches: the unit pass alone, 0.3 of the weighted pass; near pairs: both).  Off by default. */
enum { TA_OPT_EARLY_OUT = 1, TA_OPT_UNIT_PREFILTER = 2 };
int ta_set_option(int option, int value);
/* number of visible HIP devices (0 => every compute call returns TA_ERR_HIP) */
int ta_device_count(void);
/* text of the last HIP error seen on this thread ("" if none) */
const char *ta_last_error(void);
/* the dominant kernel of the calling thread's last pass, as a profiler prints it (no "void ta::", no parameter list); "" before the first pass */
const char *ta_last_kernel_name(void);

/* The dispatcher arithmetic of levenshtein_simd_k_with_opts, src/levenshtein.rs:731-791:
 * clamped max_k, unit_k, and the cell width (8/16/32 bits) the reference would pick.
 * The GPU kernels keep u8/u16/u32 *semantics* by this rule (DESIGN.md "cell width"). */
typedef struct {
    uint32_t max_k;
    uint32_t unit_k;
    uint32_t cell_bits;       /* 8, 16 or 32 */
    uint32_t ref_lanes;       /* 32/64/128/256 for the u8 Jewel types, 0 for the Vec-backed ones */
} ta_lev_select;
int ta_levenshtein_select(size_t a_len, size_t b_len, uint32_t k, const ta_edit_costs *costs, ta_lev_select *out);

/* What the last distance batch launched on this thread used (for tests / debug logging;
 * the analogue of the reference's `debug` feature println, src/levenshtein.rs:840-847). */
typedef struct {
    uint32_t kernel;          /* 1 = band-wavefront (registers+DPP), 2 = wide-band workgroup, 3 = bit-parallel band (unit costs), 4 = bit-parallel full columns (unit costs, long pairs), 5 = pair-sliced systolic band (EXPERIMENTAL builds), 6 = single pair, band <= 64 diagonals (unit costs), 7 = small-alphabet bit-parallel band (ta_levenshtein_k_batch_alphabet), 8 = checkpoint-and-recompute traceback of the unit-cost families (ta_levenshtein_trace_batch, bands of up to 33 diagonals); pairs_per_wave 128 with kernel 3 = two pairs per lane */
    uint32_t diags_per_lane;  /* D */
    uint32_t lanes_per_pair;  /* L */
    uint32_t pairs_per_wave;
    uint32_t band_offset;     /* o: diagonal index of d = 0 */
    uint32_t cell_bits;       /* width class chosen by the reference's rule for the batch's max lengths */
    uint32_t affine;
    uint32_t transpose;
    uint32_t grid;
    uint32_t lds_bytes;
} ta_launch_info;
int ta_last_launch_info(ta_launch_info *out);

/* ---- single-call host API (the reference's function set) ------------------------------- */

/* hamming(a, b), src/hamming.rs:390 -> :317 -> :36-47.  A pair of more than 64 MiB per string is staged through the device 64 MiB at
 * a time (the device holds two such pieces whatever the pair's length); a pair of 64 KiB or more is sliced over the chip. */
int ta_hamming(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t *out);

/* levenshtein_simd_k_with_opts(a, b, k, trace_on, costs), src/levenshtein.rs:714-720.
 * *out = distance, or TA_NONE when the distance exceeds k.  trace_on != 0 -> TA_ERR_UNSUPPORTED here: the traceback
 * has its own entry point, ta_levenshtein_trace, because it returns an edit script. */
int ta_levenshtein_simd_k_with_opts(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len,
                                    uint32_t k, int trace_on, const ta_edit_costs *costs, uint32_t *out);
/* levenshtein_simd_k_with_opts(a, b, k, true, costs): distance + run-length traceback (library-owned, ta_free).
 * 2-bit argmin codes come from the band-wavefront kernel; the walk is host code.  Bands wider than 4222 diagonals
 * (unit_k > 4220): the unit-cost families use the row-blocked bit-parallel kernel with 3-bit records, other costs the DP
 * wide kernel with 2-bit codes; more than 8 GB of records returns TA_ERR_UNSUPPORTED. */
int ta_levenshtein_trace(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t k,
                         const ta_edit_costs *costs, uint32_t *out, ta_edit **edits, size_t *n_edits);
/* levenshtein_exp_with_opts(a, b, true, costs), src/levenshtein.rs:1480-1494 */
int ta_levenshtein_exp_trace(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len,
                             const ta_edit_costs *costs, uint32_t *out, ta_edit **edits, size_t *n_edits);
/* levenshtein_simd_k, src/levenshtein.rs:677-684 */
int ta_levenshtein_simd_k(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t k, uint32_t *out);
/* levenshtein, src/levenshtein.rs:1397 ; rdamerau :1419 */
int ta_levenshtein(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t *out);
int ta_rdamerau(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t *out);
/* levenshtein_exp :1445, levenshtein_exp_with_opts :1480 (trace_on unsupported), rdamerau_exp :1516 */
int ta_levenshtein_exp(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t *out);
int ta_levenshtein_exp_with_opts(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len,
                                 int trace_on, const ta_edit_costs *costs, uint32_t *out);
int ta_rdamerau_exp(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t *out);

/* levenshtein_search_simd_with_opts(needle, haystack, k, search_type, costs, anchored),
 * src/levenshtein.rs:1911-1918.  This entry returns the whole result: *out is library-owned (release with ta_free), *n_out its
 * length.  The reference's iterator is lazy; ta_levenshtein_search_first (below) is its `.next()`. */
int ta_levenshtein_search_simd_with_opts(const uint8_t *needle, size_t needle_len,
                                         const uint8_t *haystack, size_t haystack_len,
                                         uint32_t k, int search_type, const ta_edit_costs *costs, int anchored,
                                         ta_match **out, size_t *n_out);
/* levenshtein_search, src/levenshtein.rs:2508 (k = ceil(n/2), Best, LEVENSHTEIN_COSTS, unanchored) */
int ta_levenshtein_search(const uint8_t *needle, size_t needle_len, const uint8_t *haystack, size_t haystack_len,
                          ta_match **out, size_t *n_out);
/* hamming_search_simd_with_opts, src/hamming.rs:454 ; hamming_search :588 */
int ta_hamming_search_simd_with_opts(const uint8_t *needle, size_t needle_len,
                                     const uint8_t *haystack, size_t haystack_len,
                                     uint32_t k, int search_type, ta_match **out, size_t *n_out);
int ta_hamming_search(const uint8_t *needle, size_t needle_len, const uint8_t *haystack, size_t haystack_len,
                      ta_match **out, size_t *n_out);
/* hamming_search_naive_with_opts, src/hamming.rs:96-146 (and hamming_search_naive :70 with k = ceil(n/2), Best): the scalar
 * routine's contract -- no NUL-byte panic, an empty needle matches with k = 0 at every offset 0..=haystack_len. */
int ta_hamming_search_naive_with_opts(const uint8_t *needle, size_t needle_len,
                                      const uint8_t *haystack, size_t haystack_len,
                                      uint32_t k, int search_type, ta_match **out, size_t *n_out);
/* The FIRST element of levenshtein_search_simd_with_opts(.., SearchType::All, ..): what `.next()` on the reference's lazy
 * iterator returns (src/levenshtein.rs:2282-2420; tests/basic_tests.rs:628-632) without scanning the rest of the haystack.
 * The haystack is searched window by window (64 KiB, then four times as much each time, each window behind needle_len +
 * unit_k + 2 bytes of left context -- exact for every cost <= k) and the scan stops at the first window that holds a hit;
 * the host form also uploads only that far.  *found = 0 when there is no match at all.  The bindings' All-mode iterators
 * call this for their first element and run the full search only when a second one is asked for. */
int ta_levenshtein_search_first(const uint8_t *needle, size_t needle_len, const uint8_t *haystack, size_t haystack_len,
                                uint32_t k, const ta_edit_costs *costs, int anchored, ta_match *out, int *found);
/* The All-mode result for a caller that has just taken its first element with ta_levenshtein_search_first on THE SAME haystack (same pointer
 * and length, bytes unchanged: the caller's promise -- the bindings' lazy iterators hold the haystack immutable): the bytes that call uploaded
 * stay on the device, only the rest travels (src/levenshtein.rs:2282-2420: the reference's lazy iterator continues where it stopped).  After
 * any other call of the thread it is ta_levenshtein_search_simd_with_opts(.., TA_SEARCH_ALL, ..). */
int ta_levenshtein_search_resume(const uint8_t *needle, size_t needle_len, const uint8_t *haystack, size_t haystack_len,
                                 uint32_t k, const ta_edit_costs *costs, int anchored, ta_match **out, size_t *n_out);
/* the same over a haystack shard resident in HBM (positions + base; the end == 0 match is the caller's, as with *_search_dev) */
int ta_levenshtein_search_first_dev(const uint8_t *needle_host, size_t needle_len,
                                    const uint8_t *haystack_dev, size_t haystack_len,
                                    uint32_t k, const ta_edit_costs *costs, uint64_t base,
                                    ta_match *out, int *found, void *stream);
/* Limits of the host search forms: needles up to 65,535 bytes (TA_ERR_ARG beyond); the result list is bounded only by memory
 * (a pass that overflows its first hit buffer is repeated once with room for the count it reported). */
void ta_free(void *p);

/* Threading.  Every entry point may be called from any number of threads at once.  The single-call host functions
 * (ta_hamming .. ta_levenshtein_exp, the *_search host forms, the tracebacks) run on a stream the library keeps per calling
 * thread (non-blocking: concurrent callers never serialise on the null stream) and stage short pairs through a pinned,
 * device-mapped buffer of that thread -- one kernel launch and one stream synchronisation per call.  The batch / *_dev
 * functions run on the stream the caller passes; a thread that switches streams between two such calls is ordered by an
 * event the library records at the end of each call (the thread-local scratch of the first call may still be in use).
 * The single-call functions are ordered after the thread's earlier batch / *_dev calls in the same way: their stream waits for
 * that event before it touches the scratch they share with them (tests/test_gpu_stream_order.py holds every entry to this).
 * ta_thread_release() frees what the calling thread holds inside the library (device scratch, its stream, the pinned
 * buffer); optional -- without it they live until process exit.
 * Graph capture.  The batch / *_dev entries that say so may be captured into a hipGraph (hipStreamBeginCapture on the stream they are given).
 * A captured call bakes the calling thread's scratch pointers into the graph: run the same call once OUTSIDE the capture first (it sizes the
 * scratch); a call that would have to grow the scratch during a capture returns TA_ERR_UNSUPPORTED instead of allocating.  The graph is
 * invalid after any later call of the thread that grows the scratch (a bigger batch, a wider band) and after ta_thread_release(). */
void ta_thread_release(void);

/* ---- batch API on device-resident data (new surface; N = 1 equals the single-call form) -- */

/* String i of a batch is blob[off[i] .. off[i+1]) (CSR, n+1 offsets, device memory), or, when
 * off == NULL, blob[i*stride .. i*stride+len) (fixed length `len`, byte stride `stride`).
 * What the layout may be (tests/test_gpu_layouts.py holds every device entry to it, on every kernel route):
 *   - `blob` may have any byte alignment, and may point into the middle of an allocation;
 *   - `stride` and `len` are independent: stride > len leaves gaps between the strings, stride < len makes the strings overlapping
 *     windows of one sequence; stride = 0 is ONE string shared by every pair (documented for the needles of the two *_search_batch
 *     entries; the other entries then compare that one string n times);
 *   - CSR offsets need not start at 0 and `off` may point into the middle of a larger batch's offsets: only off[0 .. n] are read, and
 *     only blob[off[0] .. off[n]) belongs to the batch;
 *   - the bytes that belong to no string -- in front of the blob, in the gaps of the strided form, the TA_BLOB_SLACK bytes behind the
 *     last string -- must be READABLE where the slack rule says so; what they hold is irrelevant to every answer;
 *   - outputs are written at the documented slots only: nothing in front of out[0], nothing behind the last slot. */
typedef struct {
    const uint8_t *blob;     /* device */
    const uint64_t *off;     /* device, n+1 entries, or NULL for the strided form */
    uint64_t stride;         /* strided form only */
    uint64_t len;            /* strided form only */
    uint64_t max_len;        /* upper bound on any string length (CSR form; 0 = let the library measure it) */
} ta_strings;

/* N x levenshtein_simd_k_with_opts(a_i, b_i, k, false, costs) -> out[i] (u32 or TA_NONE). */
int ta_levenshtein_k_batch(const ta_strings *a, const ta_strings *b, size_t n, uint32_t k,
                           const ta_edit_costs *costs, uint32_t *out_dev, void *stream);
/* The same for strings written in a small alphabet the caller names: at most four distinct byte values -- DNA, RNA -- for which
 * a two-bit code (byte >> h) & 3 exists, or up to 32 -- IUPAC nucleotide codes, amino acids, digits, one case of the letters -- with a
 * five-bit code (byte >> h) & 31 and the byte's other three bits the same in every symbol.  The match vector of a column becomes a
 * table lookup: about half (four symbols) / two thirds (twenty) of the instructions of the byte test.  The promise is verified on
 * the device: pairs that hold any other byte are answered by the general kernel inside the same call.  Batches the small-alphabet
 * kernels do not cover run ta_levenshtein_k_batch unchanged. */
int ta_levenshtein_k_batch_alphabet(const ta_strings *a, const ta_strings *b, size_t n, uint32_t k, const ta_edit_costs *costs,
                                    const uint8_t *alphabet, size_t alphabet_len, uint32_t *out_dev, void *stream);
/* N x levenshtein_exp_with_opts(a_i, b_i, false, costs): doubling k from 30 over the still-unresolved
 * subset (src/levenshtein.rs:1480-1494).  Batches of >= 1024 pairs: the whole k schedule is enqueued at once -- every list's length stays on
 * the device -- and the call returns without synchronising (capturable in a graph; a CSR side with max_len = 0 costs one synchronisation to
 * measure it).  Smaller batches synchronise the stream between rounds.  The device-driven rounds size every launch for the whole batch (a list's
 * length is only known on the device): a round whose list is short or empty still costs its launches (10-15 us each) and takes the kernel the
 * batch size suggests -- a batch where a handful of long pairs survive to the unbounded pass pays for that; TA_EXP_HOST_ROUNDS=1 (TA_TUNING) keeps
 * the host-driven loop, which sizes every round for the pairs that are left.  The first threshold is the widest the cheapest kernel's window
 * holds (k = 32 for LEVENSHTEIN_COSTS: the price of 30), then the reference's 60, 120, ...: the returned distances do not depend on the schedule. */
int ta_levenshtein_exp_batch(const ta_strings *a, const ta_strings *b, size_t n,
                             const ta_edit_costs *costs, uint32_t *out_dev, void *stream);
/* Batch form of ta_levenshtein_trace (no reference analogue: the reference's trace_on is per call, src/levenshtein.rs:714-720, :561-606):
 * out_dev[i] = distance | TA_NONE, n_edits_dev[i] = runs of pair i's script (0 for None), edits_dev[i * cap .. i * cap + n_edits_dev[i]) =
 * the script front to back -- edit for edit the reference's Vec<Edit>.  All buffers are device memory; the call enqueues kernels on
 * `stream` and returns (no synchronisation).  2 k + 1 records per pair always suffice; a longer script is cut at `cap` records and
 * n_edits_dev[i] says how many it has.  LEVENSHTEIN_COSTS / RDAMERAU_COSTS with k <= 32 (30): no per-cell records -- the distance pass leaves a
 * checkpoint of its column state every 16th column, one more kernel recomputes tile after tile backwards and walks; any
 * other costs / wider bands: 2-bit argmin codes of the DP band kernel + a walk kernel (3.4b).  EditCosts(g, g, 0, None | Some(g)) -- unit costs
 * times g -- ride the checkpoint route with k / g (the script is the unit-cost script, the distance g times the unit one).  Batches whose
 * scratch (checkpoints, run lists) would not fit are worked through in sub-batches of whole wavefronts on the same stream.
 * TA_ERR_UNSUPPORTED for bands beyond the register kernel (> 4222 diagonals). */
int ta_levenshtein_trace_batch(const ta_strings *a, const ta_strings *b, size_t n, uint32_t k, const ta_edit_costs *costs,
                               uint32_t *out_dev, ta_edit *edits_dev, uint32_t *n_edits_dev, size_t cap, void *stream);

/* ta_levenshtein_trace_batch with PACKED records: one 32-bit word per run, (edit type << 29) | count; pair i's script is the
 * min(n_edits_dev[i], cap) words that END at packed_dev[(i + 1) * cap] -- front to back, right-aligned in the pair's slot of `cap` words (a
 * script of more than `cap` runs keeps its LAST cap runs and n_edits_dev[i] says how long it is; the words in front of a script are not
 * written).  A quarter of the bytes of the 16-byte ta_edit form, which stays the ABI's default; the bindings expand the words on the host.
 * On the checkpoint route (LEVENSHTEIN_COSTS / RDAMERAU_COSTS and their multiples EditCosts(g, g, 0, None | Some(g)), k / g <= 32 (30)) the
 * walk writes every run where it belongs: no run lists in scratch, no reversal step.  Strings of 2^29 bytes and more: TA_ERR_UNSUPPORTED. */
int ta_levenshtein_trace_batch_packed(const ta_strings *a, const ta_strings *b, size_t n, uint32_t k, const ta_edit_costs *costs,
                                      uint32_t *out_dev, uint32_t *packed_dev, uint32_t *n_edits_dev, size_t cap, void *stream);

/* N x ta_levenshtein_search_simd_with_opts(needle_i, haystack_i, k, search_type, costs, anchored) on device-resident data (no reference
 * analogue: the reference searches one haystack per call, src/levenshtein.rs:1911-1966).  Pair i's result is exactly that call's -- the
 * end == 0 match (:1693-1706), the empty-needle answers (:1919-1963), the Best fold (:1812-1835), quirk Q2 -- with positions relative to
 * haystack i: counts_dev[i] = its length, matches_dev[i * cap .. i * cap + min(counts_dev[i], cap)) = its first `cap` matches in the
 * reference's order (increasing end; pad_ = 0).  cap = 0: counts only ("which reads contain the adapter").  The cut at `cap` is
 * ta_levenshtein_trace_batch's convention.  `needles` may be the strided form with stride = 0: ONE needle blob[0 .. len) shared by every
 * pair (an adapter, a primer) -- the only form that takes the scan route below; per-pair needles (CSR or strided) are fully supported.
 * Both sides follow the TA_BLOB_SLACK rule.  One haystack is ONE lane's work: the entry is meant for many short-to-medium haystacks (reads,
 * records); a long haystack belongs on ta_levenshtein_search_dev, which spreads one haystack over the whole device.
 * Routes: the exact recurrence over each whole haystack, one lane per pair, longest haystacks first; for a shared needle
 * of up to 64 bytes, unanchored, a bit-parallel unit-cost scan first finds each haystack's span of candidate ends (a superset filter
 * under any EditCosts) and the exact recurrence runs on those spans only.
 * Errors, all before any device work: TA_ERR_BAD_COSTS when EditCosts::new or check_search fails (:1965) -- decided for the whole batch,
 * even when every needle is empty (the single call does not check an empty needle's costs against check_search); TA_ERR_ARG for null
 * pointers with n > 0, a search_type other than 0 / 1, n * cap overflowing, or a needle over 65,535 bytes (the host search forms'
 * limit); TA_ERR_UNSUPPORTED for a haystack of 2^32 bytes or more.  No device: TA_ERR_HIP.
 * The call enqueues its work on `stream` and returns without synchronising.  With every length bound known (strided sides, CSR max_len
 * given on both) it is capturable, like the other batches: no host round trip between kernels, the candidate list's length is read on
 * the device; a CSR side with max_len = 0 costs one synchronisation to measure it. */
int ta_levenshtein_search_batch(const ta_strings *needles, const ta_strings *haystacks, size_t n,
                                uint32_t k, int search_type, const ta_edit_costs *costs, int anchored,
                                ta_match *matches_dev, uint32_t *counts_dev, size_t cap, void *stream);

/* N x ta_hamming_search_simd_with_opts(needle_i, haystack_i, k, search_type) on device-resident data (no reference analogue: the reference
 * searches one haystack per call, src/hamming.rs:454-475, scalar text :96-146).  Pair i's result is exactly that call's, in the layout of
 * ta_levenshtein_search_batch: counts_dev[i] = its length, matches_dev[i * cap .. i * cap + min(counts_dev[i], cap)) = its first `cap`
 * matches in increasing start (end = start + needle_len, k = the mismatch count, pad_ = 0), positions relative to haystack i.  cap = 0:
 * counts only, matches_dev may be NULL.  The reference's checks keep their order per pair: needle_len > haystack_len, then needle_len == 0,
 * give an empty result (:455-461); only then a haystack that holds a 0x00 byte gets counts_dev[i] = TA_NONE and no matches (its slots are
 * not meaningful) where the single call returns TA_ERR_NULL_BYTE -- the other pairs are unaffected and the call returns TA_OK.  A NUL byte
 * in a needle, or in a haystack shorter than its needle, is not an error.  Best is the scalar routine's rule (:105-142): the windows at
 * the smallest mismatch count <= k, no overlap fold -- ta_search_fold_best(.., overlap_fold = 0) -- and counts_dev[i] is their number
 * whatever `cap` is.  All-mode k >= needle_len reports every offset.  `needles` may be the strided form with stride = 0: ONE needle shared
 * by every pair (a barcode, a primer); per-pair needles (CSR or strided) of up to 65,535 bytes are fully supported.  Both sides follow the
 * TA_BLOB_SLACK rule.  One haystack is ONE lane's work; a long haystack belongs on ta_hamming_search_dev.
 * Routes: a SWAR window compare for every input (needle in registers up to 64 bytes, CSR batches of >= 4096 pairs longest
 * haystack first); bit-sliced mismatch counters for a shared needle of up to 32 bytes with 4 k <= needle_len.
 * Errors, all before any device work: TA_ERR_ARG for NULL needles / haystacks, with n > 0 a NULL blob, NULL counts_dev or cap > 0 with NULL
 * matches_dev, a search_type other than 0 / 1, n * cap * sizeof(ta_match) overflowing, or a needle over 65,535 bytes; TA_ERR_UNSUPPORTED
 * for a haystack of 2^32 bytes or more.  No device: TA_ERR_HIP.  n == 0: TA_OK.
 * The call enqueues its work on `stream` and returns without synchronising.  With every length bound known (strided sides, CSR max_len
 * given on both) it is capturable under the rule above (run once outside the capture first); a CSR side with max_len = 0 costs one
 * synchronisation to measure it.  ta_last_kernel_name names the route taken. */
int ta_hamming_search_batch(const ta_strings *needles, const ta_strings *haystacks, size_t n,
                            uint32_t k, int search_type,
                            ta_match *matches_dev, uint32_t *counts_dev, size_t cap, void *stream);

/* Every query against every target within k, on device-resident data (no reference analogue: the reference takes one pair per call).
 * The pair (q, t) is a hit with distance d exactly when ta_levenshtein_simd_k_with_opts(query q, target t, k, 0, costs) gives d and not
 * TA_NONE (levenshtein_simd_k_with_opts, src/levenshtein.rs:714-720).  *count_dev = the number of hits whatever `cap` is;
 * hits_dev[0 .. min(count, cap)) holds that many DISTINCT hits {query, target, k = d, pad_ = 0} in no particular order (an atomic cursor);
 * when count > cap, which hits are kept is unspecified -- each kept one is a true hit and none appears twice.  cap = 0 asks for the count
 * only, hits_dev may then be NULL.  nearest_dev, when not NULL, gets for every query q the word (uint64_t)d << 32 | t that is smallest
 * over the hits of q -- the smallest distance, at equal distance the lowest target index -- and all ones when q has no hit; it does not
 * depend on cap.  Nothing of size nq x nt is allocated or written: the caller no longer gathers the pairs for ta_levenshtein_k_batch.
 * Both sides take the strided and the CSR form and follow the TA_BLOB_SLACK rule.
 * Costs: LEVENSHTEIN_COSTS, RDAMERAU_COSTS and their multiples EditCosts(g, g, 0, None | Some(g)) (run with k / g, reported as g d, as the
 * batch entries do); any other valid EditCosts: TA_ERR_UNSUPPORTED; invalid ones: TA_ERR_BAD_COSTS.  Every QUERY is at most 64 bytes: a
 * longer bound (the strided len, the CSR max_len given or measured) is TA_ERR_UNSUPPORTED; targets may have any length below 2^32
 * (TA_ERR_UNSUPPORTED beyond).  The distance is symmetric under these costs: a caller whose short side is the other one swaps the
 * arguments (and the two index fields of the records).
 * TA_ERR_ARG: NULL queries / targets / costs / count_dev; with nq, nt > 0 a NULL blob; cap > 0 with NULL hits_dev; nq or nt of 2^32 or
 * more; cap * sizeof(ta_cross_hit) overflowing.  All of these come before any device work.  No device: TA_ERR_HIP.  nq == 0 or nt == 0:
 * TA_OK, the count zero (and every nearest word all ones).
 * The call enqueues its work on `stream` and returns without synchronising; the counter and nearest_dev are initialised by kernels.  With
 * every length bound known (strided sides, CSR max_len given on both) it is capturable under the rule above (run once outside the
 * capture first); a CSR side with max_len = 0 costs one synchronisation to measure it.  ta_last_kernel_name names the kernel
 * (DESIGN.md 3.13). */
typedef struct {
    uint32_t query;
    uint32_t target;
    uint32_t k;
    uint32_t pad_;           /* 0 */
} ta_cross_hit;
int ta_levenshtein_cross(const ta_strings *queries, size_t nq, const ta_strings *targets, size_t nt,
                         uint32_t k, const ta_edit_costs *costs,
                         ta_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                         uint64_t *nearest_dev /* nq entries, or NULL */, void *stream);

/* Every query against every target within k MISMATCHES, on device-resident data: the Hamming twin of ta_levenshtein_cross, for sets of
 * fixed-length tags -- cell barcodes against a whitelist, a UMI set against itself, sample indices against a sheet -- where substitution
 * is the only error considered (at k = 1 Levenshtein also accepts a shifted tag).  The pair (q, t) is a hit with distance d exactly when
 * the two strings have the same length and ta_hamming(query q, target t) gives d <= k (hamming, src/hamming.rs:390).  Strings of
 * different lengths are never a hit (the reference panics there, ta_hamming_batch answers TA_NONE); two empty strings are a hit with
 * d = 0.  Bytes are opaque: 0x00 is an ordinary symbol (the NUL rule belongs to hamming_search only).
 * *count_dev, hits_dev[0 .. min(count, cap)) and nearest_dev follow ta_levenshtein_cross's rules word for word: the count is exact
 * whatever `cap` is, kept records are distinct {query, target, k = d, pad_ = 0} in no particular order, cap = 0 asks for the count only
 * (hits_dev may then be NULL), nearest_dev[q] = the smallest (uint64_t)d << 32 | t over q's hits, all ones when there is none.
 * per_query_dev, when not NULL, gets the number of hits of every query, whatever `cap` is: with nearest_dev it answers the
 * demultiplexer's question "exactly one whitelist entry within k?".  flags = TA_CROSS_UPPER restricts EVERY output (count, hits, nearest,
 * per-query) to the pairs with target index > query index: a set against itself gives each unordered pair once and no (i, i); a
 * wavefront whose 64 targets all lie at or below a query does not compare that query.  Any other flag bit: TA_ERR_ARG.
 * Every QUERY is at most 64 bytes: a longer bound (the strided len, the CSR max_len given or measured) is TA_ERR_UNSUPPORTED; targets
 * may have any length below 2^32 (TA_ERR_UNSUPPORTED beyond), those longer than 64 bytes are never hits and are not read.  Both sides take
 * the strided and the CSR form at any byte alignment and follow the TA_BLOB_SLACK rule.  Nothing of size nq x nt is allocated or written.
 * TA_ERR_ARG: NULL queries / targets / count_dev; an unknown flag bit; nq or nt of 2^32 or more; with nq, nt > 0 a NULL blob; cap > 0 with
 * NULL hits_dev; cap * sizeof(ta_cross_hit) overflowing.  All of these come before any device work.  No device: TA_ERR_HIP.  nq == 0 or
 * nt == 0: TA_OK, the count zero, every nearest word all ones, every per-query count zero.
 * The call enqueues its work on `stream` and returns without synchronising; the counter, nearest_dev and per_query_dev are initialised
 * by kernels.  With every length bound known (strided sides, CSR max_len given on both) it is capturable under the rule above (run once
 * outside the capture first); a CSR side with max_len = 0 costs one synchronisation to measure it.  ta_last_kernel_name names the kernel,
 * ham_cross_kernel<NW> with NW = 4, 8 or 16 dwords per string. */
#define TA_CROSS_UPPER 1u   /* only pairs with target index > query index (a set against itself: each unordered pair once, no (i, i)) */
int ta_hamming_cross(const ta_strings *queries, size_t nq, const ta_strings *targets, size_t nt,
                     uint32_t k, uint32_t flags,
                     ta_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                     uint64_t *nearest_dev    /* nq entries, or NULL */,
                     uint32_t *per_query_dev  /* nq entries, or NULL */, void *stream);

/* ta_levenshtein_cross with queries of up to 256 bytes and ta_hamming_cross's two further outputs: short reads against each other or a
 * panel, amplicons, dictionary lines, a read or UMI set de-duplicated within a few edits.  The hit rule, *count_dev, hits_dev, cap,
 * nearest_dev and the costs accepted are ta_levenshtein_cross's word for word; per_query_dev and flags = TA_CROSS_UPPER are
 * ta_hamming_cross's word for word (per_query_dev[q] = the number of hits of q whatever `cap` is; TA_CROSS_UPPER restricts EVERY output
 * to the pairs with target index > query index; any other flag bit: TA_ERR_ARG).  Every QUERY is at most 256 bytes: a longer bound (the
 * strided len, the CSR max_len given or measured) is TA_ERR_UNSUPPORTED; targets may have any length below 2^32.  Nothing of size
 * nq x nt is allocated or written.
 * TA_ERR_ARG: NULL queries / targets / costs / count_dev; an unknown flag bit; then the costs (TA_ERR_BAD_COSTS, TA_ERR_UNSUPPORTED); then
 * nq or nt of 2^32 or more; with nq, nt > 0 a NULL blob; cap > 0 with NULL hits_dev; cap * sizeof(ta_cross_hit) overflowing; the length
 * bounds.  All of these come before any device work.  No device: TA_ERR_HIP.  nq == 0 or nt == 0: TA_OK, the count zero, every nearest
 * word all ones, every per-query count zero.
 * The call enqueues its work on `stream` and returns without synchronising; the counter, nearest_dev and per_query_dev are initialised
 * by kernels.  With every length bound known it is capturable as the two entries above are; a CSR side with max_len = 0 costs one
 * synchronisation to measure it.  With the longest query at most 64 bytes the kernel is ta_levenshtein_cross's,
 * lev_cross_kernel<NW, TRANS>; beyond, lev_cross_win_kernel<WW, TRANS>, which keeps a window of WW = 2, 3 or 4 32-row blocks of the
 * column around the diagonal (k <= 8, 24, 40 in units of the gap cost) or all 8. */
int ta_levenshtein_cross_with_opts(const ta_strings *queries, size_t nq, const ta_strings *targets, size_t nt,
                                   uint32_t k, const ta_edit_costs *costs, uint32_t flags,
                                   ta_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                   uint64_t *nearest_dev    /* nq entries, or NULL */,
                                   uint32_t *per_query_dev  /* nq entries, or NULL */, void *stream);

/* Every needle of a panel searched in every haystack of a batch within k, on device-resident data: the shape a demultiplexer or an
 * adapter trimmer asks for -- 12 adapters, 96 sample barcodes, a primer set against a batch of reads: which needle occurs where in every
 * read (no reference analogue: the reference searches one needle in one haystack per call, src/levenshtein.rs:1911-1966).  The two cross
 * entries above compare whole strings, the search-batch entries take one needle per haystack.
 * For needle p and haystack i let R(p, i) be the list ta_levenshtein_search_simd_with_opts(needle p, haystack i, k, TA_SEARCH_BEST, costs,
 * anchored) returns: the reference's Best result -- the end == 0 match (:1693-1706), the empty-needle answers (:1919-1963), the overlap
 * fold (:1812-1835), quirk Q2 -- with positions relative to haystack i.  The pair is a hit exactly when R is not empty; its record is
 * {haystack = i, needle = p, start = R[0].start, end = R[0].end, k = R[0].k, n_matches = len(R)}.  Best mode only: there is no
 * search_type argument.
 * *count_dev and hits_dev[0 .. min(count, cap)) follow ta_levenshtein_cross's rules word for word: the count is the exact number of hits
 * whatever `cap` is, the kept records are distinct true hits in no particular order (an atomic cursor), cap = 0 asks for the count only
 * and hits_dev may then be NULL.  nearest_dev[i], when not NULL, is the smallest (uint64_t)R[0].k << 32 | p over the hits of haystack
 * i -- the cheapest needle, at equal cost the lowest needle index -- and all ones when haystack i has no hit.  best_dev[i], when not NULL,
 * is that needle's R[0] as a ta_match with pad_ = 0, or {0, 0, TA_NONE, 0} when there is no hit; it may be asked for without nearest_dev
 * (the library then keeps the nearest words in its own scratch).  per_haystack_dev[i], when not NULL, is the number of needles that hit
 * haystack i: with nearest_dev it answers "best needle per read, and is it the only one within k?".  None of the three depends on cap.
 * Nothing of size nn x nh is allocated or written by the caller, and the library's own scratch is bounded: the candidate pairs of at
 * most 256 MB worth of haystacks at a time (sub-batches of whole workgroups on the same stream).
 * Both sides take the strided and the CSR form at any byte alignment and follow the TA_BLOB_SLACK rule; every layout freedom listed
 * above ta_strings applies.  Limits, TA_ERR_UNSUPPORTED: every NEEDLE is at most 32 bytes -- a longer bound (the strided len, the CSR
 * max_len given or measured) is unsupported, the exact kernel's register form goes no further; nn is at most 65,535 (the needle groups
 * are the grid's y dimension); a haystack of 2^32 bytes or more, or nh >= 2^32.
 * Errors, all before any device work, in the search-batch entries' order: TA_ERR_ARG for NULL costs / needles / haystacks / count_dev;
 * TA_ERR_BAD_COSTS when EditCosts::new or check_search fails (:1965), decided for the whole call; TA_ERR_ARG for a NULL blob with
 * nn, nh > 0, cap > 0 with NULL hits_dev, cap * sizeof(ta_search_cross_hit) overflowing; the limits above; no device: TA_ERR_HIP.
 * nn == 0 or nh == 0: TA_OK, the count zero, every nearest word all ones, every per-haystack count zero, every best {0, 0, TA_NONE, 0}.
 * The call enqueues its work on `stream` and returns without synchronising; the counter and the three per-haystack outputs are
 * initialised by kernels.  With every length bound known (strided sides, CSR max_len given on both) it is capturable under the rule
 * above (run once outside the capture first; the number of sub-batches depends on nn and nh only); a CSR side with max_len = 0 costs one
 * synchronisation to measure it.  Routes: a bit-parallel unit-cost scan of every haystack against 64 needles per wavefront (a superset
 * filter under any EditCosts), then the exact recurrence on the candidate pairs' spans; anchored: the exact recurrence on every pair's
 * prefix.  ta_last_kernel_name names the scan kernel, lev_search_cross_scan_kernel<TRANS>, or the exact kernel
 * lev_search_cross_exact_kernel<N, TRANS, PACKED> when the call is anchored. */
typedef struct {
    uint32_t haystack, needle;   /* indices */
    uint32_t start, end;         /* R[0] of the pair, relative to the haystack */
    uint32_t k;                  /* R[0].k */
    uint32_t n_matches;          /* len(R) */
} ta_search_cross_hit;
int ta_levenshtein_search_cross(const ta_strings *needles, size_t nn, const ta_strings *haystacks, size_t nh,
                                uint32_t k, const ta_edit_costs *costs, int anchored,
                                ta_search_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                uint64_t *nearest_dev      /* nh entries, or NULL */,
                                ta_match *best_dev         /* nh entries, or NULL */,
                                uint32_t *per_haystack_dev /* nh entries, or NULL */, void *stream);

/* ta_levenshtein_search_cross for panels with needles of up to 64 bytes: read-through adapters (33, 34 bytes), full-length indexed
 * adapters, primer-plus-tag constructs (the reference searches one needle in one haystack per call, src/levenshtein.rs:1911-1966; R(p, i)
 * is the same list: the end == 0 match :1693-1706, the empty-needle answers :1919-1963, the overlap fold :1812-1835).  The contract is
 * ta_levenshtein_search_cross's word for word -- records, count, cap, nearest_dev, best_dev, per_haystack_dev, both string forms, empty
 * sides, asynchrony, capture, bounded scratch -- with two differences:
 *   1. every NEEDLE is at most 64 bytes: a longer bound (the strided len, the CSR max_len given or measured) is TA_ERR_UNSUPPORTED;
 *   2. `flags` must be 0: any set bit is TA_ERR_ARG (the word is reserved), checked behind the NULL pointers and before the costs.
 * The error order is otherwise the same: NULL pointers, flags, costs, blobs / cap / overflow, the limits, TA_ERR_HIP.
 * Routes, decided once per call from the panel's longest-needle bound.  Up to 32 bytes: exactly the kernels, the sub-batch plan and the
 * ta_last_kernel_name of ta_levenshtein_search_cross.  33..64 bytes: the two-word route for the WHOLE panel -- the scan
 * on two dwords per needle against 32 needles per half wavefront, lev_search_cross_w2_scan_kernel<TRANS>, then the exact recurrence with
 * its column in device scratch (at most 256 MB of columns), lev_search_cross_w2_exact_kernel<TRANS>, which ta_last_kernel_name names when the
 * call is anchored.  The word count is not chosen per group of needles (a CSR panel's lengths are known on the device only), so short
 * needles in a long panel pay for two words and for the memory-backed column: a caller with 96 barcodes and 2 long adapters does better
 * with two calls, one per entry. */
int ta_levenshtein_search_cross_with_opts(const ta_strings *needles, size_t nn, const ta_strings *haystacks, size_t nh,
                                          uint32_t k, const ta_edit_costs *costs, int anchored, uint32_t flags,
                                          ta_search_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                          uint64_t *nearest_dev      /* nh entries, or NULL */,
                                          ta_match *best_dev         /* nh entries, or NULL */,
                                          uint32_t *per_haystack_dev /* nh entries, or NULL */, void *stream);

/* Every needle of a panel searched in every haystack of a batch within k MISMATCHES, on device-resident data: the Hamming twin of
 * ta_levenshtein_search_cross, for panels designed around a minimum Hamming distance -- sample barcodes behind staggers, inline indices,
 * primers -- where "at most k mismatches, no indels" is the rule (at k = 1 the Levenshtein entry also accepts a shifted tag, and its
 * start, end and k differ).  A tag at a KNOWN offset is ta_hamming_cross over a strided view; this entry finds it at any offset (no
 * reference analogue: the reference searches one needle in one haystack per call, src/hamming.rs:454-475, scalar text :96-146).
 * For needle p and haystack i let R(p, i) be the list ta_hamming_search_simd_with_opts(needle p, haystack i, k, TA_SEARCH_BEST) returns:
 * the windows at the smallest mismatch count <= k, in increasing start, no overlap fold (:105-142).  The pair is a hit exactly when R is
 * not empty; its record is {haystack = i, needle = p, start = R[0].start, end = R[0].start + needle_len, k = R[0].k, n_matches = len(R)}.
 * Best mode only: there is no search_type argument.  k is any uint32_t: k >= needle_len makes every window a candidate, Best then reports
 * the windows at the minimum and n_matches can be haystack_len - needle_len + 1.
 * *count_dev, hits_dev[0 .. min(count, cap)), cap = 0, nearest_dev, best_dev and per_haystack_dev follow ta_levenshtein_search_cross word
 * for word: the count is the exact number of hits whatever `cap` is, the kept records are distinct true hits in no particular order,
 * cap = 0 asks for the count only and hits_dev may then be NULL; nearest_dev[i] is the smallest (uint64_t)R[0].k << 32 | p over the hits
 * of haystack i, all ones when there is none; best_dev[i] is that needle's R[0] with pad_ = 0, or {0, 0, TA_NONE, 0}, and may be asked
 * for without nearest_dev; per_haystack_dev[i] is the number of needles that hit haystack i.  None of the three depends on cap.
 * The reference's checks keep their order per pair (:455-461): needle_len > haystack_len, then needle_len == 0, give no hit -- an empty
 * needle never hits, unlike the Levenshtein entry.  Only then the NUL rule applies: in a haystack that holds a 0x00 byte the pairs with
 * 1 <= needle_len <= haystack_len, where the single call returns TA_ERR_NULL_BYTE, produce no record and touch neither nearest nor
 * best, and per_haystack_dev[i] = TA_NONE when at least one such pair exists; the call still returns TA_OK and every other haystack is
 * unaffected (ta_hamming_search_batch's convention).  A caller who cannot rule out 0x00 bytes asks for per_haystack_dev.  A NUL in a
 * needle, in the bytes around the strings, or in a haystack shorter than every non-empty needle is not an error.
 * Both sides take the strided and the CSR form at any byte alignment and follow the TA_BLOB_SLACK rule; every layout freedom listed
 * above ta_strings applies.  Limits, TA_ERR_UNSUPPORTED: every NEEDLE is at most 32 bytes -- a longer bound (the strided len, the CSR
 * max_len given or measured) is unsupported, the counters are one dword wide; nn is at most 65,535 (the needle groups are the grid's y
 * dimension); a haystack of 2^32 bytes or more, or nh >= 2^32.
 * Errors, all before any device work, in this order: TA_ERR_ARG for NULL needles / haystacks / count_dev; TA_ERR_ARG for a NULL blob
 * with nn, nh > 0, cap > 0 with NULL hits_dev, cap * sizeof(ta_search_cross_hit) overflowing; the limits above; no device: TA_ERR_HIP.
 * nn == 0 or nh == 0: TA_OK, the count zero, every nearest word all ones, every per-haystack count zero, every best {0, 0, TA_NONE, 0}.
 * The call enqueues its work on `stream` and returns without synchronising; every output is initialised by kernels.  With every length
 * bound known (strided sides, CSR max_len given on both) it is capturable under the rule above (run once outside the capture first); a
 * CSR side with max_len = 0 costs one synchronisation to measure it.  One pass, exact: bit-sliced mismatch counters of every haystack
 * against 64 needles per wavefront -- no candidate list, no scratch of size nn x nh, no sub-batches (the library keeps one 64-bit word
 * per haystack when nearest_dev or best_dev is asked for).  ta_last_kernel_name names the scan kernel with its plane count,
 * ham_search_cross_kernel<B>, B = the smallest with 2^B - 1 >= min(k, longest needle): 1 .. 6. */
int ta_hamming_search_cross(const ta_strings *needles, size_t nn, const ta_strings *haystacks, size_t nh,
                            uint32_t k,
                            ta_search_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                            uint64_t *nearest_dev      /* nh entries, or NULL */,
                            ta_match *best_dev         /* nh entries, or NULL */,
                            uint32_t *per_haystack_dev /* nh entries, or NULL */, void *stream);

/* ta_hamming_search_cross for panels with needles of up to 64 bytes: read-through adapters (33, 34 bytes), full-length indexed adapters,
 * primer-plus-tag constructs of 40 to 64 bytes, where "at most k mismatches, no indels" is the rule (the reference searches one needle in
 * one haystack per call, src/hamming.rs:454-475, scalar text :96-146; R(p, i) is the same list: the windows at the smallest mismatch
 * count <= k, in increasing start, no overlap fold).  The contract is ta_hamming_search_cross's word for word -- R(p, i), records, count,
 * cap, cap = 0, nearest_dev, best_dev, per_haystack_dev, the per-pair order of the checks (needle_len > haystack_len, needle_len == 0,
 * then the 0x00 rule with per_haystack_dev[i] = TA_NONE), both string forms at any alignment, empty sides, asynchrony, capture, every
 * output initialised by kernels -- with two differences:
 *   1. every NEEDLE is at most 64 bytes: a longer bound (the strided len, the CSR max_len given or measured) is TA_ERR_UNSUPPORTED;
 *   2. `flags` must be 0: any set bit is TA_ERR_ARG (the word is reserved), checked behind the NULL pointers and before the blobs.
 * The error order is otherwise the same: NULL pointers, flags, blobs / cap / overflow, the limits, TA_ERR_HIP.
 * Routes, decided once per call from the panel's longest-needle bound.  Up to 32 bytes: exactly the kernel, the work split and the
 * ta_last_kernel_name of ta_hamming_search_cross (ham_search_cross_kernel<B>).  33..64 bytes: the two-word route for the WHOLE panel
 *  -- mismatch counters of 64 positions on two dwords against 32 needles per half wavefront, still one exact pass
 * without a candidate list: ham_search_cross_w2_kernel<B>, B = the smallest with 2^B - 1 >= min(k, longest needle): 1 .. 7.  The word
 * count is not chosen per group of needles (a CSR panel's lengths are known on the device only), so short barcodes in a long panel pay
 * for two words: a caller with 96 barcodes and 2 long adapters does better with two calls, one per entry. */
int ta_hamming_search_cross_with_opts(const ta_strings *needles, size_t nn, const ta_strings *haystacks, size_t nh,
                                      uint32_t k, uint32_t flags,
                                      ta_search_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                      uint64_t *nearest_dev      /* nh entries, or NULL */,
                                      ta_match *best_dev         /* nh entries, or NULL */,
                                      uint32_t *per_haystack_dev /* nh entries, or NULL */, void *stream);

/* ---- token batches: sequences of 32-bit items (new surface) ----------------------------------
 * The generic entry points of the reference take any item type T: PartialEq (levenshtein_naive<T>, levenshtein_naive_with_opts<T>,
 * levenshtein_naive_k_with_opts<T>, src/levenshtein.rs:105-148, 376).  These entries extend the batch contracts above to sequences of
 * u32 items -- token ids, word ids -- resident in device memory.  Results follow the byte entries exactly (TA_NONE above k, the EditCosts
 * checks, scripts edit for edit the scalar path's, src/levenshtein.rs:471-532, 561-606).
 * Inside, a kernel codes every pair as two byte strings with  a[i] == b[j]  <=>  ca[i] == cb[j]  (the kernels only ever compare an item of
 * a with an item of b), the byte entries run on the codes, and the rare pair whose shorter side is longer than 255 items and which holds
 * more than 254 distinct common items is answered by the DP wide kernel over 32-bit items.
 * Item i of sequence p is data[off[p] + i] (CSR, n+1 ELEMENT offsets) or data[p * stride + i] (off == NULL, `len` items each).  No read
 * slack is required.  CSR: `len` = items `data` holds (an upper bound of off[n]; 0 = the library reads off[n]: one synchronisation), and
 * max_len = 0 lets the library measure it (one synchronisation).  Scratch: the byte codes (one byte per item) and, for pairs whose
 * shorter side exceeds 255 items, a hash table per wavefront. */
typedef struct {
    const uint32_t *data;    /* device */
    const uint64_t *off;     /* device, n+1 element offsets, or NULL for the strided form */
    uint64_t stride;         /* elements, strided form only */
    uint64_t len;            /* strided: elements per sequence; CSR: elements `data` holds (0 = read off[n]) */
    uint64_t max_len;        /* elements; CSR: 0 = let the library measure it */
} ta_tokens;

/* ta_levenshtein_k_batch over token sequences (levenshtein_naive_k_with_opts<T>, src/levenshtein.rs:376; the batch contract of
 * ta_levenshtein_k_batch).  Asynchronous and capturable (with max_len and len given) like its byte twin: the overflow pass reads the
 * length of its list on the device. */
int ta_levenshtein_k_batch_tokens(const ta_tokens *a, const ta_tokens *b, size_t n, uint32_t k,
                                  const ta_edit_costs *costs, uint32_t *out_dev, void *stream);
/* ta_levenshtein_exp_batch over token sequences (levenshtein_naive_with_opts<T>, src/levenshtein.rs:105-148): overflow pairs go straight
 * to the unbounded pass (the distances do not depend on the schedule). */
int ta_levenshtein_exp_batch_tokens(const ta_tokens *a, const ta_tokens *b, size_t n,
                                    const ta_edit_costs *costs, uint32_t *out_dev, void *stream);
/* ta_levenshtein_trace_batch over token sequences (levenshtein_naive_k_with_opts<T> with trace_on, src/levenshtein.rs:376, 561-606): the
 * same buffers and `cap` cutting.  When a pair's shorter side can exceed 255 items the call reads the overflow count (ONE stream
 * synchronisation: not capturable then) and traces the overflow pairs one by one (wide kernel + host walk) into the caller's buffers. */
int ta_levenshtein_trace_batch_tokens(const ta_tokens *a, const ta_tokens *b, size_t n, uint32_t k, const ta_edit_costs *costs,
                                      uint32_t *out_dev, ta_edit *edits_dev, uint32_t *n_edits_dev, size_t cap, void *stream);
/* One pair from host memory (levenshtein_naive_k_with_opts<T>, src/levenshtein.rs:376): *out = distance or TA_NONE; edits == NULL:
 * distance only, else the run-length script (library-owned, ta_free) as ta_levenshtein_trace returns it. */
int ta_levenshtein_tokens(const uint32_t *a, size_t a_len, const uint32_t *b, size_t b_len, uint32_t k,
                          const ta_edit_costs *costs, uint32_t *out, ta_edit **edits, size_t *n_edits);

/* ta_levenshtein_cross_with_opts over token sequences: EVERY query against EVERY target within k, nothing of size nq x nt anywhere
 * (DESIGN.md 3.20).  The pair (q, t) is a hit with distance d exactly when levenshtein_naive_k_with_opts<u32>(query q, target t, k, false,
 * costs) is Some(d) (src/levenshtein.rs:376) -- ta_levenshtein_k_batch_tokens' answer for that pair.  *count_dev, hits_dev, cap (0: the
 * count only), nearest_dev, per_query_dev and flags = TA_CROSS_UPPER are ta_levenshtein_cross_with_opts' word for word, and so are the
 * costs: LEVENSHTEIN_COSTS, RDAMERAU_COSTS and their multiples (g, g, 0, None | g), run with k / g and reported as g d; other valid costs
 * are TA_ERR_UNSUPPORTED.
 * Limits: every query at most 64 tokens -- a longer bound, the strided `len` or a CSR max_len given or measured, is TA_ERR_UNSUPPORTED;
 * targets of any length below 2^32 items; nq, nt < 2^32.  Both sides take the strided and the CSR form (element offsets, which may start
 * above 0); no read slack: nothing outside a sequence's items is read.  The CSR field `len` is not needed and is ignored; max_len = 0
 * costs one synchronisation (both sides are measured together).
 * Error order, all before any device work: NULL pointers, flags, the costs, the counts / NULL data with nq, nt > 0 / cap with NULL
 * hits_dev / cap overflow, the length bounds, then TA_ERR_HIP without a device.  nq == 0 or nt == 0: TA_OK, count zero, nearest words all
 * ones, per-query counts zero.  Asynchronous on `stream`, the counters initialised by kernels: capturable when every length bound is
 * known.  Inside, a lane owns a target and a wavefront walks a tile of queries as in ta_levenshtein_cross; a query's match vectors come
 * from a hash table of 256 slots in the wavefront's LDS, keyed by the raw 32-bit values (the per-pair byte codes of the batch entries
 * cannot be shared among 64 targets).  ta_last_kernel_name: lev_cross_tok_kernel<NW, TRANS>, NW = 1 up to 32 tokens, else 2. */
int ta_levenshtein_cross_tokens(const ta_tokens *queries, size_t nq, const ta_tokens *targets, size_t nt,
                                uint32_t k, const ta_edit_costs *costs, uint32_t flags,
                                ta_cross_hit *hits_dev, unsigned long long *count_dev, size_t cap,
                                uint64_t *nearest_dev    /* nq entries, or NULL */,
                                uint32_t *per_query_dev  /* nq entries, or NULL */, void *stream);

/* N x hamming(a_i, b_i); out[i] = TA_NONE where the lengths differ (Rust: panic).  Strings below 64 KiB run one wavefront (or a part of
 * one) per pair; longer ones are cut into slices of 16 KiB, one wavefront per slice, the slices of the whole batch spread over the chip
 * (strided: len >= 64 KiB; CSR: the same on the sides' max_len, or up to 8,192 pairs without one; never CSR batches of more than 65,536
 * pairs).  The answers are the same either way and out_dev[i] is stored exactly once.  The sliced form keeps thread-local scratch:
 * capturable under the rule above. */
int ta_hamming_batch(const ta_strings *a, const ta_strings *b, size_t n, uint32_t *out_dev, void *stream);
/* hamming(a, b), src/hamming.rs:390 -> :317, of ONE pair that already lies in device memory as two pointers of `len` bytes each, at any
 * and different byte alignments: *out_dev = the number of differing positions.  No read slack is needed: nothing outside
 * [a_dev, a_dev + len) and [b_dev, b_dev + len) is read.  Asynchronous on `stream`, capturable under the rule above; from 64 KiB on
 * the pair is sliced over the chip (below, one wavefront is faster: the rule is ta_hamming_batch's for one pair).  len = 0: *out_dev = 0 (the pointers may be NULL).  A NULL out_dev, or a NULL string with
 * len > 0: TA_ERR_ARG.  len >= 0xFFFFFFFF: TA_ERR_UNSUPPORTED (the count is a u32 and 0xFFFFFFFF is TA_NONE). */
int ta_hamming_dev(const uint8_t *a_dev, const uint8_t *b_dev, size_t len, uint32_t *out_dev, void *stream);

/* ---- a queue for callers that produce pairs ONE AT A TIME (the reference's calling convention, src/levenshtein.rs:714-720) but
 * can wait for the answers: a single call costs a kernel launch (22-25 us for a 256-byte pair, against ~2 us on a host core);
 * pushed pairs are copied into pinned staging and answered together by ONE ta_levenshtein_k_batch per flush.
 *   ta_queue_create: every pair of the queue is levenshtein_simd_k_with_opts(a, b, k, false, costs).
 *   ta_queue_push:   copies the pair; *ticket = its index in the next flush's result array.
 *   ta_queue_flush:  uploads, one batch pass (CSR, length-ordered on the device), downloads; *results (library-owned, valid until
 *                    the next push / flush / destroy) holds *n answers (TA_NONE = None) in push order; the queue is empty again.
 * A queue belongs to one thread at a time.  Tickets restart at 0 after every flush. */
typedef struct ta_queue ta_queue;
int ta_queue_create(uint32_t k, const ta_edit_costs *costs, ta_queue **out);
int ta_queue_push(ta_queue *q, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, size_t *ticket);
int ta_queue_flush(ta_queue *q, const uint32_t **results, size_t *n);
void ta_queue_destroy(ta_queue *q);

/* ---- the device set: the multi-GPU split behind this boundary ----------------------------------------------------------
 * BASELINE.json north_star: "large batches of independent string pairs -- and for levenshtein_search the haystack itself -- are
 * partitioned across the 8 GPUs of one node", for callers that stay on the reference's calling convention: host slices, one process
 * (src/levenshtein.rs:714-720, 1911-1918, 2508-2511; src/hamming.rs:454-475).  The library keeps one worker thread per entry of the
 * device set (hipSetDevice, its own stream, pinned staging ring and scratch).  Pairs shard as contiguous ranges, a haystack as contiguous
 * byte ranges behind needle_len + unit_k + 2 bytes of left context (Levenshtein) / in front of needle_len - 1 bytes of overlap (Hamming);
 * there is no device-to-device traffic: results return over each device's own PCIe link and are concatenated in shard order.
 *   ta_set_devices(ids, n): the set (NULL / 0: every visible device, also the default).  An id may appear more than once -- that many
 *   workers share the device (how a one-GPU box exercises the N-way logic).  Not to be called while other calls are in flight; resident
 *   handles created before keep the workers they were created on.  A process that owns ONE GPU of a node (one rank per GPU under a launcher,
 *   all GPUs visible) should name it -- ta_set_devices(&mine, 1) -- or its big host calls fan out over its neighbours' devices too.
 * What fans out when the set has more than one entry: the *_host batch entries below, ta_queue_flush (and through it the bindings'
 * levenshtein_simd_k_with_opts_many), and the host search entries ta_levenshtein_search_simd_with_opts (unanchored) /
 * ta_hamming_search_simd_with_opts / ta_hamming_search_naive_with_opts for haystacks of >= 8 MiB (>= 4 MiB per device used).
 * Results are identical to the one-device path's, bit for bit and in the same order. */
int ta_set_devices(const int *devices, size_t n);
int ta_get_devices(int *out, size_t cap, size_t *n_out);

/* Batches whose strings live in HOST memory (ta_strings with host pointers: CSR offsets or the strided form): N x
 * levenshtein_simd_k_with_opts(a_i, b_i, k, false, costs) / levenshtein_exp_with_opts(a_i, b_i, false, costs) / hamming(a_i, b_i)
 * -> out[i] (host; TA_NONE = None / a length mismatch).  Every device of the set takes a contiguous slice of the pairs (no device gets
 * fewer than 4,096) and works through it in chunks of <= 64 MiB of strings: uploaded (big pieces by the runtime's path for pageable memory, CSR
 * offsets rebased through a pinned ring), answered by the batch entry of the same name, the answers downloaded; a device whose slice holds >= 16 MiB
 * of strings is fed by two threads and streams.  Synchronous. */
int ta_levenshtein_k_batch_host(const ta_strings *a_host, const ta_strings *b_host, size_t n, uint32_t k,
                                const ta_edit_costs *costs, uint32_t *out_host);
int ta_levenshtein_exp_batch_host(const ta_strings *a_host, const ta_strings *b_host, size_t n,
                                  const ta_edit_costs *costs, uint32_t *out_host);
int ta_hamming_batch_host(const ta_strings *a_host, const ta_strings *b_host, size_t n, uint32_t *out_host);
/* N x levenshtein_simd_k_with_opts(a_i, b_i, k, true, costs) for HOST strings over the device set: out_host[i] = distance | TA_NONE, n_edits_host[i] =
 * the runs of pair i's script (0 for None), packed_host[i * cap ..]: the script as packed runs, (edit type << 29) | count, front to back, in the LAST
 * min(n_edits_host[i], cap) words of the pair's slot (ta_levenshtein_trace_batch_packed's layout; the words in front of a script are undefined).
 * cap = 2 k + 1 holds every script of cost <= k; a longer script keeps its last cap runs. */
int ta_levenshtein_trace_batch_host(const ta_strings *a_host, const ta_strings *b_host, size_t n, uint32_t k, const ta_edit_costs *costs,
                                    uint32_t *out_host, uint32_t *packed_host, uint32_t *n_edits_host, size_t cap);

/* A pair batch uploaded ONCE and kept resident, sharded over the first n_shards devices of the set (0: as the *_host entries choose);
 * every later call runs the shards side by side and downloads 4 bytes per pair.  ta_sharded_pairs_time_levenshtein_k: `steps` passes back
 * to back with the answers left on the devices; *device_ms = the slowest shard's device time (HIP events on its worker's stream). */
typedef struct ta_sharded_pairs ta_sharded_pairs;
int ta_sharded_pairs_upload(const ta_strings *a_host, const ta_strings *b_host, size_t n, size_t n_shards, ta_sharded_pairs **out);
int ta_sharded_pairs_levenshtein_k(ta_sharded_pairs *s, uint32_t k, const ta_edit_costs *costs, uint32_t *out_host);
int ta_sharded_pairs_levenshtein_exp(ta_sharded_pairs *s, const ta_edit_costs *costs, uint32_t *out_host);
int ta_sharded_pairs_hamming(ta_sharded_pairs *s, uint32_t *out_host);
int ta_sharded_pairs_time_levenshtein_k(ta_sharded_pairs *s, uint32_t k, const ta_edit_costs *costs, int steps, float *device_ms);
int ta_sharded_pairs_shards(const ta_sharded_pairs *s, size_t *n_shards, size_t *n_pairs);
void ta_sharded_pairs_free(ta_sharded_pairs *s);

/* A haystack uploaded ONCE and kept resident as contiguous shards (BASELINE config 5: one shard per GPU), each with `overlap` bytes of its
 * neighbours on either side: every search with needle_len + unit_k + 2 <= overlap (Levenshtein) / needle_len - 1 <= overlap (Hamming) runs
 * on the resident bytes -- TA_ERR_ARG beyond.  The results are those of ta_levenshtein_search_simd_with_opts (unanchored) /
 * ta_hamming_search_simd_with_opts over the whole haystack: library-allocated (ta_free). */
typedef struct ta_sharded_haystack ta_sharded_haystack;
int ta_sharded_haystack_upload(const uint8_t *haystack, size_t len, size_t overlap, size_t n_shards, ta_sharded_haystack **out);
int ta_sharded_haystack_levenshtein_search(ta_sharded_haystack *h, const uint8_t *needle, size_t needle_len, uint32_t k, int search_type,
                                           const ta_edit_costs *costs, ta_match **out, size_t *n_out);
int ta_sharded_haystack_hamming_search(ta_sharded_haystack *h, const uint8_t *needle, size_t needle_len, uint32_t k, int search_type,
                                       ta_match **out, size_t *n_out);
int ta_sharded_haystack_shards(const ta_sharded_haystack *h, size_t *n_shards, size_t *len);
void ta_sharded_haystack_free(ta_sharded_haystack *h);

/* All-mode hits of one haystack shard resident in HBM (levenshtein_search_simd_with_opts with
 * SearchType::All; the order-dependent Best fold is a sequential host pass, ta_search_fold_best).
 * `base` is added to start/end (global offset of this shard inside a larger haystack);
 * `emit_from` suppresses hits whose end <= emit_from (left-halo positions).
 * hits_dev receives up to `cap` records in NO particular order (atomic cursor): sort them by `end` -- unique per
 * hit -- before ta_search_fold_best; *count_host receives the total found
 * (may exceed cap => TA_ERR_CAPACITY after sync).  Synchronises the stream. */
int ta_levenshtein_search_dev(const uint8_t *needle_host, size_t needle_len,
                              const uint8_t *haystack_dev, size_t haystack_len,
                              uint32_t k, const ta_edit_costs *costs, int anchored,
                              uint64_t base, uint64_t emit_from,
                              ta_match *hits_dev, size_t cap, uint64_t *count_host, void *stream);
int ta_hamming_search_dev(const uint8_t *needle_host, size_t needle_len,
                          const uint8_t *haystack_dev, size_t haystack_len, uint32_t k,
                          uint64_t base, ta_match *hits_dev, size_t cap, uint64_t *count_host, void *stream);
/* ta_hamming_search_dev with the hits on the host, sorted by end, library-allocated (ta_free): the hits of an ordinary search (up to 680)
 * arrive through host-mapped pinned memory with the call's one stream synchronisation; more are copied from hits_dev (which must hold
 * `cap` records either way).  Synchronises the stream.  (src/hamming.rs:454-554: the All-mode result of hamming_search_simd_with_opts.) */
int ta_hamming_search_dev_sorted(const uint8_t *needle_host, size_t needle_len,
                                 const uint8_t *haystack_dev, size_t haystack_len, uint32_t k,
                                 uint64_t base, ta_match *hits_dev, size_t cap, ta_match **out, size_t *n_out, void *stream);

/* The Best-mode pass over one shard in a single call (what `levenshtein_search` with SearchType::Best needs from a shard,
 * src/levenshtein.rs:1792-1835): ta_levenshtein_search_dev (unanchored) + ta_search_best_hits_dev fused.  The All-mode hits stay
 * in hits_dev (*count_host of them); *out receives only the hits with the smallest k -- the only ones ta_search_fold_best can
 * keep -- library-allocated (ta_free), sorted by end.  For unit-cost families and needles of up to 64 bytes the whole pass is
 * one fill, two kernels and one stream synchronisation (the number of flagged blocks, the minimum and the selection never leave
 * the device; the result arrives in host-mapped memory).  Synchronises the stream. */
int ta_levenshtein_search_best_dev(const uint8_t *needle_host, size_t needle_len,
                                   const uint8_t *haystack_dev, size_t haystack_len,
                                   uint32_t k, const ta_edit_costs *costs, uint64_t base, uint64_t emit_from,
                                   ta_match *hits_dev, size_t cap, uint64_t *count_host,
                                   ta_match **out, size_t *n_out, void *stream);

/* Best-mode shortcut for a shard whose All-mode hits sit in HBM (the hits_dev / count of ta_*_search_dev): only the hits
 * with the smallest k can survive ta_search_fold_best, so the minimum and the selection run on the device and only those
 * records come back -- library-allocated (ta_free), sorted by end, ready for ta_search_fold_best.  Synchronises. */
int ta_search_best_hits_dev(const ta_match *hits_dev, uint64_t count, ta_match **out, size_t *n_out, void *stream);

/* Sequential Best post-pass over All-mode hits in increasing `end` order (host memory):
 * running curr_k, overlap fold, final filter (src/levenshtein.rs:1792-1796, 1812-1835;
 * hamming: src/hamming.rs:122-143 with fold = 0).  In place; returns the new count. */
size_t ta_search_fold_best(ta_match *hits, size_t n, uint32_t k, int overlap_fold);

#ifdef __cplusplus
}
#endif
#endif
