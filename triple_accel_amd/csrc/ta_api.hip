// ta_api.hip -- the C ABI (include/triple_accel_amd.h) of the distance path: the thread's context, the distance pass (lev_pass), the k /
// alphabet / exp batch entries, the queue, the single calls and their staging (the traceback entries: ta_trace.hip).  No CPU fallback.
// The host rules the other C-ABI files share are defined here once (declared in ta_internal.h: measure_max_lens, order_pairs,
// check_batch_args; the scratch slots are named by its ScratchSlot); the pure ones -- cost checks, unit-cost tests, the length-order
// threshold, the cross entries' query tile -- are in lev_plan.h.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <mutex>
#include <vector>

#include "ta_internal.h"

namespace ta {

static thread_local std::string g_last_error;
static thread_local ta_launch_info g_last_launch = {};
ta_launch_info &last_launch() { return g_last_launch; }
// true when the last distance pass of this thread was ONE kernel whose only store to its result slot is the answer: the
// single-call entry points may then watch the pinned result word instead of synchronising the stream (fetch_u32)
static thread_local bool g_answer_single_store = false;
static thread_local int g_exp_passes = 0;          // distance passes the last ta_levenshtein_exp_batch of this thread launched

void set_last_error(const char *what, hipError_t e) {
    g_last_error = std::string(what) + ": " + hipGetErrorString(e);
}
void set_last_error_msg(const char *msg) { g_last_error = msg; }
static thread_local char g_last_kernel_name[96] = "";
void set_last_kernel_name(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_kernel_name, sizeof(g_last_kernel_name), fmt, ap);
    va_end(ap);
}

bool device_ready() {
    static int state = -1;   // -1 unknown, 0 no, 1 yes
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    if (state < 0) {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        state = (e == hipSuccess && n > 0) ? 1 : 0;
        if (!state) set_last_error_msg("no HIP device available (triple_accel_amd has no CPU fallback)");
    }
    if (!state) set_last_error_msg("no HIP device available (triple_accel_amd has no CPU fallback)");
    return state == 1;
}

// set by every Scratch::ensure, consumed by the StreamGuard of the call: did this call put thread-local scratch to use?
static thread_local bool g_scratch_in_use = false;

// true while the call's stream is being captured into a graph (StreamGuard): thread-local scratch must not grow then -- hipFree / hipMalloc are
// illegal inside a capture, and the graph bakes the scratch pointers in
static thread_local bool g_call_capturing = false;

int Scratch::ensure(size_t bytes) {
    g_scratch_in_use = true;
    if (bytes <= cap) return TA_OK;
    if (g_call_capturing) {
        set_last_error_msg("stream capture: the call needs more thread-local scratch than this thread holds -- run the same call once outside the capture first "
                           "(the graph stays valid until a later call of the thread grows the scratch, or ta_thread_release)");
        return TA_ERR_UNSUPPORTED;
    }
    if (dev) { (void)hipFree(dev); dev = nullptr; cap = 0; }
    size_t want = bytes < 4096 ? 4096 : bytes + bytes / 4;
    TA_HIP(hipMalloc(&dev, want));
    cap = want;
    return TA_OK;
}
void Scratch::release() {
    if (dev) (void)hipFree(dev);
    dev = nullptr; cap = 0;
}
Scratch::~Scratch() { /* at thread exit the HIP runtime may already be gone (process teardown): ta_thread_release() is the explicit way */ }
Scratch &tls_scratch(ScratchSlot which) {
    static thread_local Scratch s[TA_SCRATCH_SLOTS];
    return s[which];
}

int CallCtx::ensure() {
    if (st && pin) return TA_OK;
    if (!st) TA_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    if (!pin) {
        void *h = nullptr, *d = nullptr;
        TA_HIP(hipHostMalloc(&h, PIN_BYTES, hipHostMallocMapped));
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) d = h;
        pin = (uint8_t *)h; pin_dev = (uint8_t *)d;
    }
    return TA_OK;
}
void CallCtx::release() {
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); st = nullptr; }
    if (pin) { (void)hipHostFree(pin); pin = nullptr; pin_dev = nullptr; }
}
CallCtx &call_ctx() {
    static thread_local CallCtx c;
    return c;
}

int PinBox::ensure() {
    if (host) return TA_OK;
    void *h = nullptr, *d = nullptr;
    TA_HIP(hipHostMalloc(&h, SEARCH_REPORT_BYTES, hipHostMallocMapped));
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) d = h;
    host = (uint8_t *)h; dev = (uint8_t *)d;
    return TA_OK;
}
void PinBox::release() {
    if (host) (void)hipHostFree(host);
    host = dev = nullptr;
}
PinBox &search_report_box() {
    static thread_local PinBox b;
    return b;
}

struct LastUse { hipStream_t st = nullptr; hipEvent_t ev = nullptr; bool pending = false; };
static LastUse &last_use() {
    static thread_local LastUse u;
    return u;
}
// A call that put thread-local scratch to use records an event at its end (its kernels may still be reading that scratch when
// it returns); a later call of the thread on ANOTHER stream waits for that event first.  Calls that touch no scratch -- the
// fixed-length batch passes, ta_hamming_batch: the hot paths -- record nothing (an event record per call was a fifth of a small
// batch call's cost).  The event is recorded while the stream is certainly alive: the caller may destroy it afterwards.
// A stream that is being CAPTURED into a graph neither waits for the event nor records it: an event recorded inside a capture belongs to
// the capture (a later wait on it from an ordinary stream is not a wait for the replayed graph's kernels -- it put the kernels of the
// following calls out of order on gfx950: a memory fault in bench.py --unit-prefilter under its hipGraph), and the graph's own edges
// order the captured calls.  Whoever replays a captured call next to ordinary calls of the same thread on ANOTHER stream orders them
// himself (one stream, or an event of his own): the thread-local scratch is shared.
bool stream_is_capturing(hipStream_t s) {
    if (!s) return false;                                 // (the null stream cannot be captured)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}
StreamGuard::StreamGuard(hipStream_t s) : st(s) {
    LastUse &u = last_use();
    was_capturing = g_call_capturing;
    capturing = stream_is_capturing(s);
    g_call_capturing = capturing;
    if (u.pending && u.st != s && u.ev && !capturing) (void)hipStreamWaitEvent(s, u.ev, 0);
}
StreamGuard::~StreamGuard() {
    g_call_capturing = was_capturing;
    if (!g_scratch_in_use) return;
    g_scratch_in_use = false;
    if (capturing) return;
    LastUse &u = last_use();
    if (!u.ev && hipEventCreateWithFlags(&u.ev, hipEventDisableTiming) != hipSuccess) { u.ev = nullptr; return; }
    if (hipEventRecord(u.ev, st) == hipSuccess) { u.st = st; u.pending = true; }
}

// Test / tuning switches.  They are honoured only when TA_TUNING was set in the environment when the
// library was loaded: a production process reads the environment exactly once (here) and never on the call path.
static const bool g_tuning = getenv("TA_TUNING") != nullptr;
bool tuning_enabled() { return g_tuning; }
const char *env_str(const char *name) { return g_tuning ? getenv(name) : nullptr; }
int env_int(const char *name) {
    const char *v = env_str(name);
    return v ? atoi(v) : 0;
}

static thread_local bool g_opt_early_out = false;
bool early_out_enabled() { return g_opt_early_out || env_int("TA_EARLY_OUT"); }
static thread_local bool g_opt_unit_prefilter = false;
bool unit_prefilter_enabled() { return g_opt_unit_prefilter || env_int("TA_UNIT_PREFILTER"); }

// longest string of a batch side: given, implied (strided) or measured on the device
static int side_max_len(const ta_strings *s, uint32_t n, hipStream_t st, uint64_t *out) {
    if (!s->off) { *out = s->len; return TA_OK; }
    if (s->max_len) { *out = s->max_len; return TA_OK; }
    Scratch &sc = tls_scratch(SLOT_COUNT);
    int rc = sc.ensure(16);
    if (rc) return rc;
    TA_HIP(hipMemsetAsync(sc.dev, 0, 4, st));
    TA_HIP(strings_maxlen_launch(view_of(s), n, (uint32_t *)sc.dev, st));
    uint32_t v = 0;
    TA_HIP(hipMemcpyAsync(&v, sc.dev, 4, hipMemcpyDeviceToHost, st));
    TA_HIP(hipStreamSynchronize(st));
    *out = v;
    return TA_OK;
}

// The switches of the distance path (lev_route.h: LevSwitches), one name per line; nothing else on that path reads these names.
LevSwitches lev_switches() {
    LevSwitches sw = {};
    if (!g_tuning) return sw;
    sw.no_bits = env_int("TA_NO_BITS") != 0;
    sw.no_unit_scale = env_int("TA_NO_UNIT_SCALE") != 0;
    sw.force_d = env_int("TA_FORCE_D");
    sw.force_l = env_int("TA_FORCE_L");
    sw.force_ch = env_int("TA_FORCE_CH");
    sw.force_na = env_int("TA_FORCE_NA");
    sw.bits_static = env_int("TA_BITS_STATIC");
    sw.force_affine = env_int("TA_FORCE_AFFINE") != 0;
    sw.force_trans_select = env_int("TA_FORCE_TRANS_SELECT") != 0;
    sw.force_wide = env_int("TA_FORCE_WIDE") != 0;
    sw.force_widebits = env_int("TA_FORCE_WIDEBITS");
    sw.wb_no_tiles = env_int("TA_WB_NO_TILES") != 0;
    sw.no_latency_rule = env_int("TA_NO_LATENCY_RULE") != 0;
    sw.force_sliced = env_int("TA_FORCE_SLICED") != 0;
    sw.no_one = env_int("TA_NO_ONE") != 0;
    sw.no_bits2 = env_int("TA_NO_BITS2") != 0;
    return sw;
}

// One k-bounded distance pass over the batch (or over `subset`); the heart of every distance entry point.  Which kernel it takes, with
// what geometry, is lev_pass_route's answer (lev_route.h) to the facts gathered here; this function launches what the route names.
// columns_ordered: `subset` lists the pairs by their exact column count (length_order_launch): 64 consecutive ones share it -- what
// the VLINE form of the bit-parallel band kernel wants (one pass per wavefront)
// n_dev (optional): the length of `subset` as a kernel before this pass left it on the device -- n_work is then its upper bound (grids,
// kernel choice) and the kernels read the real count themselves (the rounds of ta_levenshtein_exp_batch: no host round trip between them)
int lev_pass(const ta_strings *a, const ta_strings *b, uint32_t n_work, const uint32_t *subset, uint32_t k,
             const ta_edit_costs *c, uint64_t max_len, uint32_t *out_dev, hipStream_t st, bool columns_ordered /* = false */,
             const uint32_t *n_dev /* = nullptr */) {
    if (env_int("TA_FAIL_PASS")) { set_last_error_msg("TA_FAIL_PASS: a distance pass that fails (tests)"); return TA_ERR_UNSUPPORTED; }
    const LevSwitches sw = lev_switches();
    const bool trans = c->has_transpose != 0;
    LevParams P;
    P.a = view_of(a); P.b = view_of(b);
    LevPassFacts F = {};
    F.n_work = n_work; F.subset = subset != nullptr; F.n_dev = n_dev != nullptr; F.columns_ordered = columns_ordered;
    F.a_csr = a->off != nullptr; F.b_csr = b->off != nullptr; F.a_len = a->len; F.b_len = b->len;
    F.max_len = max_len; F.k = k; F.c = costs_of(c);
#ifdef TA_EXPERIMENTAL
    if (const uint32_t g = costs_scale(c); sw.force_sliced && g) {      // (the band of the unit-cost pass: k / g)
        uint32_t strips = 0;
        if (lev_sliced_applies(P.a, P.b, lev_batch_unit_k(k / g, 1, 1, 0, max_len), &strips)) F.sliced_strips = strips;
    }
#endif
    const LevPassRoute R = lev_pass_route(F, sw);
    // unit costs times g: the unit-cost kernels with k / g, then the answers times g (lev_plan.h: lev_unit_scale)
    const ta_edit_costs uc = unit_costs(trans);
    if (R.scale) { c = &uc; k /= R.scale; }
    P.subset = subset; P.trace = nullptr; P.out = out_dev; P.n = n_work; P.k = k;
    P.mc = c->mismatch_cost; P.gc = c->gap_cost; P.sg = c->start_gap_cost; P.tc = trans ? c->transpose_cost : 0;
    P.u = R.u; P.o = R.o; P.L = R.L; P.PW = R.PW; P.lds_per_wave = R.lds_per_wave; P.Tw = R.Tw; P.ch = R.ch;
    P.tune = R.tune; P.n_dev = n_dev;
    ta_launch_info li = {};
    li.kernel = R.info.kernel; li.diags_per_lane = R.info.diags_per_lane; li.lanes_per_pair = R.info.lanes_per_pair;
    li.pairs_per_wave = R.info.pairs_per_wave; li.band_offset = R.info.band_offset; li.cell_bits = R.info.cell_bits;
    li.affine = R.info.affine; li.transpose = R.info.transpose;
    switch (R.kind) {
    case LEV_PASS_SLICED:
#ifdef TA_EXPERIMENTAL
        TA_HIP(lev_sliced_launch(P.a, P.b, n_work, k, R.bp.u, out_dev, st, &li.grid, &li.lds_bytes, &li.pairs_per_wave));
        break;
#else
        return TA_ERR_UNSUPPORTED;                     // (the route names it in TA_EXPERIMENTAL builds only)
#endif
    case LEV_PASS_ONE:
        TA_HIP(lev_one_launch(P, trans, max_len, st, &li.lds_bytes));
        li.grid = 1;
        break;
    case LEV_PASS_BITS2:
        TA_HIP(lev_bits2_launch(P, R.b2, trans, st, &li.grid, &li.lds_bytes));
        break;
    case LEV_PASS_BITS:
        TA_HIP(lev_bits_launch(P, R.bp, trans, max_len, st, &li.grid, &li.lds_bytes));
        break;
    case LEV_PASS_HUGE:                                // pair after pair; li.grid: the launches of a pair
        for (uint32_t p = 0; p < n_work; p++)
            TA_HIP(lev_widebits_huge_launch(a->blob + (uint64_t)p * a->stride, (uint32_t)a->len, b->blob + (uint64_t)p * b->stride,
                                            (uint32_t)b->len, R.bp.u, k, R.rows_per_lane, trans, out_dev + p, st, &li.grid));
        break;
    case LEV_PASS_ROWS:
        TA_HIP(lev_widebits_launch(P, R.rows_per_lane, max_len, trans, st, &li.grid, &li.lds_bytes));
        break;
    case LEV_PASS_BAND:
        TA_HIP(lev_band_launch(P, R.pl, R.affine, R.tmode, st, &li.grid, &li.lds_bytes));
        break;
    case LEV_PASS_WIDE:
        TA_HIP(lev_wide_launch(P, trans, st, &li.grid, &li.lds_bytes, &li.lanes_per_pair, &li.diags_per_lane));
        break;
    }
    if (R.scale) TA_HIP(scale_results_launch(out_dev, subset, n_work, n_dev, R.scale, st));
    g_last_launch = li;
    g_answer_single_store = R.single_store;
    if (!env_int("TA_DEBUG")) return TA_OK;
    if (R.kind == LEV_PASS_SLICED)
        fprintf(stderr, "[triple_accel_amd] lev pass: n=%u k=%u u=%u kernel=5 (pair-sliced) grid=%u lds=%u\n", n_work, k, R.bp.u, li.grid, li.lds_bytes);
    else if (R.kind == LEV_PASS_ONE)
        fprintf(stderr, "[triple_accel_amd] lev pass: n=1 k=%u u=%u kernel=6 (single pair, scalar-unit recurrence) lds=%u\n", k, R.u, li.lds_bytes);
    else
        fprintf(stderr, "[triple_accel_amd] lev pass: n=%u k=%u u=%u kernel=%u D=%u L=%u pairs/wave=%u width=%u-bit grid=%u lds=%u\n",
                n_work, k, R.pl.u, li.kernel, li.diags_per_lane, li.lanes_per_pair, li.pairs_per_wave, li.cell_bits, li.grid,
                li.lds_bytes);
    return TA_OK;
}

// (ta_internal.h) every fill of a capturable call is a kernel, never a memset node: DESIGN.md 3.2f
int order_pairs(const ta_strings *a, const ta_strings *b, uint32_t n, uint32_t u, uint64_t max_len, bool by_steps, bool exact,
                ScratchSlot order_slot, ScratchSlot bins_slot, hipStream_t st, const uint32_t **order_out, bool *exact_columns) {
    Scratch &ord = tls_scratch(order_slot), &bins = tls_scratch(bins_slot);
    constexpr size_t BINS_BYTES = 2 * 1024 * 32 * 4;                    // histogram + cursors: 1024 bins x 32 counters each
    const bool fresh = bins.cap < BINS_BYTES || !bins.bins_clean;
    int rc;
    if ((rc = ord.ensure((size_t)n * 4)) || (rc = bins.ensure(BINS_BYTES))) return rc;
    if (fresh) TA_HIP(fill_u32_launch((uint32_t *)bins.dev, 0u, (uint32_t)(BINS_BYTES / 8), st));
    bins.bins_clean = false;
    TA_HIP(length_order_launch(view_of(a), view_of(b), nullptr, n, u, max_len, by_steps, (uint32_t *)bins.dev, (uint32_t *)ord.dev, st, exact, exact_columns));
    bins.bins_clean = true;
    *order_out = (const uint32_t *)ord.dev;
    return TA_OK;
}

int measure_max_lens(const ta_strings *a, uint32_t na, const ta_strings *b, uint32_t nb, unsigned long long *dst, hipStream_t st,
                     uint64_t *ma, uint64_t *mb) {
    *ma = side_bound(a);
    *mb = side_bound(b);
    const bool need_a = !side_bound_known(a), need_b = !side_bound_known(b);
    if (!need_a && !need_b) return TA_OK;
    TA_HIP(fill_u32_launch((uint32_t *)dst, 0u, 4, st));
    const StrView none = {nullptr, nullptr, 0, 0};
    if (need_a && need_b && na == nb) TA_HIP(search_batch_maxlen_launch(view_of(a), view_of(b), na, dst, st));   // pair batches: one launch
    else {
        if (need_a) TA_HIP(search_batch_maxlen_launch(view_of(a), none, na, dst, st));
        if (need_b) TA_HIP(search_batch_maxlen_launch(none, view_of(b), nb, dst, st));
    }
    unsigned long long host[2] = {0, 0};
    TA_HIP(hipMemcpyAsync(host, dst, 16, hipMemcpyDeviceToHost, st));
    TA_HIP(hipStreamSynchronize(st));
    if (need_a) *ma = host[0];
    if (need_b) *mb = host[1];
    return TA_OK;
}

int batch_max_len(const ta_strings *a, const ta_strings *b, uint32_t n, hipStream_t st, uint64_t *out) {
    uint64_t ma = 0, mb = 0;
    int rc = side_max_len(a, n, st, &ma);
    if (rc) return rc;
    rc = side_max_len(b, n, st, &mb);
    if (rc) return rc;
    *out = ma > mb ? ma : mb;
    return TA_OK;
}

int check_batch_args(const void *a, const void *b, const void *a_data, const void *b_data, size_t n, const void *out, const char *what) {
    if (!a || !b || (!out && n) || n > 0xFFFFFFF0ull) { set_last_error_msg("bad batch arguments"); return TA_ERR_ARG; }
    if (n && (!a_data || !b_data)) { set_last_error_msg(what); return TA_ERR_ARG; }
    return TA_OK;
}

}  // namespace ta

using namespace ta;

extern "C" {

#ifdef TA_EXPERIMENTAL
const char *ta_version(void) { return "triple_accel_amd 0.3 (gfx950) +experimental"; }
#else
const char *ta_version(void) { return "triple_accel_amd 0.3 (gfx950)"; }
#endif

const char *ta_status_str(int s) {
    switch (s) {
        case TA_OK: return "ok";
        case TA_ERR_LEN_MISMATCH: return "length mismatch (reference: assert!(a.len() == b.len()))";
        case TA_ERR_NULL_BYTE: return "No zero/null bytes allowed in the string!";
        case TA_ERR_BAD_COSTS: return "invalid EditCosts";
        case TA_ERR_HIP: return "HIP error / no device";
        case TA_ERR_ARG: return "bad argument";
        case TA_ERR_UNSUPPORTED: return "unsupported on the GPU path";
        case TA_ERR_CAPACITY: return "output capacity exceeded";
        case TA_ERR_DIV_ZERO: return "attempt to divide by zero";
        default: return "unknown";
    }
}

int ta_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *ta_last_error(void) { return g_last_error.c_str(); }
const char *ta_last_kernel_name(void) { return g_last_kernel_name; }
int ta_set_option(int option, int value) {
    if (option == TA_OPT_EARLY_OUT) { g_opt_early_out = value != 0; return TA_OK; }
    if (option == TA_OPT_UNIT_PREFILTER) { g_opt_unit_prefilter = value != 0; return TA_OK; }
    set_last_error_msg("unknown option");
    return TA_ERR_ARG;
}

ta_edit_costs ta_levenshtein_costs(void) { ta_edit_costs c = {1, 1, 0, 0, 0}; return c; }
ta_edit_costs ta_rdamerau_costs(void) { ta_edit_costs c = {1, 1, 0, 1, 1}; return c; }

int ta_edit_costs_new(uint8_t mismatch, uint8_t gap, uint8_t start_gap, int has_transpose, uint8_t transpose,
                      ta_edit_costs *out) {
    ta_edit_costs c = {mismatch, gap, start_gap, (uint8_t)(has_transpose ? 1 : 0), (uint8_t)(has_transpose ? transpose : 0)};
    if (!costs_ok(&c)) return TA_ERR_BAD_COSTS;
    if (out) *out = c;
    return TA_OK;
}

int ta_edit_costs_check_search(const ta_edit_costs *c) {   // src/levenshtein.rs:67-71
    if (!c) return TA_ERR_ARG;
    if (c->has_transpose && !((uint32_t)c->transpose_cost <= (uint32_t)c->start_gap_cost + (uint32_t)c->gap_cost))
        return TA_ERR_BAD_COSTS;
    return TA_OK;
}

// src/levenshtein.rs:731-791
int ta_levenshtein_select(size_t a_len, size_t b_len, uint32_t k, const ta_edit_costs *c, ta_lev_select *out) {
    if (!c || !out) return TA_ERR_ARG;
    if (!costs_ok(c)) return TA_ERR_BAD_COSTS;
    const LevSelect s = lev_select(a_len, b_len, k, c->mismatch_cost, c->gap_cost, c->start_gap_cost);     // lev_route.h
    out->max_k = s.max_k; out->unit_k = s.unit_k; out->cell_bits = s.cell_bits; out->ref_lanes = s.ref_lanes;
    return TA_OK;
}

int ta_last_launch_info(ta_launch_info *out) {
    if (!out) return TA_ERR_ARG;
    *out = g_last_launch;
    return TA_OK;
}

void ta_free(void *p) { free(p); }

/* Frees what the calling thread holds inside the library: its device scratch, its stream and its pinned staging buffer.
 * Optional -- a thread that exits without it leaves them to process exit (nothing is freed from a thread-exit hook: the HIP
 * runtime may already be gone by then). */
void ta_thread_release(void) {
    (void)hipDeviceSynchronize();
    for (int i = 0; i < TA_SCRATCH_SLOTS; i++) tls_scratch((ScratchSlot)i).release();
    call_ctx().release();
    search_report_box().release();
    search_resident_reset();
    LastUse &u = last_use();                     // the event that orders this thread's calls across streams
    if (u.ev) (void)hipEventDestroy(u.ev);
    u = LastUse{};
}

/* ---------------------------------------------------------------- batch API */

int ta_levenshtein_k_batch(const ta_strings *a, const ta_strings *b, size_t n, uint32_t k,
                           const ta_edit_costs *costs, uint32_t *out_dev, void *stream) {
    int rc = check_batch_args(a, b, n, out_dev);
    if (rc) return rc;
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (!device_ready()) return TA_ERR_HIP;
    if (n == 0) return TA_OK;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    uint64_t max_len = 0;
    rc = batch_max_len(a, b, (uint32_t)n, st, &max_len);
    if (rc) return rc;
    // Ragged (CSR) batches: the band kernels run a wavefront to the longest of its 64 / L pairs, so the pairs are taken in the
    // order of a counting sort on their length class (util_kernels.hip: three small launches, ~20 us per million pairs) --
    // every wavefront then sees pairs within 8 bytes of each other.  TA_NO_LENGTH_ORDER=1 keeps the batch order.
    const uint32_t *order = nullptr;
    bool exact_columns = false;
    const LevSwitches sw = lev_switches();
    if (lev_wants_length_order(a->off || b->off, n, max_len) && !env_int("TA_NO_LENGTH_ORDER")) {
        const uint32_t u = lev_batch_unit_k(k, costs->mismatch_cost, costs->gap_cost, costs->start_gap_cost, max_len);
        // the key counts what the kernel of this pass iterates over: columns (bit-parallel kernels) or anti-diagonal steps (DP band kernel).
        // (the kernels whose time follows max(len_a, len_b) or len_a -- two pairs per lane, the single-pair kernel, the row-blocked
        // one -- never see a length-ordered CSR wavefront of many pairs: the first takes fixed-length batches only, the other two run ONE pair
        // per wavefront, where the order only shapes the launch's tail; len_b is the right key for everything that is ordered by columns.)
        const bool by_steps = !costs_scale(costs) || sw.unit_off();
        if ((rc = order_pairs(a, b, (uint32_t)n, u, max_len, by_steps, env_int("TA_BITS_VLINE") != 0, SLOT_ORDER, SLOT_ORDER_BINS, st, &order, &exact_columns))) return rc;
    }
    // TA_OPT_UNIT_PREFILTER (an option, off by default: the work then depends on the data): a weighted batch first runs the UNIT-cost
    // bit-parallel band pass with k' = lev_unit_filter_k -- "unit distance > k'" implies "weighted distance > k", i.e. None
    // (src/levenshtein.rs:539-541) -- and the DP band kernel prices only the pairs that pass answered (a list whose length stays on the
    // device).  Dissimilar batches cost the unit pass alone; a batch of near pairs pays for both.
    if (unit_prefilter_enabled() && n >= 1024 && !sw.unit_off()) {
        const bool trans = costs->has_transpose != 0;
        const uint32_t kf = lev_unit_filter_k(k, costs->mismatch_cost, costs->gap_cost, costs->start_gap_cost, trans, costs->transpose_cost);
        if (!costs_scale(costs) && kf != 0xFFFFFFFFu && lev_choose(kf, 1, 1, 0, trans, trans ? 1u : 0u, max_len, false, (uint32_t)n).kernel == LEV_K_BITS) {
            const ta_edit_costs uc = unit_costs(trans);
            Scratch &lst = tls_scratch(SLOT_SUBSET_A), &cnt = tls_scratch(SLOT_COUNT);
            if ((rc = lst.ensure(n * 4)) || (rc = cnt.ensure(16))) return rc;
            if ((rc = lev_pass(a, b, (uint32_t)n, order, kf, &uc, max_len, out_dev, st, false))) return rc;
            TA_HIP(fill_u32_launch((uint32_t *)cnt.dev, 0u, 1, st));
            TA_HIP(compact_some_launch(out_dev, order, (uint32_t)n, (uint32_t *)lst.dev, (uint32_t *)cnt.dev, st));
            rc = lev_pass(a, b, (uint32_t)n, (const uint32_t *)lst.dev, k, costs, max_len, out_dev, st, false, (const uint32_t *)cnt.dev);
            g_answer_single_store = false;
            return rc;
        }
    }
    return lev_pass(a, b, (uint32_t)n, order, k, costs, max_len, out_dev, st, exact_columns);
}

/* ta_levenshtein_k_batch for strings written in a SMALL ALPHABET the caller names (up to four byte values -- DNA, RNA: lev_bitsq_body.h;
 * up to 32 -- IUPAC codes, amino acids: lev_bitsqw_body.h): the column's match vector is then a table lookup instead of a byte test --
 * the same answers, bit for bit.
 * The promise is verified on the device, byte by byte: a pair that holds any other byte is answered by the general kernel in the
 * same call (a second, usually empty, launch over the list of such pairs; no host round trip).  Batches the small-alphabet kernel
 * does not cover (CSR batches, general EditCosts, bands beyond 33 diagonals, fewer than 16384 pairs, alphabets of more than 32
 * symbols or without a code: two bits for up to four symbols, else five bits with the byte's other three bits the same in every
 * symbol -- one case of the letters, the digits) run ta_levenshtein_k_batch as they are. */
int ta_levenshtein_k_batch_alphabet(const ta_strings *a, const ta_strings *b, size_t n, uint32_t k, const ta_edit_costs *costs,
                                    const uint8_t *alphabet, size_t alphabet_len, uint32_t *out_dev, void *stream) {
    int rc = check_batch_args(a, b, n, out_dev);
    if (rc) return rc;
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (!device_ready()) return TA_ERR_HIP;
    if (n == 0) return TA_OK;
    const bool fixed = !a->off && !b->off;
    const bool trans = costs->has_transpose != 0;
    const uint64_t max_len = fixed ? (a->len > b->len ? a->len : b->len) : 0;
    uint32_t u = 0, q_shift = 0, q_table = 0, q_memb = 0, q_hi = 0;
    const LevSwitches sw = lev_switches();
    const bool pinned = sw.no_bits || sw.force_na || sw.bits_static || sw.force_d || env_int("TA_NO_BITSQ");
    if (!fixed || pinned || !alphabet ||
        !lev_bitsq_applies(k, costs->mismatch_cost, costs->gap_cost, costs->start_gap_cost, trans, trans ? costs->transpose_cost : 0, max_len, true, n, &u) ||
        alphabet_len == 0)
        return ta_levenshtein_k_batch(a, b, n, k, costs, out_dev, stream);
    // at most four symbols with a two-bit code: lev_bitsq_body.h; up to 32 with a five-bit code: lev_bitsqw_body.h
    const bool force_wide = env_int("TA_BITSQ_WIDE") != 0;
    const bool narrow = !force_wide && lev_bitsq_hash(alphabet, alphabet_len, &q_shift, &q_table);
    if (!narrow) {
        if (env_int("TA_NO_BITSQW") || !lev_bitsqw_hash(alphabet, alphabet_len, &q_shift, &q_memb, &q_hi))
            return ta_levenshtein_k_batch(a, b, n, k, costs, out_dev, stream);
        // Where the 5-bit-code kernel pays (measured, profiles/r04/ab_alphabet.md): its per-16-rows conversion grows with the groups of
        // four codes that hold a symbol, and narrow bands have the two-pairs-per-lane byte test.  Beyond 4 groups (IUPAC's 16 letters
        // and the 20 amino acids: 7) or at 15 diagonals and fewer the byte-test kernels are as fast or faster: the general path runs.
        uint32_t groups = 0;
        for (uint32_t g4 = 0; g4 < 8; g4++) groups += ((q_memb >> (4u * g4)) & 15u) ? 1u : 0u;
        if (!force_wide && (groups > 4 || (uint64_t)u + 1u + (trans ? 2u : 0u) <= 15u))
            return ta_levenshtein_k_batch(a, b, n, k, costs, out_dev, stream);
    }
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    Scratch &bad = tls_scratch(SLOT_ALPHA_BAD), &cnt = tls_scratch(SLOT_ALPHA_COUNT);
    // two counters taken in turn: this pass appends to one and zeroes the other for the next pass (no fill per call; both are
    // zeroed once, when the scratch is allocated)
    // (`clean`: the last pass of this thread ran to its last launch -- the counter it left behind is zero.  A pass that failed midway leaves
    // it unknown: both counters are zeroed again and the turn restarts.)
    static thread_local uint32_t turn = 0;
    static thread_local bool clean = false;
    const bool fresh = cnt.cap < 64 || !clean;
    if ((rc = bad.ensure(n * 4)) || (rc = cnt.ensure(64))) return rc;
    if (fresh) { TA_HIP(hipMemsetAsync(cnt.dev, 0, 64, st)); turn = 0; }
    clean = false;
    uint32_t *counters = (uint32_t *)cnt.dev;
    const uint32_t mine = turn & 1u;
    turn++;
    LevParams P;
    P.a = view_of(a); P.b = view_of(b);
    P.subset = nullptr; P.trace = nullptr; P.out = out_dev; P.n = (uint32_t)n; P.k = k;
    P.mc = 1; P.gc = 1; P.sg = 0; P.tc = trans ? 1 : 0;
    P.u = u; P.o = 0; P.L = 1; P.PW = 64; P.lds_per_wave = 0; P.Tw = 0; P.ch = 0;
    P.q_table = q_table; P.q_shift = q_shift; P.q_memb = q_memb; P.q_hi = q_hi; P.q_ns = (uint32_t)alphabet_len; P.q_bad_count = counters + 8u * mine; P.q_bad_list = (uint32_t *)bad.dev;
    P.q_next_count = counters + 8u * (mine ^ 1u);
    ta_launch_info li = {};
    li.transpose = trans;
    li.cell_bits = launch_cell_bits(max_len, k, costs);
    uint32_t grid = 0, lds = 0;
    if (narrow) TA_HIP(lev_bitsq_launch(P, trans, st, &grid, &lds));
    else TA_HIP(lev_bitsqw_launch(P, trans, st, &grid, &lds));
    li.kernel = 7; li.diags_per_lane = 33; li.lanes_per_pair = 1; li.pairs_per_wave = 64; li.grid = grid; li.lds_bytes = lds;
    // the pairs that hold a byte outside the alphabet: the byte-test kernel over the list the first kernel wrote (its length is read
    // on the device; a small grid strides over it)
    const LevBitsPlan bp = lev_bits_make_plan(k, 1, 1, 0, trans, trans ? 1u : 0u, max_len, 0, 0, 0);
    LevParams F = P;
    F.subset = (const uint32_t *)bad.dev; F.n_dev = counters + 8u * mine;
    F.q_bad_count = nullptr; F.q_bad_list = nullptr; F.q_next_count = nullptr;
    F.u = bp.u; F.lds_per_wave = bp.lds_per_wave; F.Tw = bp.Tw; F.ch = bp.ch;
    char name[96];
    snprintf(name, sizeof(name), "%s", ta_last_kernel_name());
    TA_HIP(lev_bits_launch(F, bp, trans, max_len, st, nullptr, nullptr));
    set_last_kernel_name("%s", name);                   // the pass's dominant kernel is the first one
    if (env_int("TA_DEBUG")) fprintf(stderr, "[triple_accel_amd] lev pass: n=%zu k=%u u=%u kernel=7 (small alphabet, %s, shift %u table %08x) grid=%u lds=%u\n", n, k, u, narrow ? "2-bit codes" : "5-bit codes", q_shift, narrow ? q_table : q_memb, grid, lds);
    g_last_launch = li;
    g_answer_single_store = false;
    clean = true;
    return TA_OK;
}

int ta_levenshtein_exp_batch(const ta_strings *a, const ta_strings *b, size_t n,
                             const ta_edit_costs *costs, uint32_t *out_dev, void *stream) {
    int rc = check_batch_args(a, b, n, out_dev);
    if (rc) return rc;
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (!device_ready()) return TA_ERR_HIP;
    if (n == 0) return TA_OK;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    uint64_t max_len = 0;
    rc = batch_max_len(a, b, (uint32_t)n, st, &max_len);
    if (rc) return rc;
    // subset ping-pong buffers + counter
    Scratch &s0 = tls_scratch(SLOT_SUBSET_A), &s1 = tls_scratch(SLOT_SUBSET_B), &cnt = tls_scratch(SLOT_COUNT), &bnd = tls_scratch(SLOT_EXP_BOUND), &wrk = tls_scratch(SLOT_EXP_WORK);
    if ((rc = s0.ensure(n * 4)) || (rc = s1.ensure(n * 4)) || (rc = cnt.ensure(16))) return rc;
    // Bag lower bound per pair (util_kernels.hip): a doubling round only takes the unresolved pairs whose bound admits its
    // threshold -- the others could only return None from it.  Same return values, fewer rounds for dissimilar strings.
    const bool bounded = n >= 64 && max_len >= 64 && !env_int("TA_EXP_NO_BOUND") && !env_int("TA_EXP_FAITHFUL");
    if (bounded) {
        if ((rc = bnd.ensure(n * 4)) || (rc = wrk.ensure(n * 4))) return rc;
        TA_HIP(fill_u32_launch(out_dev, 0xFFFFFFFFu, (uint32_t)n, st));
        TA_HIP(bag_bound_launch(view_of(a), view_of(b), (uint32_t)n, costs->mismatch_cost, costs->gap_cost, (uint32_t *)bnd.dev, st));
    }
    g_exp_passes = 0;
    uint32_t *sub_in = nullptr, *bufs[2] = {(uint32_t *)s0.dev, (uint32_t *)s1.dev};
    uint32_t n_left = (uint32_t)n;                          // unresolved pairs (sub_in == nullptr: all of them)
    // the threshold schedule (lev_route.h: lev_exp_first_k, lev_exp_finish_now, lev_exp_next_k), the same for both loops below
    const LevSwitches sw = lev_switches();
    const LevCosts lc = costs_of(costs);
    const bool dpo = sw.no_bits, faithful = env_int("TA_EXP_FAITHFUL") != 0;
    const uint32_t k_first = lev_exp_first_k(lc, faithful);
    uint32_t k = k_first;
    // ragged (CSR) batches: the rounds take their pairs in length order, as ta_levenshtein_k_batch does (the list of the still
    // unresolved pairs is compacted from the ordered one, which keeps it ordered block by block)
    if (lev_wants_length_order(a->off || b->off, n, max_len) && !env_int("TA_NO_LENGTH_ORDER")) {
        const uint32_t u0 = lev_batch_unit_k(k, costs->mismatch_cost, costs->gap_cost, costs->start_gap_cost, max_len);
        const uint32_t *ordered = nullptr;
        if ((rc = order_pairs(a, b, (uint32_t)n, u0, max_len, !costs_scale(costs) || sw.no_bits, false, SLOT_ORDER, SLOT_ORDER_BINS, st, &ordered, nullptr))) return rc;
        sub_in = (uint32_t *)ordered;
    }
    int flip = 0;
    // Big batches: the rounds are DEVICE-DRIVEN -- every list (the pairs a round works on, the pairs it leaves unresolved) carries its
    // length in a device counter that the next kernel reads, every launch is sized for the list's upper bound (the batch) and the
    // wavefronts behind its end leave at once: the whole k schedule is enqueued without a host round trip between rounds, the call
    // returns while the device works (and can be captured in a hipGraph).  The schedule itself is the host-driven one's for a list that
    // never shrinks: k = 30, 60, ... until a bounded pass would cost more than a quarter of the unbounded one, then k = u32::MAX -- a
    // round whose list is empty costs its (empty) launches, 10-15 us.  Small batches (a lone pair's first round is the unbounded one;
    // the kernel choice follows the number of pairs left) keep the host-driven loop below.  TA_EXP_HOST_ROUNDS=1 pins it.
    if (n >= 1024 && !faithful && !env_int("TA_EXP_HOST_ROUNDS")) {
        constexpr int MAX_ROUNDS = 40;
        if ((rc = cnt.ensure(2 * MAX_ROUNDS * 4))) return rc;
        TA_HIP(fill_u32_launch((uint32_t *)cnt.dev, 0u, 2 * MAX_ROUNDS, st));
        uint32_t *counters = (uint32_t *)cnt.dev;
        const uint32_t *n_in_dev = nullptr;                 // the length of sub_in (nullptr: n, exactly)
        for (int round = 0; round < MAX_ROUNDS; round++) {
            if (k != 0xFFFFFFFFu && lev_exp_finish_now(k, lc, max_len, dpo, (uint32_t)n)) k = 0xFFFFFFFFu;
            const uint32_t *work = sub_in, *work_n_dev = n_in_dev;
            if (bounded && k != 0xFFFFFFFFu) {
                TA_HIP(compact_bound_launch(out_dev, (const uint32_t *)bnd.dev, k, sub_in, (uint32_t)n, n_in_dev, (uint32_t *)wrk.dev, counters + 2 * round, st));
                work = (const uint32_t *)wrk.dev;
                work_n_dev = counters + 2 * round;
            }
            rc = lev_pass(a, b, (uint32_t)n, work, k, costs, max_len, out_dev, st, false, work_n_dev);
            g_exp_passes++;
            if (rc) return rc;
            if (k == 0xFFFFFFFFu) break;                    // the unbounded pass answers every pair it is given (all that were left)
            TA_HIP(compact_none_launch(out_dev, sub_in, (uint32_t)n, n_in_dev, bufs[flip], counters + 2 * round + 1, st));
            sub_in = bufs[flip];
            n_in_dev = counters + 2 * round + 1;
            flip ^= 1;
            k = lev_exp_next_k(k, round, k_first, lc.gc);
        }
        g_answer_single_store = false;
        return TA_OK;
    }
    for (int round = 0; round < 40 && n_left > 0; round++) {
        if (!faithful && k != 0xFFFFFFFFu && lev_exp_finish_now(k, lc, max_len, dpo, n_left)) k = 0xFFFFFFFFu;
        const uint32_t *work = sub_in;
        uint32_t n_work = n_left;
        if (bounded && k != 0xFFFFFFFFu) {
            TA_HIP(hipMemsetAsync(cnt.dev, 0, 4, st));
            TA_HIP(compact_bound_launch(out_dev, (const uint32_t *)bnd.dev, k, sub_in, n_left, nullptr, (uint32_t *)wrk.dev, (uint32_t *)cnt.dev, st));
            TA_HIP(hipMemcpyAsync(&n_work, cnt.dev, 4, hipMemcpyDeviceToHost, st));
            TA_HIP(hipStreamSynchronize(st));
            work = (const uint32_t *)wrk.dev;
        }
        if (n_work > 0) {
            // (the compacted lists keep the order block by block only -- a wavefront may straddle two blocks' shares: the chunk form,
            // which takes any mix of lengths in one pass, stays the rounds' kernel)
            rc = lev_pass(a, b, n_work, work, k, costs, max_len, out_dev, st);
            g_exp_passes++;
            if (rc) return rc;
            if (k == 0xFFFFFFFFu) break;                    // the unbounded pass answers every pair it is given (all that were left)
            TA_HIP(hipMemsetAsync(cnt.dev, 0, 4, st));
            TA_HIP(compact_none_launch(out_dev, sub_in, n_left, nullptr, bufs[flip], (uint32_t *)cnt.dev, st));
            uint32_t left = 0;
            TA_HIP(hipMemcpyAsync(&left, cnt.dev, 4, hipMemcpyDeviceToHost, st));
            TA_HIP(hipStreamSynchronize(st));
            sub_in = bufs[flip];
            flip ^= 1;
            n_left = left;
        }
        k = lev_exp_next_k(k, round, k_first, lc.gc);
    }
    return TA_OK;
}

// The sliced form of hamming (ham_long.hip).  ham_wants_slices (lev_plan.h) is the rule; under TA_TUNING,
// TA_FORCE_HAM_SLICED=1 / =0 pin the route and TA_HAM_SLICE=<bytes> (a multiple of 1,024, at least 1,024) sets the slice length.
}  // extern "C"
namespace ta {
uint32_t ham_slice_setting() {
    const int v = env_int("TA_HAM_SLICE");
    return v >= 1024 && v % 1024 == 0 && v <= (1 << 28) ? (uint32_t)v : HAM_LONG_SLICE;
}
// the smallest length bound the two sides state for a pair of EQUAL lengths (the others are TA_NONE whatever their lengths); 0: none
static uint64_t ham_len_hint(const ta_strings *a, const ta_strings *b) {
    const uint64_t ha = side_bound_known(a) ? side_bound(a) : 0, hb = side_bound_known(b) ? side_bound(b) : 0;
    return ha && hb ? (ha < hb ? ha : hb) : (ha ? ha : hb);
}
static bool ham_route_sliced(const ta_strings *a, const ta_strings *b, size_t n) {
    const bool strided = !a->off && !b->off;
    if (strided && a->len != b->len) return false;          // every answer is TA_NONE: nothing to slice
    bool sliced = ham_wants_slices(n, strided, a->len, strided ? 0 : ham_len_hint(a, b));
    if (const char *f = env_str("TA_FORCE_HAM_SLICED")) sliced = atoi(f) != 0;
    return sliced;
}
// the sliced pass over a device batch: plan (CSR), slices, finish -- out_dev[i] is stored exactly once, by the finish kernel
static int ham_long_pass(const StrView &a, const StrView &b, uint32_t n, uint32_t *out_dev, hipStream_t st, bool *taken) {
    const uint32_t S = ham_slice_setting();
    const uint64_t words = ham_long_scratch_words(a, b, n, S);
    *taken = words != 0;
    if (!words) return TA_OK;                                // more than 2^31 slices: the batch fills the chip by count
    Scratch &sc = tls_scratch(SLOT_HAM_LONG);
    int rc = sc.ensure(words * 4u);
    if (rc) return rc;
    TA_HIP(ham_long_launch(a, b, n, S, (uint32_t *)sc.dev, out_dev, st));
    return TA_OK;
}
}  // namespace ta
extern "C" {

int ta_hamming_batch(const ta_strings *a, const ta_strings *b, size_t n, uint32_t *out_dev, void *stream) {
    int rc = check_batch_args(a, b, n, out_dev);
    if (rc) return rc;
    if (!device_ready()) return TA_ERR_HIP;
    if (n == 0) return TA_OK;
    StreamGuard guard((hipStream_t)stream);
    if (ham_route_sliced(a, b, n)) {
        bool taken = false;
        if ((rc = ham_long_pass(view_of(a), view_of(b), (uint32_t)n, out_dev, (hipStream_t)stream, &taken))) return rc;
        if (taken) return TA_OK;
    }
    TA_HIP(hamming_batch_launch(view_of(a), view_of(b), (uint32_t)n, out_dev, (hipStream_t)stream));
    return TA_OK;
}

int ta_hamming_dev(const uint8_t *a_dev, const uint8_t *b_dev, size_t len, uint32_t *out_dev, void *stream) {
    if (!out_dev || (len && (!a_dev || !b_dev))) return TA_ERR_ARG;
    if (len >= 0xFFFFFFFFull) return TA_ERR_UNSUPPORTED;     // the count is a u32 and 0xFFFFFFFF is TA_NONE
    if (!device_ready()) return TA_ERR_HIP;
    StreamGuard guard((hipStream_t)stream);
    const StrView va = {a_dev, nullptr, 0, len}, vb = {b_dev, nullptr, 0, len};
    bool sliced = ham_wants_slices(1, true, len, 0);         // ta_hamming_batch's rule for one strided pair
    if (const char *f = env_str("TA_FORCE_HAM_SLICED")) sliced = atoi(f) != 0;
    if (sliced) {
        bool taken = false;
        return ham_long_pass(va, vb, 1, out_dev, (hipStream_t)stream, &taken);      // (one pair of < 4 GiB: always taken)
    }
    TA_HIP(hamming_batch_launch(va, vb, 1, out_dev, (hipStream_t)stream));           // one wavefront; it too reads nothing past len
    return TA_OK;
}

/* ---------------------------------------------------------------- queue: pairs pushed one at a time, answered by one batch pass */
}  // extern "C"

struct ta_queue {
    uint32_t k;
    ta_edit_costs costs;
    std::vector<uint8_t> blob[2];          // the pushed strings back to back (a: 0, b: 1)
    std::vector<uint64_t> off[2];          // CSR offsets (n + 1)
    uint64_t max_len = 0;
    std::vector<uint32_t> results;
    void *dev = nullptr;                   // device staging: [a blob | b blob | a offsets | b offsets | results]
    size_t dev_cap = 0;
    hipStream_t st = nullptr;
};

extern "C" {

int ta_queue_create(uint32_t k, const ta_edit_costs *costs, ta_queue **out) {
    if (!out) return TA_ERR_ARG;
    *out = nullptr;
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (!device_ready()) return TA_ERR_HIP;
    ta_queue *q = new ta_queue();
    q->k = k; q->costs = *costs;
    q->off[0].push_back(0); q->off[1].push_back(0);
    if (hipStreamCreateWithFlags(&q->st, hipStreamNonBlocking) != hipSuccess) { delete q; return TA_ERR_HIP; }
    *out = q;
    return TA_OK;
}

int ta_queue_push(ta_queue *q, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, size_t *ticket) {
    if (!q || (!a && a_len) || (!b && b_len) || a_len > 0xFFFFFFF0ull || b_len > 0xFFFFFFF0ull) return TA_ERR_ARG;
    if (q->off[0].size() > 0xFFFFFFF0ull) return TA_ERR_CAPACITY;
    if (ticket) *ticket = q->off[0].size() - 1;
    q->blob[0].insert(q->blob[0].end(), a, a + a_len);
    q->blob[1].insert(q->blob[1].end(), b, b + b_len);
    q->off[0].push_back(q->blob[0].size());
    q->off[1].push_back(q->blob[1].size());
    const uint64_t m = a_len > b_len ? a_len : b_len;
    if (m > q->max_len) q->max_len = m;
    return TA_OK;
}

// A flush that fails (an over-wide band, an allocation failure) DROPS the queued pairs: the queue is empty afterwards and accepts new
// pairs -- a queue that kept them would fail the same way on every later flush.
static int queue_flush_impl(ta_queue *q, const uint32_t **results, size_t n);
int ta_queue_flush(ta_queue *q, const uint32_t **results, size_t *n_out) {
    if (!q || !results || !n_out) return TA_ERR_ARG;
    const size_t n = q->off[0].size() - 1;
    *results = nullptr; *n_out = n;
    q->results.assign(n, 0);
    if (n == 0) return TA_OK;
    const int rc = queue_flush_impl(q, results, n);
    for (int s = 0; s < 2; s++) { q->blob[s].clear(); q->off[s].assign(1, 0); }
    q->max_len = 0;
    if (rc) { *n_out = 0; *results = nullptr; }
    return rc;
}
static int queue_flush_impl(ta_queue *q, const uint32_t **results, size_t n) {
    // more than one device in the set and enough pairs for more than one of them: contiguous slices of the queue, one per device, each
    // uploaded through its worker's pinned ring and answered on its own GPU (ta_multi.hip)
    if (multi_pair_shards(n) > 1) {
        const ta_strings A = {q->blob[0].data(), q->off[0].data(), 0, 0, 0}, B = {q->blob[1].data(), q->off[1].data(), 0, 0, 0};
        int rc = ta_levenshtein_k_batch_host(&A, &B, n, q->k, &q->costs, q->results.data());
        if (rc) return rc;
        *results = q->results.data();
        return TA_OK;
    }
    auto pad = [](size_t x) { return (x + TA_BLOB_SLACK + 255) & ~(size_t)255; };
    const size_t sa = pad(q->blob[0].size()), sb = pad(q->blob[1].size()), so = pad((n + 1) * 8), sr = pad(n * 4);
    const size_t need = sa + sb + 2 * so + sr;
    if (need > q->dev_cap) {
        if (q->dev) (void)hipFree(q->dev);
        q->dev = nullptr; q->dev_cap = 0;
        TA_HIP(hipMalloc(&q->dev, need + need / 2));
        q->dev_cap = need + need / 2;
    }
    uint8_t *base = (uint8_t *)q->dev;
    uint8_t *da = base, *db = base + sa, *doa = base + sa + sb, *dob = doa + so, *dr = dob + so;
    hipStream_t st = q->st;
    if (!q->blob[0].empty()) TA_HIP(hipMemcpyAsync(da, q->blob[0].data(), q->blob[0].size(), hipMemcpyHostToDevice, st));
    if (!q->blob[1].empty()) TA_HIP(hipMemcpyAsync(db, q->blob[1].data(), q->blob[1].size(), hipMemcpyHostToDevice, st));
    TA_HIP(hipMemcpyAsync(doa, q->off[0].data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    TA_HIP(hipMemcpyAsync(dob, q->off[1].data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    ta_strings A = {da, (const uint64_t *)doa, 0, 0, q->max_len ? q->max_len : 1}, B = {db, (const uint64_t *)dob, 0, 0, q->max_len ? q->max_len : 1};
    int rc = ta_levenshtein_k_batch(&A, &B, n, q->k, &q->costs, (uint32_t *)dr, st);
    if (rc) return rc;
    TA_HIP(hipMemcpyAsync(q->results.data(), dr, n * 4, hipMemcpyDeviceToHost, st));
    TA_HIP(hipStreamSynchronize(st));
    *results = q->results.data();
    return TA_OK;
}

void ta_queue_destroy(ta_queue *q) {
    if (!q) return;
    if (q->st) { (void)hipStreamSynchronize(q->st); (void)hipStreamDestroy(q->st); }
    if (q->dev) (void)hipFree(q->dev);
    delete q;
}

}  // extern "C"

/* ---------------------------------------------------------------- single-call host API */
namespace ta {

// One (a, b) pair of a single call (Staged, ta_internal.h).  Short pairs go into the thread's pinned, device-mapped buffer: the kernel
// reads the strings in place and writes its answer next to them (`*out_host` then reads it after one stream synchronisation).  Long
// pairs are copied to thread-local device scratch on the thread's stream.  Either way the call runs on the thread's own
// non-blocking stream `*st`.
int stage_pair(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, Staged *S) {
    if ((!a && a_len) || (!b && b_len)) return TA_ERR_ARG;
    if (a_len > 0xFFFFFFF0ull || b_len > 0xFFFFFFF0ull) return TA_ERR_ARG;
    if (!device_ready()) return TA_ERR_HIP;
    CallCtx &cx = call_ctx();
    int rc = cx.ensure();
    if (rc) return rc;
    S->st = cx.st;
    const size_t a_pad = (a_len + TA_BLOB_SLACK + 255) & ~(size_t)255, b_pad = (b_len + TA_BLOB_SLACK + 255) & ~(size_t)255;
    if (a_pad + b_pad <= CallCtx::RESULT_OFF) {
        if (a_len) memcpy(cx.pin, a, a_len);
        if (b_len) memcpy(cx.pin + a_pad, b, b_len);
        S->sa = ta_strings{cx.pin_dev, nullptr, 0, a_len, a_len};
        S->sb = ta_strings{cx.pin_dev + a_pad, nullptr, 0, b_len, b_len};
        S->out_dev = (uint32_t *)(cx.pin_dev + CallCtx::RESULT_OFF);
        S->out_host = (volatile uint32_t *)(cx.pin + CallCtx::RESULT_OFF);
        *S->out_host = TA_SLOT_EMPTY;
        return TA_OK;
    }
    Scratch &sc = tls_scratch(SLOT_PAIR_STAGE);
    if ((rc = sc.ensure(a_pad + b_pad + 256))) return rc;
    uint8_t *base = (uint8_t *)sc.dev;
    if (a_len) TA_HIP(hipMemcpyAsync(base, a, a_len, hipMemcpyHostToDevice, cx.st));
    if (b_len) TA_HIP(hipMemcpyAsync(base + a_pad, b, b_len, hipMemcpyHostToDevice, cx.st));
    S->sa = ta_strings{base, nullptr, 0, a_len, a_len};
    S->sb = ta_strings{base + a_pad, nullptr, 0, b_len, b_len};
    S->out_dev = (uint32_t *)(base + a_pad + b_pad);
    S->out_host = nullptr;
    return TA_OK;
}

// `single_store`: the call was ONE kernel whose only write to the result slot is its answer.  The slot then starts out as a
// value no answer can take, and the host watches the pinned word instead of going through the runtime's completion
// machinery (the store becomes visible no later than the kernel's end-of-kernel release); after 20 ms without an answer the
// ordinary stream synchronisation takes over (and reports a fault, if that is what happened).
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#else
    __asm__ __volatile__("" ::: "memory");
#endif
}
int fetch_u32(const Staged &S, uint32_t *out, bool single_store /* = false */) {
    if (S.out_host) {
        if (single_store) {
            // watch the word (the answer of a short pair arrives within ~10-25 us, of a 4 KiB pair within ~0.6 ms; the runtime's own
            // wait costs ~40 us more than the watch), for at most 2 ms: then the runtime's wait takes over
            const auto t0 = std::chrono::steady_clock::now();
            for (uint32_t spin = 0; *S.out_host == TA_SLOT_EMPTY; spin++) {
                cpu_relax();
                if ((spin & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
            }
            const uint32_t v = *S.out_host;
            if (v != TA_SLOT_EMPTY) { *out = v; return TA_OK; }
        }
        TA_HIP(hipStreamSynchronize(S.st));
        *out = *S.out_host;
        return TA_OK;
    }
    TA_HIP(hipMemcpyAsync(out, S.out_dev, 4, hipMemcpyDeviceToHost, S.st));
    TA_HIP(hipStreamSynchronize(S.st));
    return TA_OK;
}

// hamming of a host pair longer than `chunk` bytes: the pair goes through two fixed device halves (one per string) chunk by chunk on the
// thread's stream -- copy, copy, sliced kernel with its partial counts appended -- and one finish kernel adds them up at the end.  The
// stream alone orders the steps (a chunk's copies wait for the kernel that read the halves before).  The device holds 2 x chunk bytes
// whatever the pair's length (stage_pair would hold the whole pair).
static int hamming_host_chunked(const uint8_t *a, const uint8_t *b, size_t len, size_t chunk, uint32_t *out) {
    if (!a || !b || len > 0xFFFFFFF0ull) return TA_ERR_ARG;
    if (!device_ready()) return TA_ERR_HIP;
    CallCtx &cx = call_ctx();
    int rc = cx.ensure();
    if (rc) return rc;
    StreamGuard guard(cx.st);
    const uint32_t S = ham_long_slice_bytes(len, ham_slice_setting());
    const size_t half = (chunk + 255) & ~(size_t)255, n_chunks = (len + chunk - 1) / chunk;
    Scratch &stage = tls_scratch(SLOT_PAIR_STAGE), &part = tls_scratch(SLOT_HAM_LONG);
    if ((rc = stage.ensure(2 * half + 256))) return rc;
    if ((rc = part.ensure((len / S + n_chunks + 1) * 4u))) return rc;
    uint8_t *da = (uint8_t *)stage.dev, *db = da + half;
    uint32_t *out_dev = (uint32_t *)(db + half), *partial = (uint32_t *)part.dev;
    uint32_t done = 0;
    for (size_t at = 0; at < len; at += chunk) {
        const size_t m = len - at < chunk ? len - at : chunk;
        TA_HIP(hipMemcpyAsync(da, a + at, m, hipMemcpyHostToDevice, cx.st));
        TA_HIP(hipMemcpyAsync(db, b + at, m, hipMemcpyHostToDevice, cx.st));
        TA_HIP(ham_long_chunk_launch(da, db, m, S, partial + done, cx.st));
        done += (uint32_t)((m + S - 1) / S);
    }
    TA_HIP(ham_long_sum_launch(partial, done, out_dev, cx.st));
    TA_HIP(hipMemcpyAsync(out, out_dev, 4, hipMemcpyDeviceToHost, cx.st));
    TA_HIP(hipStreamSynchronize(cx.st));
    return TA_OK;
}
}  // namespace ta
extern "C" {

int ta_hamming(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t *out) {
    if (!out) return TA_ERR_ARG;
    if (a_len != b_len) return TA_ERR_LEN_MISMATCH;          // src/hamming.rs:318
    size_t chunk = HAM_HOST_CHUNK;                           // bytes of each string on the device at a time; TA_HAM_HOST_CHUNK under TA_TUNING
    if (const int v = env_int("TA_HAM_HOST_CHUNK"); v >= 1024) chunk = (size_t)v;
    if (a_len > chunk) return hamming_host_chunked(a, b, a_len, chunk, out);
    Staged S;
    int rc = stage_pair(a, a_len, b, b_len, &S);
    if (rc) return rc;
    rc = ta_hamming_batch(&S.sa, &S.sb, 1, S.out_dev, S.st);
    if (rc) return rc;
    // either route stores the slot exactly once: the one kernel of hamming_batch_kernel, or the finish kernel of the sliced form (its
    // partial counts live in scratch, never in the slot) -- the pinned word can be watched
    return fetch_u32(S, out, true);
}

int ta_levenshtein_simd_k_with_opts(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len,
                                    uint32_t k, int trace_on, const ta_edit_costs *costs, uint32_t *out) {
    if (!out) return TA_ERR_ARG;
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (trace_on) return TA_ERR_UNSUPPORTED;
    if (!device_ready()) return TA_ERR_HIP;
    if (a_len == 0 && b_len == 0) { *out = 0; return TA_OK; }   // src/levenshtein.rs:721-727
    Staged S;
    int rc = stage_pair(a, a_len, b, b_len, &S);
    if (rc) return rc;
    rc = ta_levenshtein_k_batch(&S.sa, &S.sb, 1, k, costs, S.out_dev, S.st);
    if (rc) return rc;
    return fetch_u32(S, out, g_answer_single_store);         // lev_pass says whether the pass was one kernel with one store
}

int ta_levenshtein_simd_k(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t k, uint32_t *out) {
    ta_edit_costs c = ta_levenshtein_costs();
    return ta_levenshtein_simd_k_with_opts(a, a_len, b, b_len, k, 0, &c, out);
}
int ta_levenshtein(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t *out) {
    return ta_levenshtein_simd_k(a, a_len, b, b_len, 0xFFFFFFFFu, out);       // :1398
}
int ta_rdamerau(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t *out) {
    ta_edit_costs c = ta_rdamerau_costs();
    return ta_levenshtein_simd_k_with_opts(a, a_len, b, b_len, 0xFFFFFFFFu, 0, &c, out);   // :1420
}
int ta_levenshtein_exp_with_opts(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len,
                                 int trace_on, const ta_edit_costs *costs, uint32_t *out) {
    if (!out) return TA_ERR_ARG;
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (trace_on) return TA_ERR_UNSUPPORTED;
    if (!device_ready()) return TA_ERR_HIP;
    if (a_len == 0 && b_len == 0) { *out = 0; return TA_OK; }
    Staged S;
    int rc = stage_pair(a, a_len, b, b_len, &S);
    if (rc) return rc;
    rc = ta_levenshtein_exp_batch(&S.sa, &S.sb, 1, costs, S.out_dev, S.st);
    if (rc) return rc;
    // one pass, one kernel, one store (a short pair goes straight to the unbounded pass): the pinned word can be watched; after
    // several rounds the slot already holds an earlier round's None
    return fetch_u32(S, out, g_exp_passes == 1 && g_answer_single_store);
}
int ta_levenshtein_exp(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t *out) {
    ta_edit_costs c = ta_levenshtein_costs();
    return ta_levenshtein_exp_with_opts(a, a_len, b, b_len, 0, &c, out);
}
int ta_rdamerau_exp(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t *out) {
    ta_edit_costs c = ta_rdamerau_costs();
    return ta_levenshtein_exp_with_opts(a, a_len, b, b_len, 0, &c, out);
}

}  // extern "C"
