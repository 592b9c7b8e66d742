// ta_trace.hip -- the traceback entries of the C ABI (include/triple_accel_amd.h): ta_levenshtein_trace, ta_levenshtein_exp_trace and the
// two ta_levenshtein_trace_batch forms.  The single calls launch a kernel that leaves records and walk them on the host (lev_script.h: the
// script and the DP kernels' record layouts; lev_trace_walk.h: the row-blocked bit-parallel kernel's); the batch forms stay on the device.
// Staging, the distance pass and the thread's launch record are ta_api.hip's (ta_internal.h).
#include "lev_script.h"
#include "lev_trace_walk.h"
#include "ta_internal.h"

using namespace ta;

// a single call's answer into *out and, unless it is None, the `words` record words its kernel left in `ts` into *rec
static int fetch_records(const Staged &S, uint32_t *out, const Scratch &ts, uint64_t words, std::vector<uint32_t> *rec) {
    uint32_t d = 0;
    int rc = fetch_u32(S, &d);
    if (rc) return rc;
    *out = d;
    if (d == TA_NONE) return TA_OK;
    rec->resize((size_t)words);
    TA_HIP(hipMemcpy(rec->data(), ts.dev, (size_t)words * 4, hipMemcpyDeviceToHost));
    return TA_OK;
}

// trace_on = true beyond the register band (unit costs): row-blocked bit-parallel kernel with 3-bit records + host walk
static int trace_widebits(const uint8_t *x, size_t n, const uint8_t *y, size_t m, bool swap, uint32_t k, const ta_edit_costs *costs,
                          uint32_t *out, ta_edit **edits, size_t *n_edits, uint64_t rec_words, uint64_t tcols) {
    Staged S;
    int rc = stage_pair(x, n, y, m, &S);
    if (rc) return rc;
    Scratch &ts = tls_scratch(SLOT_TRACE), &bl = tls_scratch(SLOT_LINES);
    if ((rc = ts.ensure((size_t)rec_words * 4)) || (rc = bl.ensure((size_t)6 * (m + 66) * 4))) return rc;
    LevParams P;
    P.a = view_of(&S.sa); P.b = view_of(&S.sb);
    P.subset = nullptr; P.out = S.out_dev; P.n = 1; P.k = k;
    P.mc = 1; P.gc = 1; P.sg = 0; P.tc = costs->has_transpose ? 1 : 0;
    P.u = lev_batch_unit_k(k, 1, 1, 0, m);
    P.o = 0; P.L = 64; P.PW = 1; P.lds_per_wave = 0; P.Tw = 0; P.ch = 0;
    P.trace = (uint32_t *)ts.dev; P.trace_cols = tcols;
    P.bnd = (uint32_t *)bl.dev; P.bnd_line = (uint64_t)m + 66;
    TA_HIP(lev_widebits_trace_launch(P, costs->has_transpose != 0, S.st));
    std::vector<uint32_t> rec;
    if ((rc = fetch_records(S, out, ts, rec_words, &rec)) || *out == TA_NONE) return rc;
    WbTrace T{rec.data(), tcols, 2u, (uint32_t)n, (uint32_t)m, P.u};
    ScriptBuilder<uint8_t> walk(x, n, y, m, swap);
    const bool ok = wb_trace_walk(T, x, y, *out, costs->has_transpose != 0, [&](int c) { walk.step(c); });
    if (!ok) { set_last_error_msg("traceback records are inconsistent"); return TA_ERR_HIP; }
    walk.finish();
    return walk.release(edits, n_edits);
}

// trace_on = true beyond the register band, any EditCosts: the DP wide kernel with 2-bit argmin codes + the usual walk
static int trace_wide(const uint8_t *x, size_t n, const uint8_t *y, size_t m, bool swap, uint32_t k, const ta_edit_costs *costs,
                      uint32_t *out, ta_edit **edits, size_t *n_edits, uint64_t code_words, uint64_t tcols) {
    Staged S;
    int rc = stage_pair(x, n, y, m, &S);
    if (rc) return rc;
    Scratch &ts = tls_scratch(SLOT_TRACE);
    if ((rc = ts.ensure((size_t)code_words * 4))) return rc;
    LevParams P;
    P.a = view_of(&S.sa); P.b = view_of(&S.sb);
    P.subset = nullptr; P.out = S.out_dev; P.n = 1; P.k = k;
    P.mc = costs->mismatch_cost; P.gc = costs->gap_cost; P.sg = costs->start_gap_cost;
    P.tc = costs->has_transpose ? costs->transpose_cost : 0;
    P.u = lev_batch_unit_k(k, P.mc, P.gc, P.sg, m);
    P.o = 0; P.L = 0; P.PW = 1; P.Tw = 0; P.ch = 0;
    P.lds_per_wave = (uint32_t)(m + 2);                                         // boundary line length
    P.trace = (uint32_t *)ts.dev; P.trace_cols = tcols;
    TA_HIP(lev_wide_trace_launch(P, costs->has_transpose != 0, S.st));
    std::vector<uint32_t> tr;
    if ((rc = fetch_records(S, out, ts, code_words, &tr)) || *out == TA_NONE) return rc;
    ScriptBuilder<uint8_t> walk(x, n, y, m, swap);
    while (walk.i() > 0 || walk.j() > 0) walk.step(wide_trace_code(tr.data(), tcols, walk.i(), walk.j()));   // :561-603
    walk.finish();
    return walk.release(edits, n_edits);
}

// The checkpoint-and-recompute traceback of one (sub-)batch of the unit-cost families, bands of up to 33 diagonals: the
// caller (ta_levenshtein_trace_batch) has validated the arguments and bounded n so that n x runs_cap fits 32 bits and the scratch fits memory.
// packed != nullptr: the packed form -- the walk writes the runs straight into the caller's buffer (cap words per pair, right-aligned): no run
// lists in scratch, no last step.
static int trace_bits_batch(const ta_strings *a, const ta_strings *b, size_t n, uint32_t k, const ta_edit_costs *costs, uint64_t max_len,
                            uint32_t *out_dev, ta_edit *edits_dev, uint32_t *n_edits_dev, size_t cap, hipStream_t st, uint32_t *packed = nullptr) {
    int rc;
    const bool trans = costs->has_transpose != 0;
    const uint32_t u = lev_batch_unit_k(k, 1, 1, 0, max_len);
    // Fixed-length batches: the distance pass IS the forward sweep -- the stride-8 kernel's CKPT instantiation stores the column
    // state in front of every 16th column (rows = the shorter string: the views are swapped for it where a is the longer one; the
    // distance is symmetric; CSR batches: pair by pair inside the kernel).  TA_TRACE_OWN_SWEEP=1 pins the trace kernel's own sweep
    // (TA_TRACE_CSR_OWN_SWEEP=1: for CSR batches only, an A/B).
    const bool fixed = !a->off && !b->off;
    const LevBitsPlan bp8 = lev_bits_make_plan(k, 1, 1, 0, trans, trans ? 1u : 0u, max_len, 0, 0, 3);
    const bool fold = bp8.ok && bp8.s8 && !env_int("TA_TRACE_OWN_SWEEP") && !env_int("TA_TRACE_TILE") && (fixed || !env_int("TA_TRACE_CSR_OWN_SWEEP"));
    const uint32_t tile = fold ? 16u : lev_bits_trace_tile(), tiles = (uint32_t)((max_len + tile - 1) / tile) + 1u, waves = (uint32_t)((n + 63) / 64);
    // CSR batches: both kernels run a wavefront to the longest of its 64 pairs -- the pairs are taken in length order (as
    // ta_levenshtein_k_batch takes them), the same list for the distance pass and the trace kernel.  TA_NO_LENGTH_ORDER=1 keeps the batch order.
    const uint32_t *order = nullptr;
    if (lev_wants_length_order(!fixed, n, max_len) && !env_int("TA_NO_LENGTH_ORDER") &&
        (rc = order_pairs(a, b, (uint32_t)n, u, max_len, false, false, SLOT_ORDER, SLOT_ORDER_BINS, st, &order, nullptr))) return rc;
    if (!fold && (rc = lev_pass(a, b, (uint32_t)n, order, k, costs, max_len, out_dev, st))) return rc;
    // (a script of cost <= u has at most 2 u + 1 runs, and never more than n + m)
    uint32_t runs_cap = (uint32_t)(2 * max_len + 1 < 2ull * u + 2 ? 2 * max_len + 1 : 2ull * u + 2);
    Scratch &cs = tls_scratch(SLOT_TRACE), &ps = tls_scratch(SLOT_AUX_B), &ss = tls_scratch(SLOT_AUX_A);
    if ((rc = cs.ensure((size_t)waves * tiles * lev_bits_trace_ckpt_words(trans) * 64u * 4u)) || (!packed && (rc = ps.ensure((size_t)n * runs_cap * 4u))) ||
        (rc = ss.ensure((size_t)n * 4u))) return rc;
    LevBitsTraceParams T;
    T.a = view_of(a); T.b = view_of(b); T.dist = out_dev; T.n = (uint32_t)n; T.u = u;
    T.ckpt = (uint32_t *)cs.dev; T.ckpt_tiles = tiles; T.runs = (uint32_t *)ps.dev; T.runs_cap = env_int("TA_TRACE_SKIP_WALK") ? 0u : runs_cap; T.n_runs = (uint32_t *)ss.dev;
    T.subset = order;
    if (packed) { T.runs = packed; T.packed_cap = (uint32_t)cap; }
    if (fold) {
        const bool sw = fixed && a->len > b->len;              // (CSR batches: the kernel swaps pair by pair)
        LevParams P;
        P.a = view_of(sw ? b : a); P.b = view_of(sw ? a : b);
        P.subset = order; P.trace = nullptr; P.out = out_dev; P.n = (uint32_t)n; P.k = k;
        P.mc = 1; P.gc = 1; P.sg = 0; P.tc = trans ? 1 : 0;
        P.u = bp8.u; P.o = 0; P.L = 1; P.PW = 64; P.lds_per_wave = bp8.lds_per_wave; P.Tw = bp8.Tw; P.ch = bp8.ch;
        P.ckpt = (uint32_t *)cs.dev; P.ckpt_tiles = tiles;
        TA_HIP(lev_bits_launch(P, bp8, trans, max_len, st, nullptr, nullptr));
        ta_launch_info l0 = {};
        l0.cell_bits = launch_cell_bits(max_len, k, costs); l0.transpose = trans;
        last_launch() = l0;
    }
    ta_launch_info li = last_launch();                 // (the distance pass's: kernel 3)
    uint32_t grid = 0, lds = 0;
    TA_HIP(lev_bits_trace_launch(T, trans, fold, edits_dev, n_edits_dev, cap, st, &grid, &lds));
    li.kernel = 8; li.diags_per_lane = 33; li.lanes_per_pair = 1; li.pairs_per_wave = 64; li.grid = grid; li.lds_bytes = lds;
    last_launch() = li;
    return TA_OK;
}

// both forms of ta_levenshtein_trace_batch (below): edits_dev or packed_dev is the caller's buffer, the other nullptr
static int trace_batch_impl(const ta_strings *a, const ta_strings *b, size_t n, uint32_t k, const ta_edit_costs *costs,
                            uint32_t *out_dev, ta_edit *edits_dev, uint32_t *packed_dev, uint32_t *n_edits_dev, size_t cap, void *stream) {
    int rc = check_batch_args(a, b, n, out_dev);
    if (rc) return rc;
    if (n && (!n_edits_dev || cap == 0)) { set_last_error_msg("bad batch arguments"); return TA_ERR_ARG; }
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (!device_ready()) return TA_ERR_HIP;
    if (n == 0) return TA_OK;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    uint64_t max_len = 0;
    if ((rc = batch_max_len(a, b, (uint32_t)n, st, &max_len))) return rc;
    const uint32_t gc = costs->gap_cost, sg = costs->start_gap_cost;
    if (packed_dev && (max_len >= (1ull << 29) || cap > 0xFFFFFFFFull)) { set_last_error_msg("packed tracebacks: strings of 2^29 bytes and more"); return TA_ERR_UNSUPPORTED; }
    // Unit costs times g (lev_unit_scale): every alignment costs g times its unit cost, every comparison of the recurrence and of the walk
    // keeps its outcome -- the script IS the unit-cost script for k / g, the distance g times the unit one (3.4c): the checkpoint kernel
    // serves EditCosts(g, g, 0, None | Some(g)) too.  The no_unit_scale switch (lev_route.h: LevSwitches) keeps the DP band kernel's records.
    const LevSwitches sw = lev_switches();
    if (const uint32_t g = lev_unit_scale(costs->mismatch_cost, gc, sg, costs->has_transpose != 0, costs->transpose_cost);
        g && !sw.no_bits && !sw.no_unit_scale && !env_int("TA_TRACE_NO_BITS")) {
        const bool tr = costs->has_transpose != 0;
        const uint32_t uu = lev_batch_unit_k(k / g, 1, 1, 0, max_len);
        if ((uint64_t)uu + 1u + (tr ? 2u : 0u) <= 33u && max_len < (1ull << 29)) {
            const ta_edit_costs uc = unit_costs(tr);
            if ((rc = trace_batch_impl(a, b, n, k / g, &uc, out_dev, edits_dev, packed_dev, n_edits_dev, cap, stream))) return rc;
            TA_HIP(scale_results_launch(out_dev, nullptr, (uint32_t)n, nullptr, g, st));
            last_launch().cell_bits = launch_cell_bits(max_len, k, costs);
            return TA_OK;
        }
    }
    // LEVENSHTEIN_COSTS / RDAMERAU_COSTS with a band of up to 33 diagonals (k <= 32; 30 with the transposition term): no per-cell records --
    // the distance pass, then ONE kernel that sweeps the columns forwards with a checkpoint (8 bytes per pair) every 16 columns, recomputes
    // tile after tile backwards with the column states of the tile in LDS, walks, and writes the runs (lev_bits_trace_body.h): 2 x the
    // strings' bytes instead of 21 x.  TA_TRACE_NO_BITS=1 keeps the DP band kernel's records for these cost sets too.
    {
        const bool trans = costs->has_transpose != 0;
        const uint32_t u = lev_batch_unit_k(k, 1, 1, 0, max_len);
        if (costs_unit(costs) && (uint64_t)u + 1u + (trans ? 2u : 0u) <= 33u && max_len < (1ull << 29) /* a run's count has 29 bits */ && !env_int("TA_TRACE_NO_BITS") && !sw.no_bits) {
            // The kernel indexes its run lists with 32 bits (pair slot x runs_cap) and its scratch -- checkpoints, run lists, run counts -- is
            // proportional to the pairs of a launch: a batch beyond either bound is worked through in chunks of whole wavefronts, each an
            // ordinary sub-batch on the same stream (65M pairs at k = 32 wrapped the index; a huge batch asked for all of its
            // scratch at once where the record path below chunks by free memory).  TA_TRACE_CHUNK_PAIRS=n pins the chunk (tests).
            const uint32_t runs_cap = (uint32_t)(2 * max_len + 1 < 2ull * u + 2 ? 2 * max_len + 1 : 2ull * u + 2);
            const uint64_t tiles16 = (max_len + 15) / 16 + 1;
            const uint64_t per_pair = tiles16 * lev_bits_trace_ckpt_words(trans) * 4ull + (uint64_t)runs_cap * 4ull + 4ull + 8ull;
            uint64_t chunk = 0xFFFFFFF0ull / (packed_dev ? (cap > runs_cap ? (uint64_t)cap : runs_cap) : (runs_cap ? runs_cap : 1u));
            const uint64_t held = tls_scratch(SLOT_TRACE).cap + tls_scratch(SLOT_AUX_B).cap + tls_scratch(SLOT_AUX_A).cap;
            if (per_pair * n > held && !stream_is_capturing(st)) {   // the scratch has to grow: not beyond half of what is free right now
                size_t free_b = 0, total_b = 0;
                if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
                    const uint64_t by_mem = (((uint64_t)free_b + held) / 2) / per_pair;
                    if (by_mem < chunk) chunk = by_mem;
                }
            }
            if (env_int("TA_TRACE_CHUNK_PAIRS") > 0) chunk = (uint64_t)env_int("TA_TRACE_CHUNK_PAIRS");
            chunk &= ~63ull;
            if (chunk < 64) chunk = 64;
            if (chunk >= n) return trace_bits_batch(a, b, n, k, costs, max_len, out_dev, edits_dev, n_edits_dev, cap, st, packed_dev);
            for (uint64_t lo = 0; lo < n; lo += chunk) {
                const size_t cnt = (size_t)((n - lo) < chunk ? (n - lo) : chunk);
                const ta_strings sa = strings_slice(a, lo, max_len), sb = strings_slice(b, lo, max_len);
                if ((rc = trace_bits_batch(&sa, &sb, cnt, k, costs, max_len, out_dev + lo, edits_dev ? edits_dev + lo * cap : nullptr, n_edits_dev + lo, cap, st,
                                           packed_dev ? packed_dev + lo * cap : nullptr))) return rc;
            }
            return TA_OK;
        }
    }
    if (packed_dev) {
        // the record routes write ta_edit records: sub-batches through a bounded ta_edit scratch (<= 256 MiB, whole wavefronts), packed as they come
        // (the ta_edit form cuts a long script at its FRONT `cap` runs, the packed form keeps the LAST ones: the scratch takes whole scripts -- a
        // script has at most n + m runs, and one of cost <= k at most 2 k + 1: every edit costs at least 1)
        const uint64_t cap_in = 2ull * k + 1 < 2 * max_len + 2 ? 2ull * k + 1 : 2 * max_len + 2;
        uint64_t chunk = (256ull << 20) / (cap_in * sizeof(ta_edit));
        chunk &= ~63ull;
        if (chunk < 64) chunk = 64;
        if (chunk > n) chunk = n;
        Scratch &es = tls_scratch(SLOT_SELECT);
        if ((rc = es.ensure((size_t)(chunk * cap_in * sizeof(ta_edit))))) return rc;
        for (uint64_t lo = 0; lo < n; lo += chunk) {
            const size_t cnt = (size_t)((n - lo) < chunk ? (n - lo) : chunk);
            const ta_strings sa = strings_slice(a, lo, max_len), sb = strings_slice(b, lo, max_len);
            if ((rc = trace_batch_impl(&sa, &sb, cnt, k, costs, out_dev + lo, (ta_edit *)es.dev, nullptr, n_edits_dev + lo, (size_t)cap_in, stream))) return rc;
            TA_HIP(pack_edits_launch((const ta_edit *)es.dev, n_edits_dev + lo, (uint32_t)cnt, cap_in, packed_dev + lo * cap, cap, st));
        }
        return TA_OK;
    }
    // the trace kernels exist for 16, 34 and 66 diagonals per lane: the cheapest layout per pair that holds the band
    LevPlan pl = {};
    pl.ok = false;
    double best = 1e300;
    for (int D : {34, 16, 66}) {
        const LevPlan c = lev_make_plan(k, costs->mismatch_cost, gc, sg, max_len, D, 0);
        const double cost = c.ok ? (5.0 * c.D + 24.0) / c.PW * (c.D > 40 ? 1.25 : 1.0) : 1e300;
        if (c.ok && cost < best) { best = cost; pl = c; }
    }
    if (!pl.ok) { set_last_error_msg("batch traceback: band wider than the register kernel (4222 diagonals)"); return TA_ERR_UNSUPPORTED; }
    const uint32_t tw = (uint32_t)lev_trace_words(pl.D);
    const uint64_t taus = (2 * max_len + 1) / 2 + 1;
    const uint64_t wave_words = taus * 2 * 64 * tw;
    // the records of one chunk: at most ~4 GiB and at most a quarter of the device memory that is free right now (or one wavefront's, if
    // that is more)
    const uint64_t waves_all = (n + pl.PW - 1) / pl.PW;
    uint64_t waves_per_chunk = ((4ull << 30) / 4) / wave_words;
    if (waves_per_chunk == 0) waves_per_chunk = 1;
    if (waves_per_chunk > waves_all) waves_per_chunk = waves_all;
    if (wave_words * waves_per_chunk * 4 > tls_scratch(SLOT_LINES).cap) {      // the scratch has to grow: not beyond a quarter of what is free right now
        size_t free_b = 0, total_b = 0;                                // (asked only then: a captured call must not query the device)
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const uint64_t budget = ((uint64_t)free_b + tls_scratch(SLOT_LINES).cap) / 4;
            if (wave_words * waves_per_chunk * 4 > budget) waves_per_chunk = (budget / 4) / wave_words;
            if (waves_per_chunk == 0) waves_per_chunk = 1;
        }
    }
    if (wave_words * waves_per_chunk * 4 > (48ull << 30)) { set_last_error_msg("batch traceback: more than 48 GB of records for one wavefront"); return TA_ERR_UNSUPPORTED; }
    Scratch &ts = tls_scratch(SLOT_LINES), &ps = tls_scratch(SLOT_TRACE);
    const uint32_t path_words = (uint32_t)((2 * max_len) / 16 + 2);                  // 2-bit codes of a pair's path, sixteen per word
    if ((rc = ts.ensure((size_t)(wave_words * waves_per_chunk * 4))) || (rc = ps.ensure((size_t)(waves_per_chunk * pl.PW) * path_words * 4))) return rc;
    LevParams P;
    P.a = view_of(a); P.b = view_of(b);
    P.subset = nullptr; P.out = out_dev; P.k = k;
    P.mc = costs->mismatch_cost; P.gc = gc; P.sg = sg; P.tc = costs->has_transpose ? costs->transpose_cost : 0;
    P.u = pl.u; P.o = pl.o; P.L = pl.L; P.PW = pl.PW; P.lds_per_wave = pl.lds_per_wave; P.Tw = pl.Tw; P.ch = pl.ch;
    P.trace = (uint32_t *)ts.dev; P.trace_wave_words = wave_words;
    const uint64_t pairs_per_chunk = waves_per_chunk * pl.PW;
    for (uint64_t lo = 0; lo < n; lo += pairs_per_chunk) {
        P.pair_base = (uint32_t)lo;
        P.n = (uint32_t)((n - lo) < pairs_per_chunk ? (n - lo) : pairs_per_chunk);
        TA_HIP(lev_band_trace_batch_launch(P, pl, sg > 0, costs->has_transpose != 0, edits_dev, n_edits_dev, cap, (uint32_t *)ps.dev, path_words, st));
    }
    ta_launch_info li = {};
    li.kernel = 1; li.diags_per_lane = pl.D; li.lanes_per_pair = pl.L; li.pairs_per_wave = pl.PW; li.band_offset = pl.o;
    li.affine = sg > 0; li.transpose = costs->has_transpose != 0; li.grid = (uint32_t)waves_per_chunk; li.lds_bytes = pl.lds_per_wave;
    li.cell_bits = launch_cell_bits(max_len, k, costs);
    last_launch() = li;
    set_last_kernel_name("lev_band_trace_kernel<%d, %s, %d>", pl.D, sg > 0 ? "true" : "false", costs->has_transpose ? 2 : 0);
    return TA_OK;
}

extern "C" {

/* levenshtein_simd_k_with_opts(..., trace_on = true): distance + run-length edit script.
 * The band-wavefront kernel stores a 2-bit argmin code per cell (tie order of src/levenshtein.rs:493-532);
 * the walk from (n, m) back to (0, 0) is the host part (:561-606). */
int ta_levenshtein_trace(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t k,
                         const ta_edit_costs *costs, uint32_t *out, ta_edit **edits, size_t *n_edits) {
    if (!out || !edits || !n_edits) return TA_ERR_ARG;
    *edits = nullptr; *n_edits = 0;
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (!device_ready()) return TA_ERR_HIP;
    if (a_len == 0 && b_len == 0) { *out = 0; return TA_OK; }                   // :721-727 (Some(vec![]))
    const bool swap = a_len > b_len;                                            // :386-390
    const uint8_t *x = swap ? b : a, *y = swap ? a : b;
    const size_t n = swap ? b_len : a_len, m = swap ? a_len : b_len;
    // every route below keeps its records in thread-local scratch that the batch entries share (SLOT_LINES, SLOT_TRACE) and runs on the
    // thread's own stream: ordered after the thread's earlier calls on other streams like any batch call (StreamGuard, ta_internal.h)
    CallCtx &cx = call_ctx();
    int rc = cx.ensure();
    if (rc) return rc;
    StreamGuard guard(cx.st);
    ta_lev_select sel;
    ta_levenshtein_select(n, m, k, costs, &sel);
    const uint32_t gc = costs->gap_cost, sg = costs->start_gap_cost;
    LevPlan pl = lev_make_plan(sel.max_k, costs->mismatch_cost, gc, sg, m, 16, 0);
    if (!pl.ok) pl = lev_make_plan(sel.max_k, costs->mismatch_cost, gc, sg, m, 66, 0);
    if (!pl.ok) {
        // band too wide for the register kernel: the unit-cost families take the row-blocked bit-parallel kernel with records
        const bool unit = costs_unit(costs);
        const uint64_t stripes = (n + 4095) / 4096, tcols = (uint64_t)m + 64;
        const uint64_t rec_words = stripes * tcols * 64ull * 6ull;
        const uint64_t code_words = ((n + 2047) / 2048) * tcols * 64ull * 2ull;           // DP wide kernel: 2 bits per cell
        if (m > 0xFFFFFF00ull || (unit ? rec_words : code_words) * 4ull > (8ull << 30)) {
            set_last_error_msg("traceback: more than 8 GB of traceback records");
            return TA_ERR_UNSUPPORTED;
        }
        if (unit) return trace_widebits(x, n, y, m, swap, k, costs, out, edits, n_edits, rec_words, tcols);
        return trace_wide(x, n, y, m, swap, k, costs, out, edits, n_edits, code_words, tcols);
    }
    Staged S;
    if ((rc = stage_pair(x, n, y, m, &S))) return rc;
    const uint32_t tw = (uint32_t)lev_trace_words(pl.D);
    const size_t taus = (n + m + 1) / 2 + 1;
    const size_t trace_words = taus * 2 * 64 * tw;
    Scratch &ts = tls_scratch(SLOT_LINES);
    if ((rc = ts.ensure(trace_words * 4))) return rc;
    LevParams P;
    P.a = view_of(&S.sa); P.b = view_of(&S.sb);
    P.subset = nullptr; P.out = S.out_dev; P.n = 1; P.k = k;
    P.mc = costs->mismatch_cost; P.gc = gc; P.sg = sg; P.tc = costs->has_transpose ? costs->transpose_cost : 0;
    P.u = pl.u; P.o = pl.o; P.L = pl.L; P.PW = pl.PW; P.lds_per_wave = pl.lds_per_wave; P.Tw = pl.Tw; P.ch = pl.ch;
    P.trace = (uint32_t *)ts.dev;
    TA_HIP(lev_band_trace_launch(P, pl, sg > 0, costs->has_transpose != 0, S.st));
    std::vector<uint32_t> tr;
    if ((rc = fetch_records(S, out, ts, trace_words, &tr)) || *out == TA_NONE) return rc;
    const uint32_t o_pair = lev_pair_offset(pl.u, n, m);
    ScriptBuilder<uint8_t> walk(x, n, y, m, swap);
    while (walk.i() > 0 || walk.j() > 0) walk.step(band_trace_code(tr.data(), (uint32_t)pl.D, tw, o_pair, walk.i(), walk.j()));   // :561-603
    walk.finish();
    return walk.release(edits, n_edits);
}

/* levenshtein_simd_k_with_opts(a_i, b_i, k, trace_on = true, costs) for a whole batch, everything on the device: out_dev[i] = the distance or
 * TA_NONE, n_edits_dev[i] = the runs of pair i's script (0 for None), edits_dev[i * cap ..] = the script, front to back, as ta_edit records --
 * edit for edit what the reference returns (its tie order, its swap of the shorter string onto the rows, its gap relabelling).  Nothing
 * comes back to the host and nothing synchronises: the DP band kernel stores 2-bit argmin codes (the records: scratch, bounded by
 * working through the batch in chunks), a second kernel walks them, one lane per pair.  A script of more than `cap` runs is cut
 * (n_edits_dev[i] > cap says so); 2 k + 1 runs always hold a script of cost <= k.  Bands beyond the register kernel (more than 4222
 * diagonals) are TA_ERR_UNSUPPORTED here -- ta_levenshtein_trace serves those pairs one by one. */
int ta_levenshtein_trace_batch(const ta_strings *a, const ta_strings *b, size_t n, uint32_t k, const ta_edit_costs *costs,
                               uint32_t *out_dev, ta_edit *edits_dev, uint32_t *n_edits_dev, size_t cap, void *stream) {
    if (n && !edits_dev) { set_last_error_msg("bad batch arguments"); return TA_ERR_ARG; }
    return trace_batch_impl(a, b, n, k, costs, out_dev, edits_dev, nullptr, n_edits_dev, cap, stream);
}
/* The same with PACKED records: one word per run, (edit << 29) | count, pair i's script the min(n_edits_dev[i], cap) words that END at
 * packed_dev[(i + 1) * cap] -- front to back, right-aligned in the pair's slot of `cap` words (a script of more runs keeps its LAST cap runs;
 * words in front of the script are not written).  A quarter of the 16-byte records' bytes; on the checkpoint route (LEVENSHTEIN_COSTS /
 * RDAMERAU_COSTS and their multiples, k / g <= 32 (30)) the walk writes every run where it belongs: no run lists in scratch, no reversal step.
 * Strings of 2^29 bytes and more: TA_ERR_UNSUPPORTED (a run's count has 29 bits). */
int ta_levenshtein_trace_batch_packed(const ta_strings *a, const ta_strings *b, size_t n, uint32_t k, const ta_edit_costs *costs,
                                      uint32_t *out_dev, uint32_t *packed_dev, uint32_t *n_edits_dev, size_t cap, void *stream) {
    if (n && !packed_dev) { set_last_error_msg("bad batch arguments"); return TA_ERR_ARG; }
    return trace_batch_impl(a, b, n, k, costs, out_dev, nullptr, packed_dev, n_edits_dev, cap, stream);
}

/* levenshtein_exp_with_opts(..., trace_on = true), src/levenshtein.rs:1480-1494 */
int ta_levenshtein_exp_trace(const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len,
                             const ta_edit_costs *costs, uint32_t *out, ta_edit **edits, size_t *n_edits) {
    uint32_t k = 30;
    for (int round = 0; round < 40; round++) {
        int rc = ta_levenshtein_trace(a, a_len, b, b_len, k, costs, out, edits, n_edits);
        if (rc != TA_OK || *out != TA_NONE) return rc;
        k = (k > 0x7FFFFFFFu) ? 0xFFFFFFFFu : k * 2;
    }
    return TA_OK;
}

}  // extern "C"
