// ta_tokens.hip -- the token-sequence entry points (include/triple_accel_amd.h, "token batches").
//
// A batch of u32 sequences is compacted pair by pair into byte codes (sym_compact_body.h) that keep the cross-sequence equality
// relation, the byte entry point runs on the codes, and the pairs the compaction could not code (overflow list, its length on the
// device) are answered by the DP wide kernel over 32-bit items (lev_wide.hip), on the same stream after the byte pass.
// The cost check, the batch argument check and the scratch slots' names (SLOT_TOK_*) are the shared ones of ta_internal.h.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <optional>
#include <unordered_map>
#include <vector>

#include "lev_script.h"
#include "sym_compact_body.h"
#include "ta_internal.h"

namespace ta {

static StrView tok_view(const ta_tokens *t) { return StrView{(const uint8_t *)t->data, t->off, t->stride, t->len}; }

static int tok_check(const ta_tokens *a, const ta_tokens *b, size_t n, const void *out) {
    return check_batch_args(a, b, a ? a->data : nullptr, b ? b->data : nullptr, n, out, "null data");
}

// longest sequence of a side (given, implied or measured: one synchronisation) and the items `data` holds (CSR: off[n])
static int tok_side(const ta_tokens *t, uint32_t n, hipStream_t st, uint64_t *max_len, uint64_t *items) {
    if (!t->off) { *max_len = t->len; *items = (uint64_t)n * t->len; return TA_OK; }
    *max_len = t->max_len;
    *items = t->len;
    if (t->max_len && t->len) return TA_OK;
    Scratch &sc = tls_scratch(SLOT_TOK_OVF);
    int rc = sc.ensure(64);
    if (rc) return rc;
    uint32_t *d = (uint32_t *)sc.dev;
    if (!t->max_len) {
        TA_HIP(hipMemsetAsync(d, 0, 4, st));
        TA_HIP(strings_maxlen_launch(tok_view(t), n, d, st));
    }
    uint32_t v = 0;
    uint64_t last = 0;
    if (!t->max_len) TA_HIP(hipMemcpyAsync(&v, d, 4, hipMemcpyDeviceToHost, st));
    if (!t->len) TA_HIP(hipMemcpyAsync(&last, t->off + n, 8, hipMemcpyDeviceToHost, st));
    TA_HIP(hipStreamSynchronize(st));
    if (!t->max_len) *max_len = v;
    if (!t->len) *items = last;
    return TA_OK;
}

struct Compacted {
    ta_strings a, b;              // the byte codes as a byte batch
    uint64_t max_len;             // of both sides
    bool may_overflow;            // some pair's shorter side can exceed 255 items
    uint32_t *ovf_list, *ovf_count;
};

// the compaction pass: codes into thread scratch, the overflow counter zeroed on the device (graph-safe) first
static int tok_compact(const ta_tokens *a, const ta_tokens *b, uint32_t n, hipStream_t st, Compacted *C) {
    uint64_t ma = 0, mb = 0, ia = 0, ib = 0;
    int rc;
    if ((rc = tok_side(a, n, st, &ma, &ia)) || (rc = tok_side(b, n, st, &mb, &ib))) return rc;
    const uint64_t short_max = ma < mb ? ma : mb;
    C->max_len = ma > mb ? ma : mb;
    C->may_overflow = short_max > SYM_SHORT_MAX;
    uint32_t waves = n;
    uint32_t table_cap = 0;
    if (C->may_overflow) {
        table_cap = 64;
        while ((uint64_t)table_cap < 2 * short_max) table_cap <<= 1;
        // one table per wavefront: at most 256 MiB of tables, at least one wavefront
        const uint64_t fit = (256ull << 20) / ((uint64_t)table_cap * 12u);
        if ((uint64_t)waves > fit) waves = fit ? (uint32_t)fit : 1u;
        waves &= ~3u;
        if (!waves) waves = 4;
    }
    Scratch &sa = tls_scratch(SLOT_TOK_CA), &sb = tls_scratch(SLOT_TOK_CB), &tb = tls_scratch(SLOT_TOK_TABLE), &ov = tls_scratch(SLOT_TOK_OVF);
    if ((rc = sa.ensure(ia + TA_BLOB_SLACK)) || (rc = sb.ensure(ib + TA_BLOB_SLACK)) || (rc = ov.ensure(64 + (size_t)n * 4))) return rc;
    if (table_cap && (rc = tb.ensure((size_t)((waves + 3u) & ~3u) * table_cap * 12u))) return rc;
    SymCompactParams P;
    P.a_data = a->data; P.b_data = b->data; P.a_off = a->off; P.b_off = b->off;
    P.a_stride = a->stride; P.a_len = a->len; P.b_stride = b->stride; P.b_len = b->len;
    P.ca = (uint8_t *)sa.dev; P.cb = (uint8_t *)sb.dev; P.n = n;
    P.table = table_cap ? (uint64_t *)tb.dev : nullptr;
    P.flags = table_cap ? (uint32_t *)((uint64_t *)tb.dev + (size_t)((waves + 3u) & ~3u) * table_cap) : nullptr;
    P.table_cap = table_cap;
    C->ovf_count = (uint32_t *)ov.dev;
    C->ovf_list = (uint32_t *)ov.dev + 16;
    P.ovf_list = C->ovf_list; P.ovf_count = C->ovf_count;
    TA_HIP(fill_u32_launch(C->ovf_count, 0u, 1, st));
    TA_HIP(sym_compact_launch(P, waves, st));
    C->a = ta_strings{P.ca, a->off, a->off ? 0 : a->len, a->off ? 0 : a->len, ma};
    C->b = ta_strings{P.cb, b->off, b->off ? 0 : b->len, b->off ? 0 : b->len, mb};
    return TA_OK;
}

static LevParams wide_params(const StrView &a, const StrView &b, uint32_t k, const ta_edit_costs *c, uint64_t max_len, uint32_t *out) {
    LevParams P;
    P.a = a; P.b = b;
    P.subset = nullptr; P.trace = nullptr; P.out = out; P.n = 1; P.k = k;
    P.mc = c->mismatch_cost; P.gc = c->gap_cost; P.sg = c->start_gap_cost; P.tc = c->has_transpose ? c->transpose_cost : 0;
    P.u = lev_batch_unit_k(k, P.mc, P.gc, P.sg, max_len);
    P.o = 0; P.L = 0; P.PW = 1; P.Tw = 0; P.ch = 0;
    P.lds_per_wave = (uint32_t)(max_len + 2);                                  // boundary line length
    return P;
}

// the overflow pairs of a k / exp batch: the u32 wide kernel over the list (its length read on the device), after the byte pass
static int tok_overflow_pass(const ta_tokens *a, const ta_tokens *b, size_t n, uint32_t k, const ta_edit_costs *costs, const Compacted &C,
                             uint32_t *out_dev, hipStream_t st) {
    if (!C.may_overflow) return TA_OK;
    LevParams P = wide_params(tok_view(a), tok_view(b), k, costs, C.max_len, out_dev);
    P.subset = C.ovf_list; P.n_dev = C.ovf_count;
    P.n = n < 1024 ? (uint32_t)n : 1024u;                                      // (the grid; the kernel strides over the list)
    char name[96];
    snprintf(name, sizeof(name), "%s", ta_last_kernel_name());
    TA_HIP(lev_wide_u32_launch(P, costs->has_transpose != 0, false, st));
    set_last_kernel_name("%s", name);                                          // the pass's dominant kernel stays the byte pass's
    return TA_OK;
}

// One pair of u32 items on the device through the wide kernel: distance, and with `res` the finished script in (*res)->runs (x = the shorter
// side on the rows, as src/levenshtein.rs:386-390; `*res` is set unless the answer is None).  Host inputs; synchronises.
static int wide_pair_u32(const uint32_t *a, size_t la, const uint32_t *b, size_t lb, uint32_t k, const ta_edit_costs *costs, hipStream_t st,
                         uint32_t *out, std::optional<ScriptBuilder<uint32_t>> *res) {
    const bool swap = res && la > lb;
    const uint32_t *x = swap ? b : a, *y = swap ? a : b;
    const size_t n = swap ? lb : la, m = swap ? la : lb;
    if (n > 0xFFFFFFF0ull || m > 0xFFFFFF00ull) { set_last_error_msg("token sequence too long"); return TA_ERR_ARG; }
    const uint64_t tcols = (uint64_t)m + 64, code_words = res ? ((n + 2047) / 2048) * tcols * 64ull * 2ull : 0;
    if (code_words * 4ull > (8ull << 30)) { set_last_error_msg("traceback: more than 8 GB of traceback records"); return TA_ERR_UNSUPPORTED; }
    Scratch &stg = tls_scratch(SLOT_TOK_STAGE), &ts = tls_scratch(SLOT_TRACE);
    int rc;
    if ((rc = stg.ensure((n + m + 4) * 4))) return rc;
    if (res && (rc = ts.ensure((size_t)code_words * 4 + 4))) return rc;
    uint32_t *dx = (uint32_t *)stg.dev, *dy = dx + n, *dout = dy + m;
    if (n) TA_HIP(hipMemcpyAsync(dx, x, n * 4, hipMemcpyHostToDevice, st));
    if (m) TA_HIP(hipMemcpyAsync(dy, y, m * 4, hipMemcpyHostToDevice, st));
    const StrView vx{(const uint8_t *)dx, nullptr, n, n}, vy{(const uint8_t *)dy, nullptr, m, m};
    LevParams P = wide_params(vx, vy, k, costs, n > m ? n : m, dout);
    if (res) { P.u = lev_batch_unit_k(k, P.mc, P.gc, P.sg, m); P.lds_per_wave = (uint32_t)(m + 2); P.trace = (uint32_t *)ts.dev; P.trace_cols = tcols; }
    TA_HIP(lev_wide_u32_launch(P, costs->has_transpose != 0, res != nullptr, st));
    uint32_t d = 0;
    TA_HIP(hipMemcpyAsync(&d, dout, 4, hipMemcpyDeviceToHost, st));
    TA_HIP(hipStreamSynchronize(st));
    *out = d;
    if (!res || d == TA_NONE) return TA_OK;
    std::vector<uint32_t> tr((size_t)code_words);
    TA_HIP(hipMemcpyAsync(tr.data(), ts.dev, (size_t)code_words * 4, hipMemcpyDeviceToHost, st));
    TA_HIP(hipStreamSynchronize(st));
    ScriptBuilder<uint32_t> &walk = res->emplace(x, n, y, m, swap);
    while (walk.i() > 0 || walk.j() > 0) walk.step(wide_trace_code(tr.data(), tcols, walk.i(), walk.j()));   // :561-603
    walk.finish();
    return TA_OK;
}

// the host form of the coding (one pair): false when the pair overflows
static bool host_codes(const uint32_t *a, size_t la, const uint32_t *b, size_t lb, std::vector<uint8_t> &ca, std::vector<uint8_t> &cb) {
    ca.assign(la, 0); cb.assign(lb, 0);
    const bool s_is_a = la <= lb;
    const uint32_t *s = s_is_a ? a : b, *t = s_is_a ? b : a;
    const size_t ls = s_is_a ? la : lb, lt = s_is_a ? lb : la;
    std::vector<uint8_t> &cs = s_is_a ? ca : cb, &ct = s_is_a ? cb : ca;
    if (ls <= SYM_SHORT_MAX) {
        std::unordered_map<uint32_t, uint32_t> first;
        for (size_t i = 0; i < ls; i++) first.emplace(s[i], (uint32_t)i);
        for (size_t i = 0; i < ls; i++) cs[i] = (uint8_t)first[s[i]];
        for (size_t j = 0; j < lt; j++) { auto f = first.find(t[j]); ct[j] = f == first.end() ? 255 : (uint8_t)f->second; }
        return true;
    }
    std::unordered_map<uint32_t, uint32_t> code;                               // items of s -> 0 (one side) / code + 1 (common)
    for (size_t i = 0; i < ls; i++) code.emplace(s[i], 0u);
    uint32_t common = 0;
    for (size_t j = 0; j < lt; j++) {
        auto f = code.find(t[j]);
        if (f != code.end() && f->second == 0) f->second = ++common;
    }
    if (common > 254) return false;
    const uint8_t only_s = s_is_a ? 254 : 255, only_t = s_is_a ? 255 : 254;
    for (size_t i = 0; i < ls; i++) { const uint32_t c = code[s[i]]; cs[i] = c ? (uint8_t)(c - 1) : only_s; }
    for (size_t j = 0; j < lt; j++) { auto f = code.find(t[j]); ct[j] = (f != code.end() && f->second) ? (uint8_t)(f->second - 1) : only_t; }
    return true;
}

}  // namespace ta

using namespace ta;

extern "C" {

int ta_levenshtein_k_batch_tokens(const ta_tokens *a, const ta_tokens *b, size_t n, uint32_t k,
                                  const ta_edit_costs *costs, uint32_t *out_dev, void *stream) {
    int rc = tok_check(a, b, n, out_dev);
    if (rc) return rc;
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (!device_ready()) return TA_ERR_HIP;
    if (n == 0) return TA_OK;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    Compacted C;
    if ((rc = tok_compact(a, b, (uint32_t)n, st, &C))) return rc;
    if ((rc = ta_levenshtein_k_batch(&C.a, &C.b, n, k, costs, out_dev, stream))) return rc;
    return tok_overflow_pass(a, b, n, k, costs, C, out_dev, st);
}

int ta_levenshtein_exp_batch_tokens(const ta_tokens *a, const ta_tokens *b, size_t n,
                                    const ta_edit_costs *costs, uint32_t *out_dev, void *stream) {
    int rc = tok_check(a, b, n, out_dev);
    if (rc) return rc;
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (!device_ready()) return TA_ERR_HIP;
    if (n == 0) return TA_OK;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    Compacted C;
    if ((rc = tok_compact(a, b, (uint32_t)n, st, &C))) return rc;
    if ((rc = ta_levenshtein_exp_batch(&C.a, &C.b, n, costs, out_dev, stream))) return rc;
    return tok_overflow_pass(a, b, n, 0xFFFFFFFFu, costs, C, out_dev, st);
}

int ta_levenshtein_trace_batch_tokens(const ta_tokens *a, const ta_tokens *b, size_t n, uint32_t k, const ta_edit_costs *costs,
                                      uint32_t *out_dev, ta_edit *edits_dev, uint32_t *n_edits_dev, size_t cap, void *stream) {
    int rc = tok_check(a, b, n, out_dev);
    if (rc) return rc;
    if (n && (!edits_dev || !n_edits_dev)) { set_last_error_msg("bad batch arguments"); return TA_ERR_ARG; }
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (!device_ready()) return TA_ERR_HIP;
    if (n == 0) return TA_OK;
    hipStream_t st = (hipStream_t)stream;
    StreamGuard guard(st);
    Compacted C;
    if ((rc = tok_compact(a, b, (uint32_t)n, st, &C))) return rc;
    if ((rc = ta_levenshtein_trace_batch(&C.a, &C.b, n, k, costs, out_dev, edits_dev, n_edits_dev, cap, stream))) return rc;
    if (!C.may_overflow) return TA_OK;
    // the overflow pairs: one synchronisation for the count, then pair by pair through the wide TRACE kernel and the host walk
    uint32_t cnt = 0;
    TA_HIP(hipMemcpyAsync(&cnt, C.ovf_count, 4, hipMemcpyDeviceToHost, st));
    TA_HIP(hipStreamSynchronize(st));
    if (!cnt) return TA_OK;
    std::vector<uint32_t> list(cnt);
    TA_HIP(hipMemcpyAsync(list.data(), C.ovf_list, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
    TA_HIP(hipStreamSynchronize(st));
    std::vector<uint32_t> xa, xb;
    std::optional<ScriptBuilder<uint32_t>> res;                              // (set by wide_pair_u32 unless the answer is None)
    for (uint32_t p : list) {
        const ta_tokens *sd[2] = {a, b};
        std::vector<uint32_t> *buf[2] = {&xa, &xb};
        for (int s = 0; s < 2; s++) {
            uint64_t o[2] = {0, 0};
            if (sd[s]->off) TA_HIP(hipMemcpyAsync(o, sd[s]->off + p, 16, hipMemcpyDeviceToHost, st));
            TA_HIP(hipStreamSynchronize(st));
            if (!sd[s]->off) { o[0] = (uint64_t)p * sd[s]->stride; o[1] = o[0] + sd[s]->len; }
            buf[s]->resize(o[1] - o[0]);
            if (o[1] > o[0]) TA_HIP(hipMemcpyAsync(buf[s]->data(), sd[s]->data + o[0], (o[1] - o[0]) * 4, hipMemcpyDeviceToHost, st));
        }
        TA_HIP(hipStreamSynchronize(st));
        uint32_t d = 0;
        if ((rc = wide_pair_u32(xa.data(), xa.size(), xb.data(), xb.size(), k, costs, st, &d, &res))) return rc;
        const uint32_t ne = d == TA_NONE ? 0u : (uint32_t)res->runs.size();
        TA_HIP(hipMemcpyAsync(out_dev + p, &d, 4, hipMemcpyHostToDevice, st));
        TA_HIP(hipMemcpyAsync(n_edits_dev + p, &ne, 4, hipMemcpyHostToDevice, st));
        const size_t keep = ne < cap ? ne : cap;
        if (keep) TA_HIP(hipMemcpyAsync(edits_dev + (size_t)p * cap, res->runs.data(), keep * sizeof(ta_edit), hipMemcpyHostToDevice, st));
        TA_HIP(hipStreamSynchronize(st));                                      // (the host buffers are reused)
    }
    return TA_OK;
}

int ta_levenshtein_tokens(const uint32_t *a, size_t a_len, const uint32_t *b, size_t b_len, uint32_t k,
                          const ta_edit_costs *costs, uint32_t *out, ta_edit **edits, size_t *n_edits) {
    if (!out || (!a && a_len) || (!b && b_len) || (edits && !n_edits)) return TA_ERR_ARG;
    if (edits) { *edits = nullptr; *n_edits = 0; }
    if (!costs_ok(costs)) return TA_ERR_BAD_COSTS;
    if (!device_ready()) return TA_ERR_HIP;
    std::vector<uint8_t> ca, cb;
    if (host_codes(a, a_len, b, b_len, ca, cb)) {
        if (edits) return ta_levenshtein_trace(ca.data(), a_len, cb.data(), b_len, k, costs, out, edits, n_edits);
        return ta_levenshtein_simd_k_with_opts(ca.data(), a_len, cb.data(), b_len, k, 0, costs, out);
    }
    int rc = call_ctx().ensure();
    if (rc) return rc;
    hipStream_t st = call_ctx().st;
    StreamGuard guard(st);                                                      // (SLOT_TRACE and SLOT_LINES are the batch entries' too)
    if (!edits) return wide_pair_u32(a, a_len, b, b_len, k, costs, st, out, nullptr);
    std::optional<ScriptBuilder<uint32_t>> res;
    if ((rc = wide_pair_u32(a, a_len, b, b_len, k, costs, st, out, &res))) return rc;
    return *out == TA_NONE ? TA_OK : res->release(edits, n_edits);
}

}  // extern "C"
