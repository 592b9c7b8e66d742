"""The gate, the cases and the runner of tests/test_gpu_stream_order.py (TEST INFRASTRUCTURE ONLY; not a conftest, no pytest hook).

A case is a function `case(seed)` -> Case(run, check, route): `run()` makes ONE library call on the current torch stream (batch entries)
or on the library's own per-thread stream (single-call functions) and returns what the call returned; `check(result)` compares it with
the oracle after everything has been synchronised; `route()` (optional) asserts, right after a call, that the call took the route the
case is named after (last_launch_info / last_kernel_name).  Host inputs and expected values are built once per (case, seed).

The gate (Gate.arm) is torch.cuda._sleep on stream s1, about 50 ms of it: whatever is enqueued on s1 afterwards is pending until the
sleep ends, and `s1.query()` says whether it still is.  Nothing here lets two library calls run at the same time on purpose: a call
that the library ordered after the gated one starts when that one has finished, and a call that it did not order finishes while s1
is still asleep -- before the gated call has started.
"""
import functools
import os

import numpy as np

import datagen as Dg
import oracle_lib as O

NONE = 0xFFFFFFFF
UNIT = (1, 1, 0, None)
WEIGHTED = (2, 3, 1, None)
GAPPY = (3, 1, 1, None)           # a mismatch dearer than two gaps: the single-call band spans 2 x the shorter string (ta_levenshtein_select)
GATE_MS = 50.0
GATE_MAX_MS = 500.0


class Case:
    def __init__(self, run, check, route=None, close=None, prep=None, control=None):
        self.run, self.check, self.route, self.close, self.prep, self.control = run, check, route, close, prep, control


# ---------------------------------------------------------------------------------------------------------------- the gate
class Gate:
    """s1: the gated stream; s2: the stream of the asynchronous B's.  Both are taken from at most 8 fresh torch streams: the first that
    the library's own stream (s1) and s1 (s2) do NOT queue up behind -- with few hardware queues two streams can share one, and a
    stream stuck behind the sleep would make every ordering assertion true for nothing."""

    def __init__(self):
        import torch
        import triple_accel_amd as T
        assert hasattr(torch.cuda, "_sleep"), "torch.cuda._sleep is gone: the gate needs another device-side delay"
        self.torch, self.T = torch, T
        torch.cuda.synchronize()
        assert T.hamming(b"abc", b"abd") == 1                       # the library's stream and pinned buffer exist from here on
        self.cycles = self._calibrate()
        self.tick = torch.zeros(64, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in range(8)]
        self.s1 = self.s2 = None
        seen = []
        for s in streams:
            if self.s1 is None:
                ok = self.control_sync(s)
                seen.append(("s1", ok))
                if ok:
                    self.s1 = s
                continue
            ok = self.control_async(s)
            seen.append(("s2", ok))
            if ok:
                self.s2 = s
                break
        assert self.s1 is not None and self.s2 is not None, \
            "none of 8 fresh torch streams passed the control (the other stream must overtake the gate): %r" % (seen,)
        self.ev = torch.cuda.Event()

    def _calibrate(self):
        torch = self.torch
        s = torch.cuda.Stream()
        probe = 2_000_000
        best = None
        for _ in range(3):                                          # (the first launch of the sleep kernel pays for its load)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(s):
                e0.record(s)
                torch.cuda._sleep(probe)
                e1.record(s)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None else min(best, ms)
        assert best > 0.02, "the sleep kernel cannot be calibrated: %d cycles took %.4f ms" % (probe, best)
        cycles = int(probe * GATE_MS / best)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            torch.cuda._sleep(cycles)
            e1.record(s)
        e1.synchronize()
        self.gate_ms = e0.elapsed_time(e1)
        assert self.gate_ms <= GATE_MAX_MS, "calibration refused: the gate would last %.1f ms (cap %.0f ms)" % (self.gate_ms, GATE_MAX_MS)
        assert self.gate_ms >= GATE_MS / 4, "calibration refused: the gate lasts only %.2f ms" % self.gate_ms
        return cycles

    def arm(self, s=None):
        s = self.s1 if s is None else s
        with self.torch.cuda.stream(s):
            self.torch.cuda._sleep(self.cycles)

    def control_sync(self, s):
        """the gate alone on `s`, then a guarded single call whose pending event (if any) is complete: s must still be asleep"""
        self.torch.cuda.synchronize()
        self.arm(s)
        assert self.T.hamming(b"abc", b"abd") == 1
        ok = not s.query()
        s.synchronize()
        return ok

    def control_async(self, s):
        """the gate alone on s1, then a trivial torch op on `s` and an event of `s` synchronised: s1 must still be asleep"""
        torch = self.torch
        torch.cuda.synchronize()
        self.arm(self.s1)
        ev = torch.cuda.Event()
        with torch.cuda.stream(s):
            self.tick.add_(1)
            ev.record(s)
        ev.synchronize()
        ok = not self.s1.query()
        self.s1.synchronize()
        return ok


def _poison(res):
    """overwrite every device tensor of a warm-up result (the armed call is handed the same blocks by the caching allocator)"""
    import torch
    if isinstance(res, torch.Tensor):
        if res.is_cuda:
            res.fill_(-7)
    elif isinstance(res, (tuple, list)):
        for r in res:
            _poison(r)


def run_gated(gate, a, b, b_async):
    """A on s1 behind the gate, then B (on s2, or a single call on the library's stream).  Asserts the premise (A is still pending when B
    is made), both answers, and the ordering: once B is complete, s1 has nothing pending."""
    torch = gate.torch
    s1, s2 = gate.s1, gate.s2

    def call_a():
        with torch.cuda.stream(s1):
            return a.run()

    def call_b():
        if not b_async:
            return b.run()
        with torch.cuda.stream(s2):
            return b.run()

    def call_prep():
        for c in (a, b):
            if c.prep:
                c.prep()

    for c in (a, b):
        if c.control:                                              # a case that brings a stream of its own shows that it overtakes the gate
            c.control(gate)
    try:
        # warm: every call once with the same shapes, synchronised -- scratch growth (hipFree / hipMalloc) would order the calls by accident
        torch.cuda.synchronize()
        call_prep()
        ra = call_a()
        if a.route:
            a.route()
        rb = call_b()
        if b.route:
            b.route()
        torch.cuda.synchronize()
        a.check(ra)
        b.check(rb)
        with torch.cuda.stream(s1):
            _poison(ra)
        with torch.cuda.stream(s2):
            _poison(rb)
        del ra, rb
        torch.cuda.synchronize()
        # armed
        call_prep()
        gate.arm()
        ra = call_a()
        premise = not s1.query()                                   # right after A, right before B
        rb = call_b() if premise else None
        if premise and b_async:
            gate.ev.record(s2)
            gate.ev.synchronize()
        ordered = s1.query()                                       # B is complete: is anything of s1 still pending?
    finally:
        torch.cuda.synchronize()
    assert premise, "premise: A left nothing pending on s1 (it synchronised, or the gate of %.1f ms ran out): choose an asynchronous A" % gate.gate_ms
    a.check(ra)
    b.check(rb)
    assert ordered, "B completed while the gated A was still pending on the other stream: B did not wait for A's scratch"
    for c in (a, b):
        if c.close:
            c.close()


# ---------------------------------------------------------------------------------------------------------------- shared helpers
def _mods():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    return torch, T, B


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _ragged(seed, n, lo, hi, edits, alphabet=None):
    g = Dg.rng(seed)
    a, b = [], []
    for _ in range(n):
        s = Dg.rand_str(g, int(g.integers(lo, hi + 1)))
        a.append(s)
        b.append(Dg.mutate(g, s, edits))
    return a, b


def _long_pair(seed, length, edits):
    g = Dg.rng(seed)
    s = Dg.rand_str(g, length)
    return s, Dg.mutate(g, s, edits)


def _kernel_is(k):
    def route():
        import triple_accel_amd as T
        info = T.last_launch_info()
        assert info["kernel"] == k, (k, info, T.last_kernel_name())
    return route


def _name_has(part):
    def route():
        import triple_accel_amd as T
        assert part in T.last_kernel_name(), (part, T.last_kernel_name())
    return route


def _norm(edits):
    return None if edits is None else [(str(e[0]), int(e[1])) for e in edits]


def _k_case(a, b, k, costs, route, fixed=False, want=None, option=None):
    """levenshtein_k_batch over lists of byte strings (CSR with max_len) or two (n, len) arrays (fixed)"""
    torch, T, B = _mods()
    if fixed:
        sa, sb = B.Strings.from_fixed(a), B.Strings.from_fixed(b)
    else:
        sa, sb = B.Strings.from_list(a), B.Strings.from_list(b)

    def run():
        if option is not None:
            T.set_option(option, True)
        try:
            return B.levenshtein_k_batch(sa, sb, k, costs)
        finally:
            if option is not None:
                T.set_option(option, False)

    return Case(run, lambda r: _same(_u32(r), want), route)


def _same(got, want):
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:8], got[:8], want[:8])


def _csr_want(a, b, k, costs):
    return O.levenshtein_k_batch(O.csr_from_list(a), O.csr_from_list(b), k, costs)


# ---------------------------------------------------------------------------------------------------------------- asynchronous cases
@functools.lru_cache(maxsize=None)
def _d_k_ragged(seed):
    a, b = _ragged(seed, 4096, 16, 48, 6)
    return a, b, _csr_want(a, b, 8, UNIT)


def k_ragged(seed):
    """4,096 CSR pairs, max_len given: the length order (SLOT_ORDER, SLOT_ORDER_BINS)"""
    a, b, want = _d_k_ragged(seed)
    return _k_case(a, b, 8, UNIT, _kernel_is(3), want=want)


@functools.lru_cache(maxsize=None)
def _d_k_small(seed):
    a, b = _ragged(seed, 200, 5, 40, 6)
    return a, b, _csr_want(a, b, 8, UNIT)


def k_small_ragged(seed):
    """a small ragged batch below the length order: no scratch (Part 1's fixed B)"""
    a, b, want = _d_k_small(seed)
    return _k_case(a, b, 8, UNIT, _kernel_is(3), want=want)


@functools.lru_cache(maxsize=None)
def _d_k_prefilter(seed):
    a, b = Dg.pairs_mutated_fixed(seed, 2048, 64, 8)
    b[::3] = Dg.pairs_random(seed + 1, len(b[::3]), 64)[1]
    return a, b, O.levenshtein_k_batch(O.csr_from_fixed(a), O.csr_from_fixed(b), 20, WEIGHTED)


def k_prefilter(seed):
    """weighted costs under OPT_UNIT_PREFILTER, 2,048 pairs (beyond the latency rule: the DP band kernel prices the survivors): the survivor list and its counter (SLOT_SUBSET_A, SLOT_COUNT)"""
    import triple_accel_amd as T
    a, b, want = _d_k_prefilter(seed)
    return _k_case(a, b, 20, WEIGHTED, _kernel_is(1), fixed=True, want=want, option=T.OPT_UNIT_PREFILTER)


@functools.lru_cache(maxsize=None)
def _d_k_widebits_lines(seed):
    a, b = _ragged(seed, 6, 3000, 4300, 40)
    a[0], b[0] = _long_pair(seed + 1, 4300, 40)                     # (max_len beyond one stripe of 4,096 rows: the boundary lines)
    return a, b, _csr_want(a, b, NONE, UNIT)


def k_widebits_lines(seed):
    """unit costs, unbounded k, CSR strings beyond one stripe: the row-blocked kernel's boundary lines (SLOT_LINES)"""
    a, b, want = _d_k_widebits_lines(seed)
    return _k_case(a, b, NONE, UNIT, _kernel_is(4), want=want)


@functools.lru_cache(maxsize=None)
def _d_k_widebits_tiles(seed):
    g = Dg.rng(seed)
    a = g.integers(33, 127, size=(2, 8400), dtype=np.uint8)
    b = a.copy()
    for r in range(2):
        pos = g.permutation(8400)[:60]
        b[r, pos] = 32
        b[r, 100:8000] = a[r, 103:8003]                             # a shift: gaps, not only substitutions
    return a, b, O.levenshtein_k_batch(O.csr_from_fixed(a), O.csr_from_fixed(b), NONE, UNIT)


def k_widebits_tiles(seed):
    """two fixed-length pairs beyond 8,192 bytes: the tiled row-blocked form (SLOT_LINES, SLOT_AUX_B)"""
    a, b, want = _d_k_widebits_tiles(seed)
    return _k_case(a, b, NONE, UNIT, _kernel_is(4), fixed=True, want=want)


@functools.lru_cache(maxsize=None)
def _d_k_wide(seed):
    a, b = _ragged(seed, 3, 4250, 4300, 30)
    return a, b, _csr_want(a, b, NONE, WEIGHTED)


def k_wide(seed):
    """weighted costs on strings beyond the register band: the DP wide kernel's boundary lines (lev_wide, SLOT_LINES)"""
    a, b, want = _d_k_wide(seed)
    return _k_case(a, b, NONE, WEIGHTED, _kernel_is(2), want=want)


@functools.lru_cache(maxsize=None)
def _d_k_fixed(seed):
    a, b = Dg.pairs_mutated_fixed(seed, 512, 48, 6)
    return a, b, O.levenshtein_k_batch(O.csr_from_fixed(a), O.csr_from_fixed(b), 8, UNIT)


def k_fixed(seed):
    """a fixed-length batch on the bit-parallel kernel: no scratch, records nothing by design (Part 2 only: it still has to wait)"""
    a, b, want = _d_k_fixed(seed)
    return _k_case(a, b, 8, UNIT, _kernel_is(3), fixed=True, want=want)


@functools.lru_cache(maxsize=None)
def _d_alphabet(seed):
    g = Dg.rng(seed)
    n = 16384
    a = g.choice(np.frombuffer(b"ACGT", np.uint8), size=(n, 32))
    b = a.copy()
    sub = g.random((n, 32)) < 0.06
    b[sub] = g.choice(np.frombuffer(b"ACGT", np.uint8), size=int(sub.sum()))
    b[7::1000, 5] = ord("N")                                        # a byte outside the alphabet: the general kernel answers these pairs
    a[11::2000, 31] = ord("N")
    return a, b, O.levenshtein_k_batch(O.csr_from_fixed(a), O.csr_from_fixed(b), 4, UNIT)


def k_alphabet(seed):
    """16,384 fixed-length ACGT pairs, a few with an N: the list of such pairs and its counters (SLOT_ALPHA_BAD, SLOT_ALPHA_COUNT)"""
    torch, T, B = _mods()
    a, b, want = _d_alphabet(seed)
    sa, sb = B.Strings.from_fixed(a), B.Strings.from_fixed(b)
    return Case(lambda: B.levenshtein_k_batch(sa, sb, 4, UNIT, alphabet=b"ACGT"), lambda r: _same(_u32(r), want), _kernel_is(7))


@functools.lru_cache(maxsize=None)
def _d_exp(seed):
    a, b = Dg.pairs_mutated_fixed(seed, 1024, 64, 24)
    b[::5] = Dg.pairs_random(seed + 1, len(b[::5]), 64)[1]          # (some pairs beyond the first threshold: more than one round has work)
    return a, b, O.levenshtein_exp_batch(O.csr_from_fixed(a), O.csr_from_fixed(b), UNIT)


def exp_batch(seed):
    """1,024 fixed-length pairs: the device-driven rounds (SLOT_SUBSET_A / _B, SLOT_COUNT, SLOT_EXP_BOUND, SLOT_EXP_WORK)"""
    torch, T, B = _mods()
    a, b, want = _d_exp(seed)
    sa, sb = B.Strings.from_fixed(a), B.Strings.from_fixed(b)
    return Case(lambda: B.levenshtein_exp_batch(sa, sb, UNIT), lambda r: _same(_u32(r), want))


@functools.lru_cache(maxsize=None)
def _d_trace(seed, costs, k):
    a, b = _ragged(seed, 96, 10, 60, 6)
    want = [O.levenshtein_simd_k_with_opts(x, y, k, True, costs) for x, y in zip(a, b)]
    return a, b, want


def _check_scripts(d, lists, want):
    for i, (wd, ws) in enumerate(want):
        if wd is None:
            assert d[i] == NONE, i
        else:
            assert d[i] == wd and _norm(lists[i]) == _norm(ws), (i, d[i], wd, lists[i], ws)


def _trace_case(seed, costs, k, packed, route):
    torch, T, B = _mods()
    a, b, want = _d_trace(seed, costs, k)
    sa, sb = B.Strings.from_list(a), B.Strings.from_list(b)
    fn = B.levenshtein_trace_batch_packed if packed else B.levenshtein_trace_batch
    to_lists = B.packed_to_lists if packed else B.edits_to_lists

    def check(r):
        out, edits, ne = r
        _check_scripts(_u32(out), to_lists(edits, ne), want)

    return Case(lambda: fn(sa, sb, k, costs), check, route)


def trace_ckpt(seed):
    """unit costs, k <= 32: checkpoints, run lists and run counts (SLOT_TRACE, SLOT_AUX_B, SLOT_AUX_A)"""
    return _trace_case(seed, UNIT, 8, False, _kernel_is(8))


def trace_records(seed):
    """weighted costs: the DP band kernel's records and the walked paths (SLOT_LINES, SLOT_TRACE)"""
    return _trace_case(seed, WEIGHTED, 20, False, _name_has("lev_band_trace_kernel"))


def trace_packed_ckpt(seed):
    return _trace_case(seed, UNIT, 8, True, _kernel_is(8))


def trace_packed_records(seed):
    """the packed form's record route: the ta_edit records of a sub-batch (SLOT_SELECT) around the inner record-route call"""
    return _trace_case(seed, WEIGHTED, 20, True, _name_has("lev_band_trace_kernel"))


# token sequences
def _tok_pairs(seed, n, overflow):
    g = np.random.default_rng(seed)
    a, b = [], []
    for i in range(n):
        x = g.integers(0, 50000, int(g.integers(1, 90))).tolist()
        y = list(x)
        for _ in range(int(g.integers(0, 6))):
            p = int(g.integers(0, len(y)))
            y[p] = int(g.integers(0, 50000))
        if i % 3 == 0:
            y = y[1:] + [7]
        a.append(x); b.append(y)
    for t in range(overflow):                                       # permutations of ~300 distinct tokens: more than 254 common items
        m = 290 + 7 * t
        x = (g.permutation(60000)[:m] + (0xFFFFFF00 if t % 2 else 0)).astype(np.int64) % (1 << 32)
        x = x.tolist()
        y = list(x)
        for _ in range(4):
            p, q = int(g.integers(0, m)), int(g.integers(0, m))
            y[p], y[q] = y[q], y[p]
        a.insert(5 * t + 2, x); b.insert(5 * t + 2, y)
    return a, b


def _tok_ref(x, y, k, trace, costs):
    import tokens_ref as R
    c = R.codes(x, y)
    if c is not None:
        d, tr = O.levenshtein_simd_k_with_opts(c[0], c[1], k, trace, costs)
        return None if d is None else (d, tr)
    return R.levenshtein(x, y, k, trace, costs)


@functools.lru_cache(maxsize=None)
def _d_tokens(seed, overflow, k, trace, costs, n=40):
    a, b = _tok_pairs(seed, n, overflow)
    return a, b, [_tok_ref(x, y, k, trace, costs) for x, y in zip(a, b)]


def _tok_dists(want):
    return np.array([NONE if w is None else w[0] for w in want], dtype=np.uint32)


def k_tokens(seed):
    """40 CSR pairs and 3 overflow pairs: codes, hash tables, overflow list, then the u32 wide kernel's lines (SLOT_TOK_*, SLOT_LINES)"""
    torch, T, B = _mods()
    a, b, want = _d_tokens(seed, 3, 40, False, UNIT)
    ta, tb = B.Tokens.from_list(a), B.Tokens.from_list(b)
    return Case(lambda: B.levenshtein_k_batch_tokens(ta, tb, 40, UNIT), lambda r: _same(_u32(r), _tok_dists(want)))


def exp_tokens(seed):
    """1,024 CSR pairs and 3 overflow pairs: the device-driven rounds over the codes, then the overflow pass"""
    torch, T, B = _mods()
    a, b, want = _d_tokens(seed, 3, NONE, False, UNIT, 1024)                 # (below 1,024 pairs the exp rounds synchronise)
    ta, tb = B.Tokens.from_list(a), B.Tokens.from_list(b)
    return Case(lambda: B.levenshtein_exp_batch_tokens(ta, tb, UNIT), lambda r: _same(_u32(r), _tok_dists(want)))


def _trace_tokens(seed, overflow):
    torch, T, B = _mods()
    a, b, want = _d_tokens(seed, overflow, 40, True, UNIT)
    ta, tb = B.Tokens.from_list(a), B.Tokens.from_list(b)

    def check(r):
        out, edits, ne = r
        _check_scripts(_u32(out), B.edits_to_lists(edits, ne), [(None, None) if w is None else w for w in want])

    return Case(lambda: B.levenshtein_trace_batch_tokens(ta, tb, 40, UNIT, cap=81), check)


def trace_tokens(seed):
    """no sequence beyond 255 items: the only asynchronous form of the entry (with overflow pairs it reads their count back)"""
    return _trace_tokens(seed, 0)


def trace_tokens_overflow(seed):
    """with overflow pairs the entry synchronises its stream (Part 2 only: complete when it returns)"""
    return _trace_tokens(seed, 2)


# searches over batches
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _reads(seed, n, needle_of, lo, hi):
    g = Dg.rng(seed)
    out = []
    for i in range(n):
        h = bytearray(bytes(g.choice(ACGT, int(g.integers(lo, hi + 1)))))
        nd = needle_of(i)
        if i % 4 != 3 and len(h) > len(nd):
            s = bytearray(nd)
            if i % 4 == 1:
                s[len(s) // 2] = ord("A") if s[len(s) // 2] != ord("A") else ord("C")
            at = int(g.integers(0, len(h) - len(s) + 1))
            h[at:at + len(s)] = s
        out.append(bytes(h))
    return out


def _matches_equal(B, m, c, want):
    got = [[tuple(int(v) for v in x) for x in row] for row in B.matches_to_lists(m, c)]
    assert got == [[tuple(x) for x in w] for w in want], next((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != [tuple(x) for x in w])


@functools.lru_cache(maxsize=None)
def _d_search_scan(seed):
    needle = bytes(Dg.rng(seed).choice(ACGT, 20))
    hays = _reads(seed + 1, 64, lambda i: needle, 60, 140)
    return needle, hays, [O.levenshtein_search_naive_with_opts(needle, h, 2, O.BEST, UNIT, False) for h in hays]


def search_batch_scan(seed):
    """a shared needle of 20 bytes: the scan route's candidate count, list and spans (SLOT_SB_CTL, SLOT_SB_LIST, SLOT_SB_SPAN)"""
    torch, T, B = _mods()
    needle, hays, want = _d_search_scan(seed)
    nd, hs = B.Strings.shared(needle, len(hays)), B.Strings.from_list(hays)
    return Case(lambda: B.levenshtein_search_batch(nd, hs, 2, T.SearchType.Best), lambda r: _matches_equal(B, r[0], r[1], want),
                _name_has("lev_search_batch_scan_kernel"))


@functools.lru_cache(maxsize=None)
def _d_search_long(seed):
    g = Dg.rng(seed)
    needles = [bytes(g.choice(ACGT, int(g.integers(33, 48)))) for _ in range(48)]
    hays = _reads(seed + 1, 48, lambda i: needles[i], 60, 140)
    return needles, hays, [O.levenshtein_search_naive_with_opts(nd, h, 3, O.BEST, UNIT, False) for nd, h in zip(needles, hays)]


def search_batch_long_needle(seed):
    """per-pair needles beyond 32 bytes: the memory-backed columns (SLOT_SB_COL)"""
    torch, T, B = _mods()
    needles, hays, want = _d_search_long(seed)
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    return Case(lambda: B.levenshtein_search_batch(nd, hs, 3, T.SearchType.Best), lambda r: _matches_equal(B, r[0], r[1], want),
                _name_has("lev_search_batch_mem_kernel"))


@functools.lru_cache(maxsize=None)
def _d_hsearch(seed):
    needle = bytes(Dg.rng(seed).choice(ACGT, 12))
    hays = _reads(seed + 1, 4096, lambda i: needle, 16, 40)
    return needle, hays, [O.hamming_search_simd_with_opts(needle, h, 2, O.BEST) for h in hays]


def hamming_search_batch(seed):
    """4,096 CSR haystacks: the length order of the search batch (SLOT_SB_ORDER, SLOT_SB_BINS); smaller batches take no scratch"""
    torch, T, B = _mods()
    needle, hays, want = _d_hsearch(seed)
    nd, hs = B.Strings.shared(needle, len(hays)), B.Strings.from_list(hays)
    return Case(lambda: B.hamming_search_batch(nd, hs, 2, T.SearchType.Best), lambda r: _matches_equal(B, r[0], r[1], want))


def _cross_records(B, hits, count, recs):
    cols = B.search_cross_to_arrays(hits, count)
    got = [tuple(int(c[i]) for c in cols) for i in range(len(cols[0]))]
    assert got == [tuple(r) for r in recs], (len(got), len(recs))


@functools.lru_cache(maxsize=None)
def _d_search_cross(seed):
    import search_cross_cases as Sx
    needles = Sx.panel(seed, 8)
    hays = Sx.reads(seed + 1, 48, needles, lo=60, hi=120)
    return needles, hays, Sx.join(needles, hays, 2, UNIT, False)


def search_cross(seed):
    """8 needles in 48 haystacks: the candidate records of a sub-batch and its count (SLOT_SX_CTL, SLOT_SX_REC, SLOT_SX_NEAR)"""
    torch, T, B = _mods()
    needles, hays, (recs, nearest, best, per) = _d_search_cross(seed)
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)

    def check(r):
        hits, count, _, got_best, _ = r
        _cross_records(B, hits, count, recs)
        gb = got_best.cpu().numpy()
        assert [(int(x[0]), int(x[1]), int(x[2]) & NONE) for x in gb] == [tuple(x) for x in best]

    return Case(lambda: B.levenshtein_search_cross(nd, hs, 2, UNIT, best=True), check, _name_has("lev_search_cross_scan_kernel"))


@functools.lru_cache(maxsize=None)
def _d_hsearch_cross(seed):
    import hsearch_cross_cases as Hx
    needles = Hx.panel(seed, 8)
    hays = Hx.reads(seed + 1, 48, needles, lo=60, hi=120)
    return needles, hays, Hx.join(needles, hays, 2)


def hamming_search_cross(seed):
    """8 needles in 48 haystacks: the packed nearest words (SLOT_HSX_CTL, SLOT_HSX_WORD)"""
    torch, T, B = _mods()
    needles, hays, (recs, nearest, best, per) = _d_hsearch_cross(seed)
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)

    def check(r):
        hits, count, got_near, _, got_per = r
        _cross_records(B, hits, count, recs)
        assert [int(x) & 0xFFFFFFFFFFFFFFFF for x in got_near.cpu().numpy()] == list(nearest)
        assert [int(x) & NONE for x in got_per.cpu().numpy()] == list(per)

    return Case(lambda: B.hamming_search_cross(nd, hs, 2, nearest=True, per_haystack=True), check, _name_has("ham_search_cross_kernel"))


# hamming
@functools.lru_cache(maxsize=None)
def _d_ham(seed, n, length):
    g = Dg.rng(seed)
    a = g.integers(1, 256, size=(n, length), dtype=np.uint8)
    b = a.copy()
    flip = g.random((n, length)) < 0.1
    b[flip] ^= 0x55
    return a, b, (a != b).sum(axis=1).astype(np.uint32)


def hamming_long(seed):
    """two strided pairs of 64 KiB: the sliced form's per-slice counts (SLOT_HAM_LONG)"""
    torch, T, B = _mods()
    a, b, want = _d_ham(seed, 2, 65536)
    sa, sb = B.Strings.from_fixed(a), B.Strings.from_fixed(b)
    return Case(lambda: B.hamming_batch(sa, sb), lambda r: _same(_u32(r), want), _name_has("ham_long"))


def hamming_short(seed):
    """short strings: one kernel, no scratch, records nothing by design (Part 2 only)"""
    torch, T, B = _mods()
    a, b, want = _d_ham(seed, 300, 100)
    sa, sb = B.Strings.from_fixed(a), B.Strings.from_fixed(b)
    return Case(lambda: B.hamming_batch(sa, sb), lambda r: _same(_u32(r), want))


def hamming_dev(seed):
    """one pair of 64 KiB resident in HBM: the sliced form (SLOT_HAM_LONG)"""
    torch, T, B = _mods()
    a, b, want = _d_ham(seed, 1, 65536)
    da, db = torch.from_numpy(a[0].copy()).cuda(), torch.from_numpy(b[0].copy()).cuda()
    return Case(lambda: B.hamming_dev(da, db), lambda r: _same(_u32(r), want), _name_has("ham_long"))


# the cross entries: no scratch in their asynchronous form (both length bounds known) -- Part 2 only
@functools.lru_cache(maxsize=None)
def _d_cross(seed, hamming):
    g = Dg.rng(seed)
    ts = [bytes(g.choice(ACGT, 24)) for _ in range(200)]
    qs = []
    for i in range(40):
        s = bytearray(ts[int(g.integers(len(ts)))])
        for _ in range(i % 3):
            s[int(g.integers(len(s)))] = int(g.choice(ACGT))
        qs.append(bytes(s))
    rows = []
    for q, x in enumerate(qs):
        for t, y in enumerate(ts):
            d = sum(c != e for c, e in zip(x, y)) if hamming else O.levenshtein_simd_k_with_opts(x, y, 2, False, UNIT)[0]
            if d is not None and d <= 2:
                rows.append((q, t, d))
    return qs, ts, rows


def _cross_case(seed, which):
    torch, T, B = _mods()
    qs, ts, rows = _d_cross(seed, which == "hamming")
    sq, st = B.Strings.from_list(qs), B.Strings.from_list(ts)
    fn = {"lev": lambda: B.levenshtein_cross(sq, st, 2), "opts": lambda: B.levenshtein_cross_with_opts(sq, st, 2),
          "hamming": lambda: B.hamming_cross(sq, st, 2)}[which]

    def check(r):
        q, t, d = B.cross_to_arrays(r[0], r[1])
        assert list(zip(q.tolist(), t.tolist(), d.tolist())) == rows

    return Case(fn, check)


def cross_lev(seed):
    return _cross_case(seed, "lev")


def cross_opts(seed):
    return _cross_case(seed, "opts")


def cross_hamming(seed):
    return _cross_case(seed, "hamming")


# the *_dev searches over one resident haystack: they read their count back, so they are complete when they return (Part 2 only)
@functools.lru_cache(maxsize=None)
def _d_dev_search(seed):
    needle = bytes(Dg.rng(seed).choice(ACGT, 14))
    hay = _reads(seed + 1, 1, lambda i: needle, 3000, 3000)[0]
    hay = hay[:1500] + needle[:7] + b"T" + needle[8:] + hay[1500:]
    lev = O.levenshtein_search_naive_with_opts(needle, hay, 2, O.ALL, UNIT, False)
    ham = O.hamming_search_simd_with_opts(needle, hay, 2, O.ALL)
    return needle, hay, lev, ham


def _dev_search_case(seed, which):
    torch, T, B = _mods()
    needle, hay, lev, ham = _d_dev_search(seed)
    ht = B.haystack_tensor(hay)
    by_end = sorted(lev, key=lambda m: m[1])
    kmin = min(m[2] for m in lev)
    if which == "all":
        return Case(lambda: B.levenshtein_search_dev(needle, ht, 2), lambda r: _same(r, np.array(by_end, dtype=np.int64).reshape(-1, 3)))
    if which == "best":
        want = np.array([m for m in by_end if m[2] == kmin], dtype=np.int64).reshape(-1, 3)
        return Case(lambda: B.levenshtein_search_best_dev(needle, ht, 2), lambda r: _same(r, want))
    if which == "first":
        return Case(lambda: B.levenshtein_search_first_dev(needle, ht, 2), lambda r: _same(np.array(r), np.array(by_end[0])))
    want = np.array(sorted(ham, key=lambda m: m[1]), dtype=np.int64).reshape(-1, 3)
    return Case(lambda: B.hamming_search_dev(needle, ht, 2), lambda r: _same(r, want))


def best_hits_dev(seed):
    """ta_search_best_hits_dev over an All-mode result that already lies in HBM (the oracle's records): SLOT_SEARCH_CTL, SLOT_SELECT"""
    import ctypes as C
    torch, T, B = _mods()
    from triple_accel_amd import _native as N
    needle, hay, lev, ham = _d_dev_search(seed)
    hits = torch.from_numpy(np.array(lev, dtype=np.int64).reshape(-1, 3).copy()).cuda()      # ta_match: u64 start, u64 end, u32 k + pad
    kmin = min(m[2] for m in lev)
    want = sorted((tuple(m) for m in lev if m[2] == kmin), key=lambda m: m[1])

    def run():
        out, n = C.POINTER(N.MatchC)(), C.c_size_t()
        T._raise(N.lib().ta_search_best_hits_dev(hits.data_ptr(), len(lev), C.byref(out), C.byref(n), B._stream()))
        rows = [(int(out[i].start), int(out[i].end), int(out[i].k)) for i in range(n.value)]
        N.lib().ta_free(out)
        return rows

    return Case(run, lambda r: _eq(r, want))


def search_dev_all(seed):
    return _dev_search_case(seed, "all")


def search_dev_best(seed):
    return _dev_search_case(seed, "best")


def search_dev_first(seed):
    return _dev_search_case(seed, "first")


def hamming_search_dev(seed):
    return _dev_search_case(seed, "hamming")


# Part 1: every A route that takes scratch and stays asynchronous
PART1 = [k_ragged, k_prefilter, k_widebits_lines, k_widebits_tiles, k_wide, k_alphabet, exp_batch, trace_ckpt, trace_records,
         trace_packed_ckpt, trace_packed_records, k_tokens, exp_tokens, trace_tokens, search_batch_scan, search_batch_long_needle,
         hamming_search_batch, search_cross, hamming_search_cross, hamming_long, hamming_dev]
# Part 2, asynchronous B's: the same, the no-scratch routes, the cross entries, and the entries that synchronise their own stream
PART2_ASYNC = PART1 + [k_small_ragged, k_fixed, hamming_short, cross_lev, cross_opts, cross_hamming, trace_tokens_overflow,
                       search_dev_all, search_dev_best, search_dev_first, hamming_search_dev, best_hits_dev]


# ---------------------------------------------------------------------------------------------------------------- single calls (Part 2)
def _single(fn, want, route=None):
    def check(r):
        assert r == want, (r, want)
    return Case(fn, check, route)


def _trace_want(a, b, k, costs):
    d, tr = O.levenshtein_simd_k_with_opts(a, b, k, True, costs)
    return None if d is None else (d, _norm(tr))


def _trace_got(r):
    return None if r is None else (r[0], _norm(r[1]))


def s_hamming_short(seed):
    import triple_accel_amd as T
    a, b, want = _d_ham(seed, 1, 200)
    return _single(lambda: T.hamming(a[0].tobytes(), b[0].tobytes()), int(want[0]))


def s_hamming_chunked(seed):
    """a pair above TA_HAM_HOST_CHUNK (set to 1,024 bytes under TA_TUNING): staged piece by piece (SLOT_PAIR_STAGE, SLOT_HAM_LONG)"""
    import triple_accel_amd as T
    a, b, want = _d_ham(seed, 1, 5000)
    x, y = a[0].tobytes(), b[0].tobytes()
    assert os.environ.get("TA_TUNING"), "the tuning switches are read only under TA_TUNING (tests/conftest.py sets it)"

    def run():
        old = os.environ.get("TA_HAM_HOST_CHUNK")
        os.environ["TA_HAM_HOST_CHUNK"] = "1024"
        try:
            return T.hamming(x, y)
        finally:
            if old is None:
                del os.environ["TA_HAM_HOST_CHUNK"]
            else:
                os.environ["TA_HAM_HOST_CHUNK"] = old

    return _single(run, int(want[0]), _name_has("ham_long"))


@functools.lru_cache(maxsize=None)
def _d_pair(seed, length, edits):
    return _long_pair(seed, length, edits)


def s_k_short(seed):
    import triple_accel_amd as T
    a, b = _d_pair(seed, 60, 8)
    return _single(lambda: T.levenshtein_simd_k_with_opts(a, b, 10, False, UNIT), (O.levenshtein_simd_k_with_opts(a, b, 10, False, UNIT)[0], None))


def s_k_wide(seed):
    """weighted costs beyond the register band: the DP wide kernel (SLOT_LINES)"""
    import triple_accel_amd as T
    a, b = _d_pair(seed, 4300, 30)
    want = (O.levenshtein_simd_k_with_opts(a, b, NONE, False, WEIGHTED)[0], None)
    return _single(lambda: T.levenshtein_simd_k_with_opts(a, b, NONE, False, WEIGHTED), want, _kernel_is(2))


def s_exp(seed):
    import triple_accel_amd as T
    a, b = _d_pair(seed, 300, 50)
    return _single(lambda: T.levenshtein_exp(a, b), O.levenshtein_exp(a, b))


def s_trace_band(seed):
    """traceback inside the register band: the DP band kernel's records (SLOT_LINES)"""
    import triple_accel_amd as T
    a, b = _d_pair(seed, 60, 8)
    want = _trace_want(a, b, 10, WEIGHTED)
    return Case(lambda: T.levenshtein_simd_k_with_opts(a, b, 10, True, WEIGHTED), lambda r: _eq(_trace_got(r), want))


def s_trace_widebits(seed):
    """unit costs beyond the register band: trace_widebits (SLOT_TRACE, SLOT_LINES)"""
    import triple_accel_amd as T
    a, b = _d_pair(seed, 4300, 30)
    want = _trace_want(a, b, NONE, UNIT)
    return Case(lambda: T.levenshtein_simd_k_with_opts(a, b, NONE, True, UNIT), lambda r: _eq(_trace_got(r), want))


def s_trace_wide(seed):
    """weighted costs beyond the register band: trace_wide (SLOT_TRACE, SLOT_LINES)"""
    import triple_accel_amd as T
    a, b = _d_pair(seed, 4300, 30)
    want = _trace_want(a, b, NONE, GAPPY)
    return Case(lambda: T.levenshtein_simd_k_with_opts(a, b, NONE, True, GAPPY), lambda r: _eq(_trace_got(r), want))


def s_exp_trace(seed):
    import triple_accel_amd as T
    a, b = _d_pair(seed, 200, 50)
    d, tr = O.levenshtein_exp_with_opts(a, b, True, UNIT)
    return Case(lambda: T.levenshtein_exp_with_opts(a, b, True, UNIT), lambda r: _eq((r[0], _norm(r[1])), (d, _norm(tr))))


def _eq(got, want):
    assert got == want, (got, want)


def _tokens_single(seed, wide, trace):
    import triple_accel_amd as T
    a, b = _tok_pairs(seed, 4, 1 if wide else 0)
    x, y = (a[2], b[2]) if wide else (a[1], b[1])
    import tokens_ref as R
    assert (R.codes(x, y) is None) == wide
    w = _tok_ref(x, y, 40, trace, UNIT)
    want = None if w is None else (w[0], _norm(w[1]) if trace else None)
    return Case(lambda: T.levenshtein_tokens(x, y, 40, trace, UNIT), lambda r: _eq(None if r is None else (r[0], _norm(r[1])), want))


def s_tokens_coded(seed):
    return _tokens_single(seed, False, False)


def s_tokens_coded_edits(seed):
    return _tokens_single(seed, False, True)


def s_tokens_wide(seed):
    """more than 254 common items: wide_pair_u32 (SLOT_TOK_STAGE, SLOT_LINES)"""
    return _tokens_single(seed, True, False)


def s_tokens_wide_edits(seed):
    """... with its records (SLOT_TRACE)"""
    return _tokens_single(seed, True, True)


def _search_single(seed, st):
    import triple_accel_amd as T
    needle, hay, lev, ham = _d_dev_search(seed)
    want = O.levenshtein_search_naive_with_opts(needle, hay, 2, st, UNIT, False)
    return Case(lambda: [tuple(m) for m in T.levenshtein_search_simd_with_opts(needle, hay, 2, st, UNIT, False)], lambda r: _eq(r, [tuple(m) for m in want]))


def s_search_all(seed):
    return _search_single(seed, O.ALL)


def s_search_best(seed):
    return _search_single(seed, O.BEST)


def s_hamming_search(seed):
    import triple_accel_amd as T
    needle, hay, lev, ham = _d_dev_search(seed)
    k = (len(needle) >> 1) + (len(needle) & 1)
    want = O.hamming_search_simd_with_opts(needle, hay, k, O.BEST)
    return Case(lambda: [tuple(m) for m in T.hamming_search(needle, hay)], lambda r: _eq(r, [tuple(m) for m in want]))


def s_hamming_search_naive(seed):
    """the scalar routine's contract (NUL bytes are fine) over the same host path"""
    import triple_accel_amd as T
    needle, hay, lev, ham = _d_dev_search(seed)
    hay = hay[:100] + b"\0" + hay[100:]
    want = O.hamming_search_naive_with_opts(needle, hay, 3, O.ALL)
    return Case(lambda: [tuple(m) for m in T.hamming_search_naive_with_opts(needle, hay, 3, T.SearchType.All)], lambda r: _eq(r, [tuple(m) for m in want]))


@functools.lru_cache(maxsize=None)
def _d_lazy(seed):
    g = Dg.rng(seed)
    needle = bytes(g.choice(ACGT, 16))
    hay = bytearray(bytes(g.choice(ACGT, 1 << 20)))
    for at in (700_001, 900_017):
        hay[at:at + 16] = needle
    hay = bytes(hay)
    return needle, hay, O.levenshtein_search_naive_with_opts(needle, hay, 1, O.ALL, UNIT, False)


def s_search_first(seed):
    """the first match of a 1 MiB haystack: windows of the staging buffer (SLOT_SEARCH_HAY, SLOT_SEARCH_HITS)"""
    import triple_accel_amd as T
    needle, hay, want = _d_lazy(seed)
    return Case(lambda: tuple(T.levenshtein_search_first(needle, hay, 1)), lambda r: _eq(r, tuple(want[0])))


def s_search_resume(seed):
    """the lazy iterator's second element: ta_levenshtein_search_resume on the bytes the first call left resident.  The first element is
    taken before the gate is armed (prep), the resume is the call the gate looks at"""
    import triple_accel_amd as T
    needle, hay, want = _d_lazy(seed)
    state = {}

    def prep():
        state["it"] = T.levenshtein_search_simd_with_opts(needle, hay, 1, T.SearchType.All, UNIT, False)
        state["first"] = tuple(next(state["it"]))

    def run():
        return [state["first"]] + [tuple(m) for m in state["it"]]

    return Case(run, lambda r: _eq(r, [tuple(m) for m in want]), prep=prep)


def s_queue_flush(seed):
    """a Queue flush: a ragged batch on the queue's own stream"""
    import triple_accel_amd as T
    import torch
    a, b, want = _d_k_small(seed)
    state = {"q": T.Queue(8)}

    def run():
        for x, y in zip(a, b):
            state["q"].push(x, y)
        return state["q"].flush()

    def control(gate):
        """the queue's stream is the library's: of at most 8 queues, the first whose flush overtakes the gate"""
        for _ in range(8):
            run()                                                  # (sizes the queue's staging memory)
            torch.cuda.synchronize()
            gate.arm()
            run()
            ok = not gate.s1.query()
            gate.s1.synchronize()
            if ok:
                return
            state["q"].close()
            state["q"] = T.Queue(8)
        raise AssertionError("none of 8 queues' streams overtook the gate: the flush cannot be told from one that waits")

    return Case(run, lambda r: _eq(r, [None if w == NONE else int(w) for w in want]), close=lambda: state["q"].close(), control=control)


PART2_SYNC = [s_hamming_short, s_hamming_chunked, s_k_short, s_k_wide, s_exp, s_trace_band, s_trace_widebits, s_trace_wide, s_exp_trace,
              s_tokens_coded, s_tokens_coded_edits, s_tokens_wide, s_tokens_wide_edits, s_search_all, s_search_best, s_search_first,
              s_search_resume, s_hamming_search, s_hamming_search_naive, s_queue_flush]
