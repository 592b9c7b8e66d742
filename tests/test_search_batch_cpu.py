"""not-gpu: the search batch body (lev_search_batch_body.h) under host emulation -- one pair as one lane of the batch kernels runs it
(the scan with a host-built match table, the span, the exact pass with the online Best fold) against the scalar oracle
levenshtein_search_naive_with_opts, All and Best, every cost family; plus the ABI's argument errors and its refusal to run without a
device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_search_batch")
COSTS = [(1, 1, 0, None), (1, 1, 0, 1), (3, 1, 0, None), (1, 1, 2, None), (2, 1, 2, None), (2, 2, 1, 3), (1, 2, 0, 1), (2, 3, 1, None)]


class _Match(C.Structure):
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("k", C.c_uint32), ("pad", C.c_uint32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(EMU_DIR, "libta_emu_search_batch.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        u8p, u32, u64, i = C.c_char_p, C.c_uint32, C.c_uint64, C.c_int
        _lib.emu_search_batch_pair.argtypes = [u8p, u32, u8p, u64, u32, i, u32, u32, u32, i, u32, i, i, u32, i, C.c_void_p, u64,
                                               C.POINTER(u64), C.POINTER(u64)]
        _lib.emu_search_batch_pair.restype = u32
        _lib.emu_search_batch_fold.argtypes = [C.c_void_p, u64, u32, i, C.c_void_p, u64]
        _lib.emu_search_batch_fold.restype = u32
        _lib.emu_search_batch_filter_k.argtypes = [u32, u32, u32, u32, i, u32]
        _lib.emu_search_batch_filter_k.restype = u32
    return _lib


def filter_k(k, costs):
    mc, gc, sg, t = costs
    if (mc, gc, sg) == (1, 1, 0) and t in (None, 1):
        return k
    return int(lib().emu_search_batch_filter_k(k, mc, gc, sg, t is not None, t or 0))


def emu_pair(needle, hay, k, best, costs, anchored=False, route_s=False, form=0, cap=None):
    """-> (count, matches[:min(count, cap)], (first, last)) of one pair"""
    mc, gc, sg, t = costs
    cap = len(hay) + 2 if cap is None else cap
    out = (_Match * max(cap, 1))()
    f, l = C.c_uint64(), C.c_uint64()
    nb = bytes(needle) + bytes(16)                      # (the blobs' read slack)
    hb = bytes(hay) + bytes(16)
    cnt = lib().emu_search_batch_pair(nb, len(needle), hb, len(hay), k, int(best), mc, gc, sg, t is not None, t or 0, int(anchored),
                                      int(route_s), filter_k(k, costs), form, C.cast(out, C.c_void_p), cap, C.byref(f), C.byref(l))
    return cnt, [(int(m.start), int(m.end), int(m.k)) for m in out[:min(cnt, cap)]], (f.value, l.value)


def oracle(needle, hay, k, best, costs, anchored=False):
    return O.levenshtein_search_naive_with_opts(needle, hay, k, O.BEST if best else O.ALL, costs, anchored)


def routes(n, k, costs, anchored):
    """the (route_s, form) combinations the batch kernels can take for this needle"""
    out = [(False, 0), (False, 2)]
    if 1 <= n <= 32:
        out.append((False, 1))
    if 1 <= n <= 64 and not anchored and filter_k(k, costs) < n:
        out += [(True, 0), (True, 2)] + ([(True, 1)] if n <= 32 else [])
    return [(s, f) for s, f in out if not (f != 2 and n > 32)]


def check(needle, hay, k, costs, anchored=False):
    for best in (False, True):
        want = oracle(needle, hay, k, best, costs, anchored)
        for route_s, form in routes(len(needle), k, costs, anchored):
            cnt, got, _ = emu_pair(needle, hay, k, best, costs, anchored, route_s, form)
            assert cnt == len(want) and got == want, (needle, hay[:80], len(hay), k, costs, anchored, best, route_s, form)


@pytest.mark.parametrize("costs", COSTS)
def test_pairs_equal_the_oracle(costs):
    assert O.costs_valid(costs) and O.costs_valid_search(costs)
    g = Dg.rng(1701)
    for n in (1, 2, 5, 13, 24, 32, 33, 40, 64, 70):
        needle = Dg.rand_str(g, n)
        for k in sorted({0, 1, n // 4 + 1, (n + 1) // 2, n, n + 3}):
            for hlen in (0, 1, n - 1 if n > 1 else 0, 300):
                hay = Dg.planted_haystack(int(g.integers(1 << 30)), needle, hlen, 70, max(1, k)) if hlen >= 64 else Dg.rand_str(g, hlen)
                check(needle, hay, k, costs)
                if n <= 33:
                    check(needle, hay, k, costs, anchored=True)


@pytest.mark.parametrize("costs", COSTS)
def test_small_alphabets_ties_and_q2(costs):
    """binary needles and haystacks maximise cost ties, where the length tie rules (quirk Q2) and the Best fold's replace rule bite"""
    g = Dg.rng(77)
    for _ in range(60):
        n = int(g.integers(1, 12))
        needle = g.integers(97, 99, size=n, dtype=np.uint8).tobytes()
        hay = g.integers(97, 99, size=int(g.integers(0, 120)), dtype=np.uint8).tobytes()
        k = int(g.integers(0, n + 3))
        check(needle, hay, k, costs, anchored=bool(g.integers(2)))
        check(needle, hay, k, costs)


def test_acgt_reads_with_planted_needles():
    g = Dg.rng(5)
    for costs in COSTS:
        for _ in range(12):
            n = int(g.integers(8, 40))
            needle = bytes(g.choice(np.frombuffer(b"ACGT", np.uint8), n))
            hay = bytearray(g.choice(np.frombuffer(b"ACGT", np.uint8), int(g.integers(50, 250))))
            m = bytearray(needle)
            for _ in range(int(g.integers(0, 3))):
                m[int(g.integers(len(m)))] = int(g.choice(np.frombuffer(b"ACGT", np.uint8)))
            p = int(g.integers(0, len(hay) - len(m) + 1)) if len(hay) > len(m) else 0
            hay[p:p + len(m)] = m
            check(needle, bytes(hay), int(g.integers(0, 6)), costs)


def test_byte_extremes():
    """the NUL byte and every byte value: the search has no NUL-byte check, the match table covers 0..255"""
    allb = bytes(range(256))
    for costs in COSTS[:4]:
        check(b"\x00", b"\x00" * 40 + b"\x01\x00", 0, costs)
        check(b"\x00\x00\x01", allb + b"\x00\x00\x01" + allb[::-1], 1, costs)
        check(allb[250:] + allb[:3], allb * 2, 2, costs)
        check(allb[:40], allb, 5, costs)


def test_empty_needle_and_empty_haystack():
    for costs in COSTS:
        for hay in (b"", b"a", b"abcdefgh"):
            for k in (0, 1, 3, 9):
                check(b"", hay, k, costs)
                check(b"", hay, k, costs, anchored=True)
                check(b"xyz", b"", k, costs)
                check(b"xyz", b"", k, costs, anchored=True)


def test_needle_longer_than_haystack():
    g = Dg.rng(9)
    for costs in COSTS:
        for n in (10, 31, 45):
            needle = Dg.rand_str(g, n)
            for k in (0, 3, n, 2 * n + 5):
                check(needle, needle[2:7], k, costs)
                check(needle, needle[2:7], k, costs, anchored=True)


def test_scan_span_is_a_superset_of_the_hits():
    """the scanned span [first, last] holds every hit's end, and the pairs without one have no hit beyond the end == 0 match"""
    g = Dg.rng(13)
    for costs in COSTS:
        for _ in range(40):
            n = int(g.integers(1, 65))
            needle = Dg.rand_str(g, n)
            hay = Dg.planted_haystack(int(g.integers(1 << 30)), needle, int(g.integers(64, 400)), 150, 2)
            k = int(g.integers(0, n + 1))
            if filter_k(k, costs) >= n:
                continue
            want = [m for m in oracle(needle, hay, k, False, costs) if m[1] > 0]
            _, _, (first, last) = emu_pair(needle, hay, k, False, costs, route_s=True)
            if not want:
                continue
            assert first and first <= want[0][1] and want[-1][1] <= last, (n, k, costs, first, last, want[0], want[-1])


def _fold_best(hits, k):
    """ta_search_fold_best with overlap_fold = 1, as the single-call host form runs it"""
    from triple_accel_amd import _native as N
    arr = (N.MatchC * max(len(hits), 1))(*[N.MatchC(s, e, kk, 0) for s, e, kk in hits])
    m = N.lib().ta_search_fold_best(arr, len(hits), k, 1)
    return [(int(arr[i].start), int(arr[i].end), int(arr[i].k)) for i in range(m)]


def test_online_fold_equals_the_two_pass_fold():
    g = Dg.rng(21)
    for _ in range(3000):
        n_hits = int(g.integers(0, 14))
        ends = np.sort(g.integers(1, 40, size=n_hits))
        hits = [(int(max(0, e - int(g.integers(0, 6)))), int(e), int(g.integers(0, 5))) for e in ends]
        k = int(g.integers(0, 6))
        hits = [h for h in hits if h[2] <= k]
        arr = (_Match * max(len(hits), 1))(*[_Match(s, e, kk, 0) for s, e, kk in hits])
        for cap in (0, 1, 3, 64):
            out = (_Match * max(cap, 1))()
            cnt = lib().emu_search_batch_fold(C.cast(arr, C.c_void_p), len(hits), k, 1, C.cast(out, C.c_void_p), cap)
            want = _fold_best(list(hits), k)
            assert cnt == len(want)
            assert [(m.start, m.end, m.k) for m in out[:min(cnt, cap)]] == want[:cap], (hits, k, cap)
            cnt_all = lib().emu_search_batch_fold(C.cast(arr, C.c_void_p), len(hits), k, 0, C.cast(out, C.c_void_p), cap)
            assert cnt_all == len(hits) and [(m.start, m.end, m.k) for m in out[:min(cnt_all, cap)]] == hits[:cap]


def test_cap_cut_keeps_the_prefix():
    needle, hay = b"ab", b"ab" * 50
    for best in (False, True):
        full_cnt, full, _ = emu_pair(needle, hay, 1, best, COSTS[0])
        for cap in (0, 1, 5):
            cnt, got, _ = emu_pair(needle, hay, 1, best, COSTS[0], cap=cap)
            assert cnt == full_cnt and got == full[:cap]


# ---------------------------------------------------------------- the C ABI: argument errors come first, no CPU fallback
def _abi():
    from triple_accel_amd import _native as N
    return N


def _call(needles, hays, n, k=1, st=1, costs=None, matches=None, counts=None, cap=0):
    N = _abi()
    cc = costs if costs is not None else N.EditCostsC(1, 1, 0, 0, 0)
    return N.lib().ta_levenshtein_search_batch(needles, hays, n, k, st, C.byref(cc), 0, matches, counts, cap, None)


def test_abi_argument_errors():
    N = _abi()
    blob = (C.c_uint8 * 64)()
    s = N.StringsC(C.cast(blob, C.c_void_p).value, 0, 0, 8, 0)
    fake = C.c_void_p(0x1000)
    assert _call(None, C.byref(s), 1, counts=fake) == N.TA_ERR_ARG
    assert _call(C.byref(s), None, 1, counts=fake) == N.TA_ERR_ARG
    assert _call(C.byref(s), C.byref(s), 1, st=2, counts=fake) == N.TA_ERR_ARG
    assert _call(C.byref(s), C.byref(s), 1, counts=None) == N.TA_ERR_ARG                   # counts_dev is required
    assert _call(C.byref(s), C.byref(s), 1, counts=fake, cap=4, matches=None) == N.TA_ERR_ARG
    assert _call(C.byref(s), C.byref(s), 1 << 20, counts=fake, cap=1 << 60, matches=fake) == N.TA_ERR_ARG   # n * cap overflows
    long_needle = N.StringsC(C.cast(blob, C.c_void_p).value, 0, 0, 65536, 0)
    assert _call(C.byref(long_needle), C.byref(s), 1, counts=fake) == N.TA_ERR_ARG
    huge_hay = N.StringsC(C.cast(blob, C.c_void_p).value, 0, 1 << 32, 1 << 32, 0)
    assert _call(C.byref(s), C.byref(huge_hay), 1, counts=fake) == N.TA_ERR_UNSUPPORTED
    # EditCosts::new and check_search decide for the whole batch, whatever the needles
    assert _call(C.byref(s), C.byref(s), 1, counts=fake, costs=N.EditCostsC(0, 1, 0, 0, 0)) == N.TA_ERR_BAD_COSTS
    empty = N.StringsC(C.cast(blob, C.c_void_p).value, 0, 0, 0, 0)
    assert _call(C.byref(empty), C.byref(s), 1, counts=fake, costs=N.EditCostsC(1, 1, 0, 1, 3)) == N.TA_ERR_BAD_COSTS


def test_no_cpu_fallback():
    import torch
    N = _abi()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    blob = (C.c_uint8 * 64)()
    s = N.StringsC(C.cast(blob, C.c_void_p).value, 0, 0, 8, 0)
    counts = (C.c_uint32 * 4)()
    assert _call(C.byref(s), C.byref(s), 1, counts=C.cast(counts, C.c_void_p)) == N.TA_ERR_HIP
    assert _call(C.byref(s), C.byref(s), 0, counts=None) == N.TA_ERR_HIP
