"""not-gpu: the Hamming search batch body (ham_search_batch_body.h) under host emulation -- one pair as one lane of the batch kernels
runs it in every form it can take (register form with 2 / 4 / 8 / 16 needle dwords, memory form, bit-sliced form) against the oracle
hamming_search_simd_with_opts, All and Best, the NUL verdict and its place behind the two length checks; the online Best fold against
ta_search_fold_best(.., overlap_fold = 0); plus the ABI's argument errors and its refusal to run without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_hsearch_batch")
NONE = 0xFFFFFFFF
CANNOT = 0xFFFFFFFE


class _Match(C.Structure):
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("k", C.c_uint32), ("pad", C.c_uint32)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(EMU_DIR, "libta_emu_hsearch_batch.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        u8p, u32, u64, i = C.c_char_p, C.c_uint32, C.c_uint64, C.c_int
        _lib.emu_hsearch_batch_pair.argtypes = [u8p, u64, u8p, u64, u32, i, i, C.c_void_p, u64]
        _lib.emu_hsearch_batch_pair.restype = u32
        _lib.emu_hsearch_batch_fold.argtypes = [C.c_void_p, u64, u32, i, C.c_void_p, u64]
        _lib.emu_hsearch_batch_fold.restype = u32
    return _lib


def forms(n, k):
    """the forms the batch kernels can take for this needle: register forms wide enough, the memory form, the bit-sliced form"""
    out = [0] + [nw for nw in (2, 4, 8, 16) if n <= 4 * nw]
    if 1 <= n <= 32 and k < n:
        out.append(1)
    return out


def emu_pair(needle, hay, k, best, form, cap=None):
    """-> (count word, matches[:min(count, cap)]) of one pair"""
    cap = len(hay) + 2 if cap is None else cap
    out = (_Match * max(cap, 1))()
    nb = bytes(needle) + b"\xa5" * 16                   # (the blobs' read slack, never NUL: a stray read must not look like a verdict)
    hb = bytes(hay) + b"\xa5" * 16
    cnt = lib().emu_hsearch_batch_pair(nb, len(needle), hb, len(hay), k, int(best), form, C.cast(out, C.c_void_p), cap)
    assert cnt != CANNOT, (len(needle), k, form)
    if cnt == NONE:
        return cnt, []
    got = [(int(m.start), int(m.end), int(m.k)) for m in out[:min(cnt, cap)]]
    assert all(m.pad == 0 for m in out[:min(cnt, cap)])
    return cnt, got


def oracle(needle, hay, k, best):
    """the pair's expected (count word, matches): the NUL verdict where the reference panics"""
    try:
        want = O.hamming_search_simd_with_opts(needle, hay, k, O.BEST if best else O.ALL)
    except ValueError:
        return NONE, []
    return len(want), want


def check(needle, hay, k):
    for best in (False, True):
        want = oracle(needle, hay, k, best)
        for form in forms(len(needle), k):
            assert emu_pair(needle, hay, k, best, form) == want, (needle, hay[:80], len(hay), k, best, form)


def ks(n):
    return sorted({0, 1, n // 2, max(n - 1, 0), n, n + 5})


def nz_bytes(g, n):
    s = Dg.random_bytes(g, n).tobytes()                 # bytes 1..255
    assert 0 not in s
    return s


def test_pairs_equal_the_oracle_bytes_1_to_255():
    g = Dg.rng(4101)
    for n in list(range(1, 71)) + [100, 300]:
        needle = nz_bytes(g, n)
        hlens = sorted({0, 1, max(n - 1, 0), n, n + 1, n + 17, int(g.integers(n, 401)) if n < 400 else n, 400})
        for hlen in hlens:
            hay = bytearray(nz_bytes(g, hlen))
            if hlen >= n:                                # a planted copy with 0..4 substitutions
                m = bytearray(needle)
                for _ in range(int(g.integers(0, 5))):
                    m[int(g.integers(n))] = int(g.integers(1, 256))
                p = int(g.integers(0, hlen - n + 1))
                hay[p:p + n] = m
            for k in ks(n):
                check(needle, bytes(hay), k)


def test_every_haystack_length_0_to_400():
    g = Dg.rng(4102)
    needle = b"GATTACAGATTACA"
    for hlen in range(0, 401):
        hay = bytearray(g.choice(np.frombuffer(b"ACGT", np.uint8), hlen))
        if hlen >= len(needle) + 3:
            hay[3:3 + len(needle)] = needle[:5] + b"C" + needle[6:]
        check(needle, bytes(hay), 2)
    for n in (3, 9, 33, 65):
        needle = nz_bytes(g, n)
        for hlen in range(0, 120):
            check(needle, nz_bytes(g, hlen), n // 2)


def test_two_letter_alphabets_many_ties():
    g = Dg.rng(4103)
    for _ in range(300):
        n = int(g.integers(1, 40))
        needle = g.integers(97, 99, size=n, dtype=np.uint8).tobytes()
        hay = g.integers(97, 99, size=int(g.integers(0, 200)), dtype=np.uint8).tobytes()
        for k in ks(n):
            check(needle, hay, k)


def test_planted_copies_with_0_to_4_substitutions():
    g = Dg.rng(4104)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    for _ in range(200):
        n = int(g.integers(1, 71))
        needle = bytes(g.choice(acgt, n))
        hay = bytearray(g.choice(acgt, int(g.integers(n, 401))))
        for subs in range(5):
            m = bytearray(needle)
            for _ in range(subs):
                m[int(g.integers(n))] = int(g.choice(acgt))
            p = int(g.integers(0, len(hay) - n + 1))
            hay[p:p + n] = m
        for k in (0, 2, 4, n // 2):
            check(needle, bytes(hay), k)


def test_nul_verdict_comes_after_the_length_checks():
    g = Dg.rng(4105)
    for n in (1, 4, 7, 24, 32, 33, 64, 65, 100):
        needle = nz_bytes(g, n)
        for hlen in (n, n + 1, n + 30, 257):
            for where in (0, hlen // 2, hlen - 1):
                hay = bytearray(nz_bytes(g, hlen))
                hay[where] = 0
                for k in ks(n):
                    for best in (False, True):
                        assert oracle(needle, bytes(hay), k, best) == (NONE, [])
                        for form in forms(n, k):
                            assert emu_pair(needle, bytes(hay), k, best, form)[0] == NONE, (n, hlen, where, k, best, form)
        # the same haystacks shorter than the needle: an empty result, no verdict
        for hlen in sorted({1, max(n - 1, 1)}):
            if hlen >= n:
                continue
            for where in sorted({0, hlen // 2, hlen - 1}):
                hay = bytearray(nz_bytes(g, hlen))
                hay[where] = 0
                check(needle, bytes(hay), n // 2)
                assert oracle(needle, bytes(hay), 1, True) == (0, [])
    # the empty needle: an empty result whatever the haystack holds
    for hay in (b"", b"\x00", b"ab\x00cd"):
        for best in (False, True):
            for form in (0, 2, 4, 8, 16):
                assert emu_pair(b"", hay, 3, best, form) == (0, [])
            assert oracle(b"", hay, 3, best) == (0, [])


def test_nul_bytes_in_the_needle_are_not_an_error():
    g = Dg.rng(4106)
    for n in (1, 5, 24, 40, 70):
        needle = bytearray(nz_bytes(g, n))
        needle[0] = 0
        needle[n // 2] = 0
        needle[n - 1] = 0
        hay = nz_bytes(g, 150)
        for k in ks(n):
            check(bytes(needle), hay, k)


def test_cap_smaller_equal_and_zero():
    needle, hay = b"ab", b"abab" * 25 + b"a"
    for best in (False, True):
        for k in (0, 1):
            full_cnt, full = emu_pair(needle, hay, k, best, 2)
            assert (full_cnt, full) == oracle(needle, hay, k, best) and full_cnt > 5
            for form in forms(2, k):
                for cap in (0, 1, 5, full_cnt, full_cnt + 3):
                    assert emu_pair(needle, hay, k, best, form, cap=cap) == (full_cnt, full[:cap]), (best, k, form, cap)


def _fold_best(hits, k):
    """ta_search_fold_best with overlap_fold = 0"""
    from triple_accel_amd import _native as N
    arr = (N.MatchC * max(len(hits), 1))(*[N.MatchC(s, e, kk, 0) for s, e, kk in hits])
    m = N.lib().ta_search_fold_best(arr, len(hits), k, 0)
    return [(int(arr[i].start), int(arr[i].end), int(arr[i].k)) for i in range(m)]


def test_online_fold_equals_the_two_pass_fold():
    g = Dg.rng(4107)
    for _ in range(3000):
        n_hits = int(g.integers(0, 14))
        starts = np.sort(g.choice(60, size=n_hits, replace=False)) if n_hits else []
        k = int(g.integers(0, 6))
        hits = [(int(s), int(s) + 7, int(g.integers(0, 5))) for s in starts]
        hits = [h for h in hits if h[2] <= k]
        arr = (_Match * max(len(hits), 1))(*[_Match(s, e, kk, 0) for s, e, kk in hits])
        for cap in (0, 1, 3, 64):
            out = (_Match * max(cap, 1))()
            cnt = lib().emu_hsearch_batch_fold(C.cast(arr, C.c_void_p), len(hits), k, 1, C.cast(out, C.c_void_p), cap)
            want = _fold_best(list(hits), k)
            assert cnt == len(want)
            assert [(m.start, m.end, m.k) for m in out[:min(cnt, cap)]] == want[:cap], (hits, k, cap)
            cnt_all = lib().emu_hsearch_batch_fold(C.cast(arr, C.c_void_p), len(hits), k, 0, C.cast(out, C.c_void_p), cap)
            assert cnt_all == len(hits) and [(m.start, m.end, m.k) for m in out[:min(cnt_all, cap)]] == hits[:cap]


# ---------------------------------------------------------------- the C ABI: argument errors come first, no CPU fallback
def _abi():
    from triple_accel_amd import _native as N
    return N


def _call(needles, hays, n, k=1, st=1, matches=None, counts=None, cap=0):
    return _abi().lib().ta_hamming_search_batch(needles, hays, n, k, st, matches, counts, cap, None)


def test_abi_symbol_is_declared_and_exported():
    N = _abi()
    assert "ta_hamming_search_batch" in N.ABI_SYMBOLS and hasattr(N.lib(), "ta_hamming_search_batch")


def test_abi_argument_errors():
    N = _abi()
    blob = (C.c_uint8 * 64)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 0, 8, 0)
    fake = C.c_void_p(0x1000)
    assert _call(None, C.byref(s), 1, counts=fake) == N.TA_ERR_ARG
    assert _call(C.byref(s), None, 1, counts=fake) == N.TA_ERR_ARG
    assert _call(None, None, 0) == N.TA_ERR_ARG
    noblob = N.StringsC(0, 0, 0, 8, 0)
    assert _call(C.byref(noblob), C.byref(s), 1, counts=fake) == N.TA_ERR_ARG
    assert _call(C.byref(s), C.byref(noblob), 1, counts=fake) == N.TA_ERR_ARG
    assert _call(C.byref(s), C.byref(s), 1, counts=None) == N.TA_ERR_ARG                   # counts_dev is required
    assert _call(C.byref(s), C.byref(s), 1, counts=fake, cap=4, matches=None) == N.TA_ERR_ARG
    for st in (2, -1, 7):
        assert _call(C.byref(s), C.byref(s), 1, st=st, counts=fake) == N.TA_ERR_ARG
    assert _call(C.byref(s), C.byref(s), 1 << 20, counts=fake, cap=1 << 60, matches=fake) == N.TA_ERR_ARG   # n * cap overflows
    long_needle = N.StringsC(ptr, 0, 0, 65536, 0)
    assert _call(C.byref(long_needle), C.byref(s), 1, counts=fake) == N.TA_ERR_ARG
    long_csr_needle = N.StringsC(ptr, 0x1000, 0, 0, 65536)
    assert _call(C.byref(long_csr_needle), C.byref(s), 1, counts=fake) == N.TA_ERR_ARG
    huge_hay = N.StringsC(ptr, 0, 1 << 32, 1 << 32, 0)
    assert _call(C.byref(s), C.byref(huge_hay), 1, counts=fake) == N.TA_ERR_UNSUPPORTED
    huge_csr_hay = N.StringsC(ptr, 0x1000, 0, 0, 1 << 32)
    assert _call(C.byref(s), C.byref(huge_csr_hay), 1, counts=fake) == N.TA_ERR_UNSUPPORTED


def test_no_cpu_fallback():
    import torch
    N = _abi()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    blob = (C.c_uint8 * 64)()
    s = N.StringsC(C.cast(blob, C.c_void_p).value, 0, 0, 8, 0)
    counts = (C.c_uint32 * 4)()
    assert _call(C.byref(s), C.byref(s), 1, counts=C.cast(counts, C.c_void_p)) == N.TA_ERR_HIP
    assert _call(C.byref(s), C.byref(s), 1, st=0, counts=C.cast(counts, C.c_void_p), cap=0) == N.TA_ERR_HIP
