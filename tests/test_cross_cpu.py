"""not-gpu: the cross body (lev_cross_body.h) under host emulation -- a wavefront of 64 emulated lanes runs ONE query against up to 64
targets, with one and two table words per row, under Levenshtein and restricted Damerau, and every lane's answer is compared with the
oracle's levenshtein_simd_k_with_opts (None = TA_NONE); the length prefilter's report; the table left zero after every query; plus
the argument errors of ta_levenshtein_cross and its refusal to run without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_cross")
NONE = 0xFFFFFFFF
COSTS = (O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS)
QUERY_LENS = (0, 1, 2, 31, 32, 33, 63, 64)
TARGET_LENS = (0, 1, 31, 32, 33, 63, 64, 65, 100)
ALPHABETS = {
    "acgt": np.frombuffer(b"ACGT", np.uint8),
    "1..255": np.arange(1, 256, dtype=np.uint8),
    "nul": np.array([0], np.uint8),
    "nul+0c": np.array([0x00, 0x0C], np.uint8),
    "0..255": np.arange(0, 256, dtype=np.uint8),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(EMU_DIR, "libta_emu_cross.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        _lib.emu_cross_query.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p]
        _lib.emu_cross_query.restype = C.c_int
        _lib.emu_cross_table_clean.argtypes = [C.c_int]
        _lib.emu_cross_table_clean.restype = C.c_int
    return _lib


def emu(query, targets, k, nw, trans):
    """-> (the answers of the len(targets) live lanes, their skip flags, whether the body ran the query)"""
    assert len(targets) <= 64
    off = np.zeros(len(targets) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in targets])
    blob = np.frombuffer(b"".join(targets) + b"\xa5" * 16, np.uint8).copy()      # (the blobs' read slack)
    res, skip = np.zeros(64, np.uint32), np.zeros(64, np.uint32)
    ran = lib().emu_cross_query(bytes(query) + b"\xa5" * 16, len(query), blob.ctypes.data, off.ctypes.data, len(targets), k, nw, int(trans),
                                res.ctypes.data, skip.ctypes.data)
    assert ran in (0, 1), (len(query), nw)
    assert lib().emu_cross_table_clean(nw) == 1, "a query left bits in the table"
    n = len(targets)
    assert (res[n:] == NONE).all() and not skip[n:].any()                          # lanes without a target
    return [int(x) for x in res[:n]], [bool(x) for x in skip[:n]], bool(ran)


def check(query, targets, ks, memo=None):
    """every lane, both cost families, every table width the query fits, against the oracle; the prefilter's report"""
    m = len(query)
    memo = {} if memo is None else memo
    for costs in COSTS:
        trans = costs[3] is not None
        for k in ks:
            want = []
            for t in targets:
                key = (query, t, k, trans)
                if key not in memo:
                    d = O.levenshtein_simd_k_with_opts(query, t, k, False, costs)[0]
                    memo[key] = NONE if d is None else d
                want.append(memo[key])
            outside = [abs(m - len(t)) > k for t in targets]
            for nw in (1, 2):
                if m > 32 * nw:
                    continue
                got, skip, ran = emu(query, targets, k, nw, trans)
                assert got == want, (m, [len(t) for t in targets], k, nw, trans, query[:40])
                assert skip == outside, (m, k, nw)                                 # a pair outside the length bound is reported as skipped ...
                assert all(g == NONE for g, o in zip(got, outside) if o)           # ... and is None
                assert ran == (not all(outside)), (m, k, nw)                       # a query no lane can match costs nothing


def ks_of(m, targets):
    lens = [len(t) for t in targets] or [0]
    return sorted({0, 1, 2, m // 2, m, m + lens[0], m + max(lens), 0xFFFFFFFF})


def rand(g, alphabet, n):
    return bytes(g.choice(alphabet, n)) if n else b""


def mixed_lengths(g, count=64):
    lens = list(TARGET_LENS) + [int(x) for x in g.integers(0, 101, size=count - len(TARGET_LENS))]
    g.shuffle(lens)
    return lens


@pytest.mark.parametrize("name", list(ALPHABETS))
def test_random_pairs_every_query_length(name):
    g = Dg.rng(5101 + len(name))
    alphabet = ALPHABETS[name]
    for m in QUERY_LENS:
        query = rand(g, alphabet, m)
        targets = [rand(g, alphabet, n) for n in mixed_lengths(g)]
        check(query, targets, ks_of(m, targets))


@pytest.mark.parametrize("name", ["acgt", "1..255", "0..255"])
def test_mutated_targets_hits_at_every_small_distance(name):
    g = Dg.rng(5201 + len(name))
    alphabet = ALPHABETS[name]
    for m in QUERY_LENS:
        query = rand(g, alphabet, m)
        targets = [Dg.mutate(g, query, e, swaps=True) for e in range(5) for _ in range(12)]
        targets += [query, query[::-1], query[1:], query + query[:1]]
        memo = {}
        check(query, targets, sorted(set(ks_of(m, targets)) | {4}), memo)
        if m >= 2:
            # hits exist at every small distance, and the transposition term is exercised: a swap costs 2 without it, 1 with it
            dists = {memo[(query, t, 4, False)] for t in targets}
            assert {0, 1, 2} <= dists, dists
            sw = bytes([query[1], query[0]]) + query[2:]
            if sw != query:
                check(query, [sw], [1, 2])
                assert emu(query, [sw], 2, 2, True)[0] == [1] and emu(query, [sw], 2, 2, False)[0] == [2]


def test_two_symbol_and_one_symbol_alphabets_mutated():
    g = Dg.rng(5301)
    for name in ("nul", "nul+0c"):
        alphabet = ALPHABETS[name]
        for m in QUERY_LENS:
            query = rand(g, alphabet, m)
            targets = []
            for e in range(5):
                for _ in range(6):
                    s = bytearray(query)
                    for _ in range(e):                                              # edits that stay inside the alphabet
                        kind = int(g.integers(0, 3))
                        if kind == 0 and s:
                            s[int(g.integers(len(s)))] = int(g.choice(alphabet))
                        elif kind == 1:
                            s.insert(int(g.integers(len(s) + 1)), int(g.choice(alphabet)))
                        elif s:
                            del s[int(g.integers(len(s)))]
                    targets.append(bytes(s))
            check(query, targets, ks_of(m, targets))


def test_fewer_than_64_targets_and_none():
    g = Dg.rng(5401)
    alphabet = ALPHABETS["acgt"]
    for nt in (0, 1, 2, 33, 63, 64):
        for m in (0, 5, 40):
            query = rand(g, alphabet, m)
            targets = [rand(g, alphabet, int(g.integers(0, 50))) for _ in range(nt)]
            check(query, targets, [0, 3, 50])


def test_prefilter_skips_pairs_outside_the_length_bound():
    query = b"ACGTACGTAC"                                                           # m = 10
    near, far = b"ACGTACGTAC", b"A" * 30
    got, skip, ran = emu(query, [near, far, b"", b"ACGTACGT"], 2, 1, False)
    assert skip == [False, True, True, False] and got == [0, NONE, NONE, 2] and ran
    got, skip, ran = emu(query, [far, b"", b"AC"], 2, 1, False)                    # every live lane outside: the query is not run
    assert skip == [True, True, True] and got == [NONE] * 3 and not ran
    got, skip, ran = emu(b"", [b"", b"AB", b"ABC"], 2, 1, True)                    # the empty query answers len(t) without the loop
    assert skip == [False, False, True] and got == [0, 2, NONE] and ran
    got, skip, ran = emu(query, [b""], 10, 2, True)                                # the empty target answers m
    assert skip == [False] and got == [10] and ran


# ---------------------------------------------------------------- the C ABI: argument errors come first, no CPU fallback
def _abi():
    from triple_accel_amd import _native as N
    return N


def _costs(c):
    N = _abi()
    return N.EditCostsC(c[0], c[1], c[2], 0 if c[3] is None else 1, 0 if c[3] is None else c[3])


def _call(queries, nq, targets, nt, k=1, costs=O.LEVENSHTEIN_COSTS, hits=None, count=None, cap=0, nearest=None):
    cs = None if costs is None else C.byref(_costs(costs))
    return _abi().lib().ta_levenshtein_cross(queries, nq, targets, nt, k, cs, hits, count, cap, nearest, None)


def test_abi_symbol_is_declared_and_exported():
    N = _abi()
    assert "ta_levenshtein_cross" in N.ABI_SYMBOLS and hasattr(N.lib(), "ta_levenshtein_cross")
    assert C.sizeof(N.CrossHitC) == 16


def test_abi_argument_errors():
    N = _abi()
    blob = (C.c_uint8 * 64)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 0, 8, 0)
    fake = C.c_void_p(0x1000)
    S = C.byref(s)
    assert _call(None, 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, None, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, costs=None, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=None) == N.TA_ERR_ARG                               # count_dev is required ...
    assert _call(S, 0, S, 0, count=None) == N.TA_ERR_ARG                               # ... whatever the sizes
    noblob = N.StringsC(0, 0, 0, 8, 0)
    assert _call(C.byref(noblob), 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, C.byref(noblob), 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=fake, cap=4, hits=None) == N.TA_ERR_ARG
    assert _call(S, 1 << 32, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1 << 32, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=fake, cap=1 << 60, hits=fake) == N.TA_ERR_ARG       # cap * sizeof(ta_cross_hit) overflows


def test_abi_unsupported_and_bad_costs():
    N = _abi()
    blob = (C.c_uint8 * 128)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 0, 8, 0)
    S = C.byref(s)
    fake = C.c_void_p(0x1000)
    for costs in ((1, 1, 1, None), (2, 1, 0, None), (1, 2, 0, None), (2, 2, 0, 3), (2, 2, 0, 1), (3, 3, 2, 3)):
        assert O.costs_valid(costs), costs
        assert _call(S, 1, S, 1, costs=costs, count=fake) == N.TA_ERR_UNSUPPORTED, costs
    for costs in ((1, 0, 0, None), (0, 1, 0, None), (1, 1, 0, 0), (2, 1, 0, 5)):
        assert not O.costs_valid(costs), costs
        assert _call(S, 1, S, 1, costs=costs, count=fake) == N.TA_ERR_BAD_COSTS, costs
    long_query = N.StringsC(ptr, 0, 65, 65, 0)
    assert _call(C.byref(long_query), 1, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED
    long_csr_query = N.StringsC(ptr, 0x1000, 0, 0, 65)
    assert _call(C.byref(long_csr_query), 1, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED
    huge_target = N.StringsC(ptr, 0, 1 << 32, 1 << 32, 0)
    assert _call(S, 1, C.byref(huge_target), 1, count=fake) == N.TA_ERR_UNSUPPORTED
    huge_csr_target = N.StringsC(ptr, 0x1000, 0, 0, 1 << 32)
    assert _call(S, 1, C.byref(huge_csr_target), 1, count=fake) == N.TA_ERR_UNSUPPORTED


def test_no_cpu_fallback():
    import torch
    N = _abi()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    blob = (C.c_uint8 * 64)()
    s = N.StringsC(C.cast(blob, C.c_void_p).value, 0, 0, 8, 0)
    count = (C.c_uint64 * 1)()
    for costs in (O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS, (3, 3, 0, None), (2, 2, 0, 2)):
        assert _call(C.byref(s), 1, C.byref(s), 1, costs=costs, count=C.cast(count, C.c_void_p)) == N.TA_ERR_HIP
    assert _call(C.byref(s), 0, C.byref(s), 4, count=C.cast(count, C.c_void_p)) == N.TA_ERR_HIP   # the count is zeroed on the device
