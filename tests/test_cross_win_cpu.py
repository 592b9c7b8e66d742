"""not-gpu: the window cross body (lev_cross_win_body.h) under host emulation -- a wavefront of 64 emulated lanes runs ONE query of up
to 256 bytes against up to 64 targets with a window of WW blocks of the column, for every WW that suffices for the threshold, under
Levenshtein and restricted Damerau, and every lane's answer is compared with the oracle's levenshtein_simd_k_with_opts (None =
TA_NONE); the length prefilter's report; the table left zero after every query; plus the argument errors of
ta_levenshtein_cross_with_opts and its refusal to run without a device.

Every (query length, k, cost family) group has to show something: over its alphabets the oracle finds at least 16 hits, at least one
of them at distance exactly k, and at least 16 non-hits pass the length prefilter.  Two of the three cannot hold at k = 2^32 - 1 (no
string is that long: every pair is a hit, none at distance k), so that k asserts the first one only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_cross_win")
NONE = 0xFFFFFFFF
KMAX = 0xFFFFFFFF
COSTS = (O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS)
QUERY_LENS = (1, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256)
KS = (0, 1, 8, 9, 24, 25, 40, 41, 300, KMAX)                                       # every WW and both sides of each switch
WWS = (2, 3, 4, 8)
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
        path = os.path.join(EMU_DIR, "libta_emu_cross_win.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        _lib.emu_cross_win_query.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p]
        _lib.emu_cross_win_query.restype = C.c_int
        _lib.emu_cross_win_ww.argtypes = [C.c_uint32]
        _lib.emu_cross_win_ww.restype = C.c_int
        _lib.emu_cross_win_table_clean.argtypes = []
        _lib.emu_cross_win_table_clean.restype = C.c_int
    return _lib


def widths(k):
    """every instantiated window that suffices for k, the entry's own choice first"""
    first = lib().emu_cross_win_ww(k)
    return [ww for ww in WWS if ww >= first]


def emu(query, targets, k, ww, trans):
    """-> (the answers of the len(targets) live lanes, their skip flags, whether the body ran the query)"""
    assert len(targets) <= 64
    off = np.zeros(len(targets) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in targets])
    blob = np.frombuffer(b"".join(targets) + b"\xa5" * 16, np.uint8).copy()      # (the blobs' read slack)
    res, skip = np.zeros(64, np.uint32), np.zeros(64, np.uint32)
    ran = lib().emu_cross_win_query(bytes(query) + b"\xa5" * 16, len(query), blob.ctypes.data, off.ctypes.data, len(targets), k, ww,
                                    int(trans), res.ctypes.data, skip.ctypes.data)
    assert ran in (0, 1), (len(query), k, ww)
    assert lib().emu_cross_win_table_clean() == 1, "a query left bits in the table"
    n = len(targets)
    assert (res[n:] == NONE).all() and not skip[n:].any()                          # lanes without a target
    return [int(x) for x in res[:n]], [bool(x) for x in skip[:n]], bool(ran)


def oracle(query, targets, k, costs):
    out = []
    for t in targets:
        d = O.levenshtein_simd_k_with_opts(query, t, k, False, costs)[0]
        out.append(NONE if d is None else d)
    return out


def check(query, targets, k, costs):
    """every lane at every window that suffices against the oracle; the prefilter's report -> the oracle's answers"""
    m, trans = len(query), costs[3] is not None
    want = oracle(query, targets, k, costs)
    outside = [abs(m - len(t)) > k for t in targets]
    for ww in widths(k):
        got, skip, ran = emu(query, targets, k, ww, trans)
        bad = [(i, len(targets[i]), got[i], want[i]) for i in range(len(targets)) if got[i] != want[i]]
        assert not bad, (m, k, ww, trans, bad[:4])
        assert skip == outside, (m, k, ww)                                         # a pair outside the length bound is reported as skipped ...
        assert all(g == NONE for g, o in zip(got, outside) if o)                   # ... and is None
        assert ran == (not all(outside)), (m, k, ww)                               # a query no lane can match costs nothing
    return want, outside


def rand(g, alphabet, n):
    return bytes(g.choice(alphabet, n)) if n else b""


def edited(g, query, alphabet, e):
    """the query after e random substitutions, insertions, deletions and adjacent swaps inside the alphabet"""
    s = bytearray(query)
    for _ in range(e):
        kind = int(g.integers(0, 4))
        if kind == 0 and s:
            s[int(g.integers(len(s)))] = int(g.choice(alphabet))
        elif kind == 1:
            s.insert(int(g.integers(len(s) + 1)), int(g.choice(alphabet)))
        elif kind == 2 and s:
            del s[int(g.integers(len(s)))]
        elif kind == 3 and len(s) > 1:
            p = int(g.integers(len(s) - 1))
            s[p], s[p + 1] = s[p + 1], s[p]
    return bytes(s)


def targets_for(g, query, alphabet, k):
    """64 targets: random ones of lengths m - k - 1 .. m + k + 1 (the string lengths kept below 600), copies of the query with 0 .. k + 2
    edits, and, where the alphabet has symbols the query does not use, planted ones: at distance exactly k, and just too far"""
    m, kk = len(query), min(k, 300)
    lo, hi = max(0, m - kk - 1), m + kk + 1
    lens = [lo, hi, max(0, m - kk), m + kk] + [int(x) for x in g.integers(lo, hi + 1, size=12)]
    out = [rand(g, alphabet, n) for n in lens]
    unused = np.array(sorted(set(int(x) for x in alphabet) - set(query)), np.uint8)
    if len(unused) and k != KMAX:
        for _ in range(8):
            if k >= m:                                                             # no symbol in common: the distance is the longer length
                out.append(rand(g, unused, k) if k else query)
            else:                                                                  # k symbols replaced by ones the query lacks: exactly k
                s = bytearray(query)
                for p in g.choice(m, k, replace=False):
                    s[int(p)] = int(g.choice(unused))
                out.append(bytes(s))
            out.append(rand(g, unused, int(g.integers(max(k + 1, m - k), m + k + 1))))   # inside the length bound, distance = its length > k
    edits = [0, kk, kk + 1, kk + 2] + [int(x) for x in g.integers(0, kk + 3, size=64)]
    for e in edits[:64 - len(out)]:
        out.append(edited(g, query, alphabet, e))
    return out


@pytest.mark.parametrize("m", QUERY_LENS)
def test_every_window_against_the_oracle(m):
    g = Dg.rng(7100 + m)
    queries = {name: rand(g, ALPHABETS[name], m) for name in ALPHABETS}
    for k in KS:
        sets = {name: targets_for(g, queries[name], ALPHABETS[name], k) for name in ALPHABETS}
        for costs in COSTS:
            hits = at_k = near_misses = 0
            for name in ALPHABETS:
                want, outside = check(queries[name], sets[name], k, costs)
                hits += sum(1 for d in want if d != NONE)
                at_k += sum(1 for d in want if d == k)
                near_misses += sum(1 for d, o in zip(want, outside) if d == NONE and not o)
            if k >= 1:                                                             # a group where nothing hits shows nothing
                assert hits >= 16, (m, k, costs, hits)
                if k != KMAX:
                    assert at_k >= 1, (m, k, costs)
                    assert near_misses >= 16, (m, k, costs, near_misses)


def test_the_transposition_term_across_a_block_edge():
    g = Dg.rng(7201)
    for m in (65, 97, 130, 256):
        query = bytearray(rand(g, ALPHABETS["1..255"], m))
        for p in (31, 63, 95, 127, m - 2):                                         # the swapped rows straddle two table words
            if p + 1 >= m:
                continue
            query[p], query[p + 1] = 1, 2
            sw = bytearray(query)
            sw[p], sw[p + 1] = 2, 1
            for ww in WWS:
                assert emu(bytes(query), [bytes(sw)], 2, ww, True)[0] == [1], (m, p, ww)
                assert emu(bytes(query), [bytes(sw)], 2, ww, False)[0] == [2], (m, p, ww)


def test_fewer_than_64_targets_and_short_queries_in_the_window_body():
    g = Dg.rng(7301)
    alphabet = ALPHABETS["acgt"]
    for nt in (0, 1, 33, 64):
        for m in (0, 5, 40, 150):                                                  # (a CSR batch mixes short queries in)
            query = rand(g, alphabet, m)
            targets = [edited(g, query, alphabet, int(g.integers(0, 12))) for _ in range(nt)]
            for k in (0, 3, 9, 50):
                for costs in COSTS:
                    check(query, targets, k, costs)


def test_prefilter_skips_pairs_outside_the_length_bound():
    query = b"ACGT" * 25                                                            # m = 100
    got, skip, ran = emu(query, [query, b"A" * 130, b"", query[:98]], 2, 2, False)
    assert skip == [False, True, True, False] and got == [0, NONE, NONE, 2] and ran
    got, skip, ran = emu(query, [b"A" * 130, b"", b"AC"], 2, 2, False)             # every live lane outside: the query is not run
    assert skip == [True, True, True] and got == [NONE] * 3 and not ran
    got, skip, ran = emu(query, [b""], 100, 8, True)                               # the empty target answers m
    assert skip == [False] and got == [100] and ran


def test_window_choice():
    assert [lib().emu_cross_win_ww(k) for k in (0, 8, 9, 24, 25, 40, 41, 300, KMAX)] == [2, 2, 3, 3, 4, 4, 8, 8, 8]
    got = np.zeros(64, np.uint32)
    assert lib().emu_cross_win_query(b"A" * 32, 16, None, None, 0, 9, 2, 0, got.ctypes.data, got.ctypes.data) == -1   # too narrow for k


# ---------------------------------------------------------------- the C ABI: argument errors come first, no CPU fallback
def _abi():
    from triple_accel_amd import _native as N
    return N


def _costs(c):
    N = _abi()
    return N.EditCostsC(c[0], c[1], c[2], 0 if c[3] is None else 1, 0 if c[3] is None else c[3])


def _call(queries, nq, targets, nt, k=1, costs=O.LEVENSHTEIN_COSTS, flags=0, hits=None, count=None, cap=0, nearest=None, per_query=None):
    cs = None if costs is None else C.byref(_costs(costs))
    return _abi().lib().ta_levenshtein_cross_with_opts(queries, nq, targets, nt, k, cs, flags, hits, count, cap, nearest, per_query, None)


def test_abi_symbol_is_declared_and_exported():
    N = _abi()
    assert "ta_levenshtein_cross_with_opts" in N.ABI_SYMBOLS and hasattr(N.lib(), "ta_levenshtein_cross_with_opts")


def test_abi_argument_errors():
    """every one of these comes before any device work: the pointers are not device memory"""
    N = _abi()
    blob = (C.c_uint8 * 512)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 0, 8, 0)
    fake = C.c_void_p(0x1000)
    S = C.byref(s)
    assert _call(None, 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, None, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, costs=None, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=None) == N.TA_ERR_ARG
    assert _call(S, 0, S, 0, count=None) == N.TA_ERR_ARG
    for flags in (2, 3, 0x80000000):                                               # TA_CROSS_UPPER is the only flag
        assert _call(S, 1, S, 1, flags=flags, count=fake, per_query=fake) == N.TA_ERR_ARG, flags
    noblob = N.StringsC(0, 0, 0, 8, 0)
    assert _call(C.byref(noblob), 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, C.byref(noblob), 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=fake, cap=4, hits=None) == N.TA_ERR_ARG
    assert _call(S, 1 << 32, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1 << 32, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=fake, cap=1 << 60, hits=fake) == N.TA_ERR_ARG
    for costs in ((1, 1, 1, None), (2, 1, 0, None), (1, 2, 0, None), (2, 2, 0, 3), (2, 2, 0, 1), (3, 3, 2, 3)):   # weighted: not here
        assert O.costs_valid(costs), costs
        assert _call(S, 1, S, 1, costs=costs, count=fake) == N.TA_ERR_UNSUPPORTED, costs
    for costs in ((1, 0, 0, None), (0, 1, 0, None), (1, 1, 0, 0), (2, 1, 0, 5)):
        assert not O.costs_valid(costs), costs
        assert _call(S, 1, S, 1, costs=costs, count=fake) == N.TA_ERR_BAD_COSTS, costs
    long_query = N.StringsC(ptr, 0, 257, 257, 0)
    assert _call(C.byref(long_query), 1, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED
    assert b"256 bytes" in N.lib().ta_last_error()
    long_csr_query = N.StringsC(ptr, 0x1000, 0, 0, 257)
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
    blob = (C.c_uint8 * 512)()
    ptr = C.cast(blob, C.c_void_p).value
    count = C.cast((C.c_uint64 * 1)(), C.c_void_p)
    for length in (8, 65, 256):                                                    # 256 bytes pass the limit: the device is what is missing
        s = N.StringsC(ptr, 0, length, length, 0)
        for costs in (O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS, (3, 3, 0, None), (2, 2, 0, 2)):
            assert _call(C.byref(s), 1, C.byref(s), 1, costs=costs, flags=1, count=count) == N.TA_ERR_HIP
    s = N.StringsC(ptr, 0, 0, 8, 0)
    assert _call(C.byref(s), 0, C.byref(s), 4, count=count) == N.TA_ERR_HIP            # the count is zeroed on the device
