"""not-gpu: the token cross body (lev_cross_tok_body.h) under host emulation -- a wavefront of 64 emulated lanes runs ONE query of 32-bit
tokens against up to 64 targets, with one and two mask words per slot, under Levenshtein and restricted Damerau, and every lane's answer
is compared with the C oracle over byte codes of the same pairs (cross_tokens_cases.dists); the length prefilter's report; the hash table
left all zero after every query; vocabularies that stress the 32-bit compare; queries built to collide in the table (with the body's own
home-slot function); parity with the byte body on byte-valued tokens; plus the argument errors of ta_levenshtein_cross_tokens and its
refusal to run without a device.

The target items are handed over in an array of exactly their size: the body may read nothing else."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cross_tokens_cases as X
import datagen as Dg
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
NONE = X.NONE
QUERY_LENS = (0, 1, 2, 31, 32, 33, 63, 64)
TARGET_LENS = (0, 1, 31, 32, 33, 63, 64, 65, 100)


def emu(query, targets, k, nw, trans):
    """-> (the answers of the len(targets) live lanes, their skip flags, whether the body ran the query)"""
    assert len(targets) <= 64
    off = np.zeros(len(targets) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in targets])
    data = np.array([x for t in targets for x in t], dtype=np.uint32)              # no slack: exactly the items
    q = np.array(query, dtype=np.uint32)
    res, skip = np.zeros(64, np.uint32), np.zeros(64, np.uint32)
    lib = X.emu_lib()
    ran = lib.emu_cross_tok_query(q.ctypes.data, len(q), data.ctypes.data, off.ctypes.data, len(targets), k, nw, int(trans),
                                  res.ctypes.data, skip.ctypes.data)
    assert ran in (0, 1), (len(query), nw)
    assert lib.emu_cross_tok_table_clean(nw) == 1, "a query left something in the table"
    n = len(targets)
    assert (res[n:] == NONE).all() and not skip[n:].any()                          # lanes without a target
    return [int(x) for x in res[:n]], [bool(x) for x in skip[:n]], bool(ran)


def check(query, targets, ks):
    """every lane, both cost families, every table width the query fits, against the oracle; the prefilter's report"""
    m = len(query)
    for costs in X.COSTS:
        trans = costs[3] is not None
        for k in ks:
            want = [int(x) for x in X.dists([query], targets, k, costs)[0]] if targets else []
            outside = [abs(m - len(t)) > k for t in targets]
            for nw in (1, 2):
                if m > 32 * nw:
                    continue
                got, skip, ran = emu(query, targets, k, nw, trans)
                assert got == want, (m, [len(t) for t in targets], k, nw, trans, query[:8])
                assert skip == outside, (m, k, nw)                                 # a pair outside the length bound is reported as skipped ...
                assert all(g == NONE for g, o in zip(got, outside) if o)           # ... and is None
                assert ran == (not all(outside)), (m, k, nw)                       # a query no lane can match costs nothing


def ks_of(m, targets):
    longest = max([len(t) for t in targets] or [0])
    return sorted({0, 1, 2, m // 2, m, m + longest, 0xFFFFFFFF})


def mixed_lengths(g, count=64):
    lens = list(TARGET_LENS) + [int(x) for x in g.integers(0, 101, size=count - len(TARGET_LENS))]
    g.shuffle(lens)
    return lens


@pytest.mark.parametrize("name", X.VOCABS)
def test_random_pairs_every_query_length(name):
    g = Dg.rng(7101 + len(name))
    voc = X.vocab(name)
    for m in QUERY_LENS:
        query = X.rand_seq(g, voc, m)
        targets = [X.rand_seq(g, voc, n) for n in mixed_lengths(g)]
        check(query, targets, ks_of(m, targets))


@pytest.mark.parametrize("name", X.VOCABS)
def test_mutated_targets_hits_at_every_small_distance(name):
    g = Dg.rng(7201 + len(name))
    voc = X.vocab(name)
    for m in QUERY_LENS:
        query = X.rand_seq(g, voc, m)
        targets = [X.edited(g, query, e, voc) for e in range(5) for _ in range(11)]
        targets += [query, query[::-1], query[1:], query + query[:1]]
        targets += [X.rand_seq(g, voc, n) for n in (0, 1, 2, 3, 5, 6, 7)][:64 - len(targets)]   # the fetch's short and tail forms
        check(query, targets, sorted(set(ks_of(m, targets)) | {4}))
        if m >= 2 and len(voc) >= 48:
            # hits exist at every small distance, and the transposition term is exercised: a swap costs 2 without it, 1 with it
            d = X.dists([query], targets, 4, O.LEVENSHTEIN_COSTS)[0]
            assert {0, 1, 2} <= {int(x) for x in d}, d
            sw = (query[1], query[0]) + query[2:]
            if sw != query:
                assert emu(query, [sw], 2, 2, True)[0] == [1] and emu(query, [sw], 2, 2, False)[0] == [2]


def test_fewer_than_64_targets_and_none():
    g = Dg.rng(7401)
    voc = X.vocab("32k")
    for nt in (0, 1, 2, 33, 63, 64):
        for m in (0, 5, 40):
            query = X.rand_seq(g, voc[:6], m)
            targets = [X.rand_seq(g, voc[:6], int(g.integers(0, 50))) for _ in range(nt)]
            check(query, targets, [0, 3, 50])


def test_prefilter_skips_pairs_outside_the_length_bound():
    a, c, g_, t = X.vocab("32k")[:4]
    query = (a, c, g_, t, a, c, g_, t, a, c)                                        # m = 10
    near, far = query, (a,) * 30
    got, skip, ran = emu(query, [near, far, (), query[:8]], 2, 1, False)
    assert skip == [False, True, True, False] and got == [0, NONE, NONE, 2] and ran
    got, skip, ran = emu(query, [far, (), (a, c)], 2, 1, False)                     # every live lane outside: the query is not run
    assert skip == [True, True, True] and got == [NONE] * 3 and not ran
    got, skip, ran = emu((), [(), (a, c), (a, c, g_)], 2, 1, True)                  # the empty query answers len(t) without the loop
    assert skip == [False, False, True] and got == [0, 2, NONE] and ran
    got, skip, ran = emu(query, [()], 10, 2, True)                                 # the empty target answers m
    assert skip == [False] and got == [10] and ran


# ---------------------------------------------------------------- queries that collide in the table
def test_collision_a_64_distinct_tokens_on_one_home_slot():
    query, targets = X.case_longest_chain()
    assert len(set(query)) == 64 and len(set(int(h) for h in X.homes(query))) == 1      # the longest chain there is
    check(query, targets, [0, 1, 2, 5, 64, 0xFFFFFFFF])
    assert emu(query, [query], 0, 2, False)[0] == [0]


def test_collision_b_two_tokens_on_one_home_slot():
    query, targets = X.case_two_on_one_slot()
    h = X.homes(query)
    assert query[0] != query[1] and h[0] == h[1]
    check(query, targets, [0, 1, 2, 3, 20])
    a, b = query[:2]
    assert emu(query, [(b, a) + query[2:]], 2, 1, False)[0] == [2]                 # the two are told apart: a swap is two substitutions


def test_collision_c_absent_items_that_start_at_a_taken_slot():
    query, targets, planted = X.case_absent_items_on_taken_slots()
    for t, e in zip(targets, planted):                                             # the preconditions, by the body's own function
        diff = [i for i in range(len(query)) if t[i] != query[i]]
        assert len(diff) == e and all(t[i] not in query for i in diff)
        assert all(X.homes([t[i]])[0] == X.homes([query[i]])[0] for i in diff)
    m = len(query)
    check(query, targets, [0, 1, 2, 3, m // 2, m])
    for nw in (1, 2):
        for trans in (False, True):
            got = emu(query, targets, m, nw, trans)[0]
            assert got == planted, (nw, trans, got)                                # a lookup without the key compare answers 0 everywhere
            assert emu(query, targets, 0, nw, trans)[0] == [NONE] * len(targets)


def test_collision_d_a_repeated_token_in_lanes_32_and_above():
    query, targets = X.case_duplicates_in_the_second_word()
    check(query, targets, [0, 1, 2, 3, 4, 64])
    z, y = query[5], query[45]
    got = emu(query, [(z,) * 3, (y,) * 2, query], 64, 2, False)[0]
    assert got == [61, 62, 0]                                                      # every row that holds the token matches it


# ---------------------------------------------------------------- byte-valued tokens: the byte body's answers
_byte_lib = None


def byte_emu(query, targets, k, nw, trans):
    global _byte_lib
    if _byte_lib is None:
        d = os.path.join(HERE, "emu_cross")
        path = os.path.join(d, "libta_emu_cross.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", d, "-s"])
        _byte_lib = C.CDLL(path)
        _byte_lib.emu_cross_query.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                              C.c_void_p, C.c_void_p]
        _byte_lib.emu_cross_query.restype = C.c_int
    off = np.zeros(len(targets) + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in targets])
    blob = np.frombuffer(b"".join(targets) + b"\xa5" * 16, np.uint8).copy()
    res, skip = np.zeros(64, np.uint32), np.zeros(64, np.uint32)
    ran = _byte_lib.emu_cross_query(bytes(query) + b"\xa5" * 16, len(query), blob.ctypes.data, off.ctypes.data, len(targets), k, nw, int(trans),
                                    res.ctypes.data, skip.ctypes.data)
    n = len(targets)
    return [int(x) for x in res[:n]], [bool(x) for x in skip[:n]], bool(ran)


def test_byte_valued_tokens_equal_the_byte_body():
    g = Dg.rng(7501)
    voc = X.vocab("bytes")
    for m in QUERY_LENS:
        query = X.rand_seq(g, voc[:20], m)
        targets = [X.edited(g, query, int(g.integers(0, 6)), voc[:20]) for _ in range(40)] + [X.rand_seq(g, voc, n) for n in mixed_lengths(g, 24)]
        for k in ks_of(m, targets):
            for nw in (1, 2):
                if m > 32 * nw:
                    continue
                for trans in (False, True):
                    assert emu(query, targets, k, nw, trans) == byte_emu(bytes(query), [bytes(t) for t in targets], k, nw, trans), (m, k, nw, trans)


# ---------------------------------------------------------------- the C ABI: argument errors come first, no CPU fallback
def _abi():
    from triple_accel_amd import _native as N
    return N


def _costs(c):
    N = _abi()
    return N.EditCostsC(c[0], c[1], c[2], 0 if c[3] is None else 1, 0 if c[3] is None else c[3])


def _call(queries, nq, targets, nt, k=1, costs=O.LEVENSHTEIN_COSTS, flags=0, hits=None, count=None, cap=0, nearest=None, per_query=None):
    cs = None if costs is None else C.byref(_costs(costs))
    return _abi().lib().ta_levenshtein_cross_tokens(queries, nq, targets, nt, k, cs, flags, hits, count, cap, nearest, per_query, None)


def _sides():
    N = _abi()
    data = (C.c_uint32 * 256)()
    ptr = C.cast(data, C.c_void_p).value
    return data, ptr, N.TokensC(ptr, 0, 8, 8, 0)


def test_abi_symbol_is_declared_and_exported():
    N = _abi()
    assert "ta_levenshtein_cross_tokens" in N.ABI_SYMBOLS and hasattr(N.lib(), "ta_levenshtein_cross_tokens")
    header = open(os.path.join(os.path.dirname(HERE), "include", "triple_accel_amd.h")).read()
    assert "int ta_levenshtein_cross_tokens(const ta_tokens *queries, size_t nq, const ta_tokens *targets, size_t nt," in header


def test_abi_argument_errors_in_their_order():
    N = _abi()
    keep, ptr, s = _sides()
    S = C.byref(s)
    fake = C.c_void_p(0x1000)
    bad_costs, weighted = (1, 0, 0, None), (2, 1, 0, None)
    # NULL pointers first, whatever else is wrong
    assert _call(None, 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, None, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, costs=None, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=None) == N.TA_ERR_ARG                               # count_dev is required ...
    assert _call(S, 0, S, 0, count=None, costs=bad_costs) == N.TA_ERR_ARG              # ... whatever the sizes and the costs
    # then the flags: only TA_CROSS_UPPER is known
    for flags in (2, 4, 0x80000000, 3):
        assert _call(S, 1, S, 1, flags=flags, count=fake, costs=bad_costs) == N.TA_ERR_ARG, flags
    # then the costs, in front of the counts and the blobs
    assert _call(S, 1 << 32, S, 1, count=fake, costs=bad_costs) == N.TA_ERR_BAD_COSTS
    assert _call(S, 1 << 32, S, 1, count=fake, costs=weighted) == N.TA_ERR_UNSUPPORTED
    # then the counts, NULL data, cap with NULL hits, cap overflow -- in front of the length bounds
    long_q = N.TokensC(ptr, 0, 65, 65, 0)
    LQ = C.byref(long_q)
    nodata = N.TokensC(0, 0, 8, 8, 0)
    assert _call(LQ, 1 << 32, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(LQ, 1, S, 1 << 32, count=fake) == N.TA_ERR_ARG
    assert _call(LQ, 1, C.byref(nodata), 1, count=fake) == N.TA_ERR_ARG
    assert _call(C.byref(nodata), 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert b"null data" in N.lib().ta_last_error()
    assert _call(LQ, 1, S, 1, count=fake, cap=4, hits=None) == N.TA_ERR_ARG
    assert _call(LQ, 1, S, 1, count=fake, cap=1 << 60, hits=fake) == N.TA_ERR_ARG      # cap * sizeof(ta_cross_hit) overflows


def test_abi_unsupported_and_bad_costs():
    N = _abi()
    keep, ptr, s = _sides()
    S = C.byref(s)
    fake = C.c_void_p(0x1000)
    for costs in ((1, 1, 1, None), (2, 1, 0, None), (1, 2, 0, None), (2, 2, 0, 3), (2, 2, 0, 1), (3, 3, 2, 3)):
        assert O.costs_valid(costs), costs
        assert _call(S, 1, S, 1, costs=costs, count=fake) == N.TA_ERR_UNSUPPORTED, costs
    for costs in ((1, 0, 0, None), (0, 1, 0, None), (1, 1, 0, 0), (2, 1, 0, 5)):
        assert not O.costs_valid(costs), costs
        assert _call(S, 1, S, 1, costs=costs, count=fake) == N.TA_ERR_BAD_COSTS, costs
    # a bound of 65 tokens, strided and CSR (max_len given): unsupported, and the message names the limit
    for long_query in (N.TokensC(ptr, 0, 65, 65, 0), N.TokensC(ptr, 0, 100, 65, 0), N.TokensC(ptr, 0x1000, 0, 0, 65), N.TokensC(ptr, 0x1000, 0, 9, 65)):
        assert _call(C.byref(long_query), 1, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED
        assert b"64 tokens" in N.lib().ta_last_error()
    # 64 is fine and the CSR field `len` plays no part: the next stop is the device (asked only where there is none -- the pointers are fake)
    if not _gpu():
        for ok_query in (N.TokensC(ptr, 0, 64, 64, 0), N.TokensC(ptr, 0x1000, 0, 1 << 40, 64)):
            assert _call(C.byref(ok_query), 1, S, 1, count=fake) == N.TA_ERR_HIP
    huge_target = N.TokensC(ptr, 0, 1 << 32, 1 << 32, 0)
    assert _call(S, 1, C.byref(huge_target), 1, count=fake) == N.TA_ERR_UNSUPPORTED
    huge_csr_target = N.TokensC(ptr, 0x1000, 0, 0, 1 << 32)
    assert _call(S, 1, C.byref(huge_csr_target), 1, count=fake) == N.TA_ERR_UNSUPPORTED


def _gpu():
    import torch
    return torch.cuda.is_available()


def test_no_cpu_fallback():
    N = _abi()
    if _gpu():
        pytest.skip("GPU present")
    keep, ptr, s = _sides()
    count = (C.c_uint64 * 1)()
    cnt = C.cast(count, C.c_void_p)
    for costs in (O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS, (3, 3, 0, None), (2, 2, 0, 2)):
        assert _call(C.byref(s), 1, C.byref(s), 1, costs=costs, count=cnt) == N.TA_ERR_HIP
    assert _call(C.byref(s), 1, C.byref(s), 1, flags=N.TA_CROSS_UPPER, count=cnt) == N.TA_ERR_HIP
    assert _call(C.byref(s), 0, C.byref(s), 4, count=cnt) == N.TA_ERR_HIP            # the count is zeroed on the device
    csr = N.TokensC(ptr, 0x1000, 0, 0, 0)                                          # max_len to be measured: still no device
    assert _call(C.byref(csr), 1, C.byref(s), 1, count=cnt) == N.TA_ERR_HIP
