"""not-gpu: the token compaction body (sym_compact_body.h) under host emulation -- for every pair a[i] == b[j] <=> ca[i] == cb[j], and the
overflow list holds exactly the pairs that have no byte coding of this form; plus the int-item oracle (tokens_ref.py) pinned against the
byte oracle on pairs that map to bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import tokens_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_tokens")
SCORE_COSTS = [(1, 1, 0, None), (1, 1, 0, 1), (2, 3, 1, None), (2, 2, 1, 3), (2, 1, 0, None), (1, 2, 0, None), (254, 127, 0, None),
               (254, 127, 255, 253), (3, 2, 0, 2), (1, 127, 7, None), (4, 2, 255, None), (2, 1, 3, 1)]

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(EMU_DIR, "libta_emu_tokens.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
        _lib.emu_sym_compact.argtypes = [vp, vp, u64, u64, vp, vp, u64, u64, u32, u32, u32, vp, vp, vp, C.POINTER(u32)]
    return _lib


def compact(a, b, fixed=False, waves=2):
    """-> (codes of a, codes of b, overflow pair indices) for lists of int sequences"""
    n = len(a)
    if fixed:
        la = len(a[0]) if n else 0
        lb = len(b[0]) if n else 0
        va = np.array(a, dtype=np.int64).reshape(-1).astype(np.uint32)
        vb = np.array(b, dtype=np.int64).reshape(-1).astype(np.uint32)
        oa = ob = None
        offs_a = [i * la for i in range(n + 1)]
        offs_b = [i * lb for i in range(n + 1)]
    else:
        offs_a = np.concatenate([[0], np.cumsum([len(s) for s in a])]).astype(np.uint64)
        offs_b = np.concatenate([[0], np.cumsum([len(s) for s in b])]).astype(np.uint64)
        va = np.array([v for s in a for v in s], dtype=np.int64).astype(np.uint32)
        vb = np.array([v for s in b for v in s], dtype=np.int64).astype(np.uint32)
        oa, ob = offs_a, offs_b
        la = lb = 0
    short = max([min(len(x), len(y)) for x, y in zip(a, b)] + [0])
    cap = 0
    if short > 255:
        cap = 64
        while cap < 2 * short:
            cap *= 2
    ca = np.full(max(int(offs_a[-1]), 1), 0xEE, dtype=np.uint8)
    cb = np.full(max(int(offs_b[-1]), 1), 0xEE, dtype=np.uint8)
    va, vb = np.ascontiguousarray(va) if va.size else np.zeros(1, np.uint32), np.ascontiguousarray(vb) if vb.size else np.zeros(1, np.uint32)
    ovf = np.zeros(max(n, 1), dtype=np.uint32)
    cnt = C.c_uint32()
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)
    lib().emu_sym_compact(p(va), p(oa), la, la, p(vb), p(ob), lb, lb, n, cap, waves, p(ca), p(cb), p(ovf), C.byref(cnt))
    return ([ca[int(offs_a[i]):int(offs_a[i + 1])] for i in range(n)], [cb[int(offs_b[i]):int(offs_b[i + 1])] for i in range(n)],
            sorted(ovf[: cnt.value].tolist()))


def unmappable(x, y):
    """the pair has no coding of the library's form: the shorter side exceeds 255 items and more than 254 distinct items are common"""
    return min(len(x), len(y)) > 255 and len(set(x) & set(y)) > 254


def check(a, b, fixed=False):
    ca, cb, ovf = compact(a, b, fixed)
    assert ovf == [i for i, (x, y) in enumerate(zip(a, b)) if unmappable(x, y)]
    for i, (x, y) in enumerate(zip(a, b)):
        if i in ovf:
            continue
        xa, ya = np.array(x, dtype=np.int64), np.array(y, dtype=np.int64)
        assert len(ca[i]) == len(x) and len(cb[i]) == len(y)
        assert not (ca[i] == 0xEE).any() or 0xEE in np.concatenate([ca[i], cb[i]]).tolist()   # every item written (0xEE may be a code)
        eq = xa[:, None] == ya[None, :]
        ceq = ca[i].astype(np.int64)[:, None] == cb[i].astype(np.int64)[None, :]
        assert np.array_equal(eq, ceq), i


def test_edge_cases():
    M = 0xFFFFFFFF
    a = [[], [1, 2], [], [0, 254, 255, M], [M] * 300, list(range(255)), list(range(256)), [7] * 40, list(range(1000, 1040))]
    b = [[], [], [3], [M, 255, 0, 254, 9], [M] * 260, list(range(255))[::-1], list(range(256))[::-1], [7] * 90, list(range(2000, 2100))]
    check(a, b)
    check(b, a)                                                            # a longer than b and the reverse


def test_254_and_255_common_items():
    rng = np.random.default_rng(1)
    a, b = [], []
    for common in (253, 254, 255, 300):
        base = (rng.permutation(common) * 7919 + 12345).tolist()
        x = base + (np.arange(40) + (1 << 31)).tolist()                    # 40 items of a only
        y = base[::-1] + (np.arange(30) + (3 << 30)).tolist() + [0xFFFFFFFF]
        a.append(x); b.append(y)
    check(a, b)
    _, _, ovf = compact(a, b)
    assert ovf == [2, 3]


def test_random_batches():
    rng = np.random.default_rng(2)
    for vocab, max_len in ((3, 80), (50, 300), (50000, 400), (1 << 32, 300)):
        a = [rng.integers(0, vocab, int(rng.integers(0, max_len + 1)), dtype=np.int64).tolist() for _ in range(10)]
        b = [(x[:] if i % 3 == 0 else rng.integers(0, vocab, int(rng.integers(0, max_len + 1)), dtype=np.int64).tolist())
             for i, x in enumerate(a)]
        check(a, b)


def test_fixed_batches():
    rng = np.random.default_rng(3)
    for L in (64, 255, 256, 320):
        a = rng.permutation(1 << 20)[: 6 * L].reshape(6, L).tolist()
        b = [list(reversed(x)) if i % 2 else rng.integers(0, 10, L).tolist() for i, x in enumerate(a)]
        check(a, b, fixed=True)


@pytest.mark.parametrize("costs", SCORE_COSTS)
def test_tokens_ref_matches_byte_oracle(costs):
    rng = np.random.default_rng(4)
    for t in range(30):
        la, lb = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        x = bytes(rng.integers(1, 6 if t % 2 else 256, la).astype(np.uint8))
        y = bytes(rng.integers(1, 6 if t % 2 else 256, lb).astype(np.uint8))
        assert R.levenshtein(x, y, None, True, costs) == O.levenshtein_naive_with_opts(x, y, True, costs), (x, y)
        for k in (0, 3, 8):
            d, tr = O.levenshtein_simd_k_with_opts(x, y, k, True, costs)
            want = None if d is None else (d, tr)
            assert R.levenshtein(x, y, k, True, costs) == want, (x, y, k)
