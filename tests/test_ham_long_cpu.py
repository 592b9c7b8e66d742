"""not-gpu: the long-pair Hamming body (ham_long_body.h) under host emulation -- a wavefront of 64 emulated lanes counts the mismatches
of one slice; every answer is compared with numpy's (a != b).sum() and the oracle's hamming.  The strings sit at every head alignment
inside buffers whose other bytes are hostile (and differ between a and b), so one byte read outside the slice changes the count; the
buffers end right behind the last hostile byte the body may not need, so a read far outside is a fault.  Plus ham_wants_slices against
an independent restatement (tests/cpp/ham_rules_check.cpp), and the argument errors of ta_hamming_dev and its refusal to run without a
device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu_ham_long")
SLICE_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)
LONGER = (4095, 4096, 4097, 4096 + 1024 + 16 + 3, 2 * 4096 + 5)       # whole trips, then the predicated pieces, then the odd bytes
ALPHABETS = {
    "acgt": np.frombuffer(b"ACGT", np.uint8),
    "lower": np.arange(97, 123, dtype=np.uint8),
    "0..255": np.arange(0, 256, dtype=np.uint8),
    "nul": np.array([0x00], np.uint8),                            # what a lane without a piece holds ...
    "nul+0c": np.array([0x00, 0x0C], np.uint8),                   # ... and the constant folded into the compare
    "0c+0d": np.array([0x0C, 0x0D], np.uint8),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(EMU_DIR, "libta_emu_ham_long.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        _lib.emu_ham_long_slice.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        _lib.emu_ham_long_slice.restype = C.c_uint32
        _lib.emu_ham_long_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]
        _lib.emu_ham_long_pair.restype = C.c_uint64
        _lib.emu_ham_long_slice_bytes.argtypes = [C.c_uint64, C.c_uint32]
        _lib.emu_ham_long_slice_bytes.restype = C.c_uint32
    return _lib


def place(data, align, fill):
    """`data` at `align` bytes past a 16-byte boundary, `fill` in the 32 bytes in front of it and the 32 behind -> (keepalive, address)"""
    raw = np.full(len(data) + 96, fill, np.uint8)
    base = (-raw.ctypes.data) % 16 + 32 + align
    raw[base:base + len(data)] = data
    return raw, raw.ctypes.data + base


def emu(a, b, aa=0, ab=0, fills=(0x5A, 0xA5)):
    ka, pa = place(a, aa, fills[0])
    kb, pb = place(b, ab, fills[1])
    return int(lib().emu_ham_long_slice(pa, pb, len(a)))


def rand(g, alphabet, n):
    return g.choice(alphabet, n).astype(np.uint8)


def mutate(g, a, alphabet, rate):
    """a with about `rate` of its bytes changed (to another symbol of the alphabet when it has one, else to any other byte)"""
    b = a.copy()
    for p in np.flatnonzero(g.random(len(a)) < rate):
        others = [int(c) for c in alphabet if int(c) != int(a[p])] or [int(a[p]) ^ 0x0C, int(a[p]) ^ 0xFF]
        b[p] = others[int(g.integers(len(others)))]
    return b


def want(a, b):
    return int((a != b).sum())


def test_numpy_count_is_the_oracles_hamming():
    g = Dg.rng(9001)
    for name, alphabet in ALPHABETS.items():
        for n in SLICE_LENS + LONGER:
            a = rand(g, alphabet, n)
            b = mutate(g, a, alphabet, 0.2)
            assert O.hamming_naive(bytes(a), bytes(b)) == want(a, b), (name, n)
    assert O.hamming_naive(b"ab", b"abc") is None


@pytest.mark.parametrize("name", list(ALPHABETS))
def test_every_slice_length_every_alphabet(name):
    g = Dg.rng(9100 + len(name))
    alphabet = ALPHABETS[name]
    for n in SLICE_LENS + LONGER:
        a = rand(g, alphabet, n)
        for rate in (0.0, 0.03, 0.5):
            b = mutate(g, a, alphabet, rate)
            assert emu(a, b) == want(a, b), (n, rate)
            assert emu(a, b, 3, 9) == want(a, b), (n, rate)


@pytest.mark.parametrize("aa", range(16))
def test_every_head_alignment_with_hostile_neighbours(aa):
    """a at every alignment 0..15, b at {0, 1, 7, 15}; the bytes around a and b differ from each other (so a byte read outside would
    count) in one run and agree where the strings differ in none: the count must be the strings' alone both times"""
    g = Dg.rng(9200 + aa)
    alphabet = ALPHABETS["0..255"]
    for n in SLICE_LENS + (4097,):
        a = rand(g, alphabet, n)
        b = mutate(g, a, alphabet, 0.1)
        w = want(a, b)
        for ab in (0, 1, 7, 15):
            assert emu(a, b, aa, ab, (0x5A, 0xA5)) == w, (n, aa, ab)
            assert emu(a, b, aa, ab, (0x00, 0x0C)) == w, (n, aa, ab)
            assert emu(a, b, aa, ab, (0xFF, 0xFF)) == w, (n, aa, ab)


@pytest.mark.parametrize("name", list(ALPHABETS))
def test_all_equal_and_all_different(name):
    alphabet = ALPHABETS[name]
    for n in SLICE_LENS + LONGER:
        a = np.full(n, alphabet[0], np.uint8)
        other = int(alphabet[-1]) if len(alphabet) > 1 else int(alphabet[0]) ^ 0x0C      # (0x00 against 0x0C: the folded constant itself)
        b = np.full(n, other, np.uint8)
        for aa, ab in ((0, 0), (5, 0), (0, 11), (15, 1)):
            assert emu(a, a.copy(), aa, ab) == 0, (n, aa, ab)
            assert emu(a, b, aa, ab) == n, (n, aa, ab)


def test_a_mismatch_in_the_first_and_in_the_last_byte_counts_once():
    g = Dg.rng(9300)
    alphabet = ALPHABETS["acgt"]
    for n in SLICE_LENS[1:] + LONGER:
        a = rand(g, alphabet, n)
        for where in {0, n - 1, n // 2, (n - 1) & ~15, max((n & ~15) - 1, 0)}:
            b = a.copy()
            b[where] ^= 0x0C
            assert emu(a, b, 7, 2) == 1, (n, where)


def test_a_pair_cut_into_slices_adds_up():
    """the kernel's cut: slices of S bytes, the last one shorter; at every S of the tests and the product's 16 KiB"""
    g = Dg.rng(9400)
    alphabet = ALPHABETS["lower"]
    for n in (0, 1, 1023, 1024, 1025, 2 * 1024 + 15, 7 * 1024 + 1, 40000, 3 * 16384 + 17):
        a = rand(g, alphabet, n)
        b = mutate(g, a, alphabet, 0.07)
        ka, pa = place(a, 3, 0x11)
        kb, pb = place(b, 14, 0xEE)
        for S in (1024, 4096, 16384):
            assert int(lib().emu_ham_long_pair(pa, pb, n, S)) == want(a, b), (n, S)


def test_slice_length_rule():
    """S doubles until the batch has at most 2^20 full slices (the partial counts fit a scratch of known size), and stops at 256 MiB"""
    f = lib().emu_ham_long_slice_bytes
    assert f(0, 16384) == 16384 and f(1 << 30, 16384) == 16384 and f((1 << 34), 16384) == 16384
    assert f((1 << 34) + 16384, 16384) == 32768 and f(1 << 40, 1024) == 1 << 20
    assert f(1 << 62, 1024) == 1 << 28
    for s0 in (1024, 16384, 65536):
        for b in (0, 1, 1 << 20, 1 << 33, (1 << 36) + 5, 1 << 44):
            s = f(b, s0)
            assert s >= s0 and s % s0 == 0 and (s & (s - 1)) == 0 and b // s <= 1 << 20
            assert s == s0 or b // (s // 2) > 1 << 20


# ---------------------------------------------------------------- the routing rule against its restatement
def test_ham_wants_slices_matches_its_restatement():
    exe = os.path.join(ROOT, "tests", "cpp", "build", "ham_rules_check")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "triple_accel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ham_rules_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ham rules: ok" in out.stdout


# ---------------------------------------------------------------- the C ABI: argument errors come first, no CPU fallback
def _abi():
    from triple_accel_amd import _native as N
    return N


def test_abi_symbol_is_declared_and_exported():
    N = _abi()
    assert "ta_hamming_dev" in N.ABI_SYMBOLS and hasattr(N.lib(), "ta_hamming_dev")
    header = open(os.path.join(ROOT, "include", "triple_accel_amd.h")).read()
    assert "int ta_hamming_dev(const uint8_t *a_dev, const uint8_t *b_dev, size_t len, uint32_t *out_dev, void *stream);" in header
    assert "src/hamming.rs:390 -> :317, of ONE pair" in header


def test_abi_argument_errors_come_before_the_device():
    N = _abi()
    f = N.lib().ta_hamming_dev
    fake, out = C.c_void_p(0x1000), C.c_void_p(0x2000)
    assert f(fake, fake, 8, None, None) == N.TA_ERR_ARG
    assert f(None, None, 0, None, None) == N.TA_ERR_ARG                                # the result slot is required whatever the length
    assert f(None, fake, 8, out, None) == N.TA_ERR_ARG
    assert f(fake, None, 8, out, None) == N.TA_ERR_ARG
    assert f(None, None, 1, out, None) == N.TA_ERR_ARG
    assert f(None, fake, 1 << 40, out, None) == N.TA_ERR_ARG                           # an argument error wins over an unsupported length
    for n in (0xFFFFFFFF, 1 << 32, 1 << 40):
        assert f(fake, fake, n, out, None) == N.TA_ERR_UNSUPPORTED, n


def test_no_cpu_fallback():
    import torch
    N = _abi()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    f = N.lib().ta_hamming_dev
    blob = (C.c_uint8 * 4096)()
    ptr = C.cast(blob, C.c_void_p)
    out = (C.c_uint32 * 1)()
    for n in (0, 1, 1024, 1025, 4096):
        assert f(ptr, ptr, n, C.cast(out, C.c_void_p), None) == N.TA_ERR_HIP, n
    assert f(None, None, 0, C.cast(out, C.c_void_p), None) == N.TA_ERR_HIP             # len = 0 is answered on the device too
    assert f(ptr, ptr, 0xFFFFFFFE, C.cast(out, C.c_void_p), None) == N.TA_ERR_HIP      # the longest supported pair
