"""not-gpu: the table form of the band kernel (lev_bits_tab_body.h) on the 64-lane host emulation (tests/emu_tab), answer by answer
against the oracle: every geometry of tab_cases.SHAPES on the 209 pairs of test_gpu_lev_bits_core.pairs() and on 209 pairs over the
alphabets that attack two nibble tables, the pair counts 1, 63, 64, 65, 209, the scaled route (k = 64 under costs (2, 2, 0)); in front of
every 16th column the driver rebuilds both tables from the window's rows and compares them with the incrementally kept ones; and the same
driver as a program of its own under AddressSanitizer + UndefinedBehaviorSanitizer (emu_tab_san) ends clean."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tab_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_tab")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(os.path.join(EMU_DIR, "libta_emu_tab.so"))
        _lib.emu_lev_bits_tab.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        _lib.emu_lev_bits_tab.restype = C.c_int
    return _lib


def emu(a, b, k, costs):
    """-> the answers; asserts that the table invariant held in front of every 16th column of every wavefront"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    n = a.shape[0]
    out, probe = np.full(n, 0x12345678, np.uint32), np.zeros(2, np.uint64)
    rc = lib().emu_lev_bits_tab(a.ctypes.data, a.shape[1], b.ctypes.data, b.shape[1], n, k, costs[0], out.ctypes.data, probe.ctypes.data)
    assert rc == 0, rc
    waves, blocks = (n + 63) // 64, (b.shape[1] + 15) // 16
    assert probe[0] == waves * blocks and probe[1] == 0, "tables rebuilt from the window differ from the kept ones: %s" % probe
    return out


@pytest.mark.parametrize("la,lb,k,costs", TC.SHAPES)
def test_shapes_on_the_core_pairs(la, lb, k, costs):
    a, b = TC.core_pairs(la, lb, k // costs[0])
    want = TC.want("core", la, lb, k, costs)
    got = emu(a, b, k, costs)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert (want != TC.NONE).sum() >= 20 and (want == TC.NONE).sum() >= 20        # every shape: answers within k and beyond it
    if la == lb:
        assert (want == k).any() and (want == 0).any() and (want == TC.NONE).sum() > 10 and (want != TC.NONE).sum() > 60


@pytest.mark.parametrize("la,lb,k,costs", TC.SHAPES)
def test_shapes_on_the_attacking_alphabets(la, lb, k, costs):
    a, b = TC.alphabet_pairs(la, lb, k // costs[0])
    want = TC.want("alpha", la, lb, k, costs)
    got = emu(a, b, k, costs)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert (want != TC.NONE).sum() >= 20 and (want == TC.NONE).sum() >= 20
    if la == lb:
        for r in range(len(TC.ALPHABETS)):                 # every alphabet has pairs within k and pairs beyond it
            w = want[r::len(TC.ALPHABETS)]
            assert (w != TC.NONE).any() and ((w == TC.NONE).any() or r == 0), r


@pytest.mark.parametrize("n", TC.PAIR_COUNTS)
def test_pair_counts(n):
    a, b = TC.core_pairs(256, 256, 32)
    got = emu(a[:n], b[:n], 32, TC.LEV)
    assert np.array_equal(got, TC.want("core", 256, 256, 32, TC.LEV)[:n])


def test_outside_the_domain_is_refused():
    a, b = TC.core_pairs(256, 256, 32)
    out = np.zeros(TC.Core.N, np.uint32)
    args = lambda aa, bb, k, g: (aa.ctypes.data, aa.shape[1], bb.ctypes.data, bb.shape[1], aa.shape[0], k, g, out.ctypes.data, None)   # noqa: E731
    assert lib().emu_lev_bits_tab(*args(np.array(a), np.array(b), 23, 1)) == 1            # 24 diagonals: below the stride-8 form
    assert lib().emu_lev_bits_tab(*args(np.array(a), np.array(b), 33, 1)) == 1            # 34 diagonals: wider than the window
    assert lib().emu_lev_bits_tab(*args(np.array(a[:, :128]), np.array(b[:, :128]), 32, 1)) == 1   # one line per string: the chunk form's


def test_sanitizer_build_of_the_driver_ends_clean():
    """the driver with its own main and its own scalar reference, built with -fsanitize=address,undefined (tests/emu_tab/Makefile).  Its
    global loads go to memory unchecked by the emulation there (blobs with the API's 16 bytes of read slack and nothing more), so a read
    outside them is the sanitizer's to report, like every LDS access and every store"""
    subprocess.check_call(["make", "-C", EMU_DIR, "-s", "emu_tab_san"])
    r = subprocess.run([os.path.join(EMU_DIR, "emu_tab_san")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "emu_tab: ok" in r.stdout and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
