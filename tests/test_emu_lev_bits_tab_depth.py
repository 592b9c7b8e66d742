"""not-gpu: the table form of the band kernel (lev_bits_tab_body.h) at both depths of its LDS stream -- LevBitsTab<EmuWave, EmuTab, Probe,
1> and <..., 2> -- on the 64-lane host emulation (tests/emu_tab_depth), answer by answer against the oracle on the shapes of
tab_depth_cases.py.  In front of every 16th column the driver rebuilds both nibble tables from the window's rows and compares them with
the incrementally kept ones: at a span's end the tables hold exactly the rows below it, however far the stream ran ahead inside the span
(zero differing words).  And the same driver as a program of its own under AddressSanitizer + UndefinedBehaviorSanitizer
(emu_tab_depth_san: its own main and scalar reference, run directly) ends clean."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tab_depth_cases as DC

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_tab_depth")
_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", EMU_DIR, "-s", "libta_emu_tab_depth.so"])
        _lib = C.CDLL(os.path.join(EMU_DIR, "libta_emu_tab_depth.so"))
        _lib.emu_lev_bits_tab_depth.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        _lib.emu_lev_bits_tab_depth.restype = C.c_int
    return _lib


def emu(a, b, k, depth):
    """-> the answers; asserts that the table invariant held in front of every 16th column of every wavefront"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    n = a.shape[0]
    out, probe = np.full(n, 0x12345678, np.uint32), np.zeros(2, np.uint64)
    rc = lib().emu_lev_bits_tab_depth(a.ctypes.data, a.shape[1], b.ctypes.data, b.shape[1], n, k, depth, out.ctypes.data, probe.ctypes.data)
    assert rc == 0, rc
    waves, blocks = (n + 63) // 64, (b.shape[1] + 15) // 16
    assert probe[0] == waves * blocks and probe[1] == 0, "tables rebuilt from the window differ from the kept ones: %s" % probe
    return out


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("la,lb,k", DC.SHAPES)
def test_shapes_at_both_depths(la, lb, k, depth):
    a, b = DC.pairs(la, lb)
    want = DC.want(la, lb, k)
    got = emu(a, b, k, depth)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    DC.check_shares(want)


def test_no_third_depth_and_no_shape_outside_the_domain():
    a, b = DC.pairs(256, 256)
    out = np.zeros(DC.N, np.uint32)
    args = lambda aa, bb, k, d: (aa.ctypes.data, aa.shape[1], bb.ctypes.data, bb.shape[1], aa.shape[0], k, d, out.ctypes.data, None)   # noqa: E731
    assert lib().emu_lev_bits_tab_depth(*args(np.array(a), np.array(b), 32, 3)) == 2
    assert lib().emu_lev_bits_tab_depth(*args(np.array(a), np.array(b), 33, 1)) == 1            # 34 diagonals: wider than the window
    assert lib().emu_lev_bits_tab_depth(*args(np.array(a[:, :128]), np.array(b[:, :128]), 32, 2)) == 1   # one line per string


def test_sanitizer_build_of_the_driver_ends_clean():
    """the driver with its own main and its own scalar reference, built with -fsanitize=address,undefined (tests/emu_tab_depth/Makefile)
    and run as a program: blobs with the API's 16 bytes of read slack and nothing more, both depths on every shape"""
    subprocess.check_call(["make", "-C", EMU_DIR, "-s", "emu_tab_depth_san"])
    r = subprocess.run([os.path.join(EMU_DIR, "emu_tab_depth_san")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "emu_tab_depth: ok" in r.stdout and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
