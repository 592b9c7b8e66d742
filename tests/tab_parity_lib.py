"""ctypes binding of the table form's parity libraries (tests/wave_parity_tab/) and the cases both sides run.  TESTS ONLY.
Layout of the buffers and the rows: tests/wave_parity_tab/tab_ops_body.h."""
import ctypes as C
import os
import subprocess

import numpy as np

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wave_parity_tab")
N_OPS = 12
ROWS = ["nib_to_byte1:lo%d" % n for n in range(4)] + ["nib_to_byte1:hi%d" % n for n in range(4)] + \
       ["lds_address", "lds_abs_xor32", "lds_abs_read32", "flip_then_lookup"]
_libs = {}


def _lib(which):
    if which not in _libs:
        subprocess.check_call(["make", "-C", _DIR, "-s"])
        L = C.CDLL(os.path.join(_DIR, {"emu": "libta_tab_parity_emu.so", "dev": "libta_tab_parity.so"}[which]))
        L.ta_tab_parity_run.restype = C.c_int
        L.ta_tab_parity_run.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        assert L.ta_tab_parity_n_ops() == N_OPS == len(ROWS)
        _libs[which] = L
    return _libs[which]


def emu():
    return _lib("emu")


def dev():
    """the device library (loading it needs the HIP runtime, not a GPU)"""
    return _lib("dev")


def build_cases():
    """-> (n, 3, 64) uint32: x, y, z per lane.  x and y: every byte value in every byte position (cases 0..15) and random words; z (the
    address register the nibble goes into): lane * 4, all ones, all zeros, random words."""
    g = np.random.default_rng(0x7AB0)
    lanes = np.arange(64, dtype=np.uint64)
    cases = []
    for pos in range(4):
        for q in range(4):
            v = (lanes + 64 * q) << np.uint64(8 * pos)
            fill = g.integers(0, 1 << 32, 64, dtype=np.uint64) & ~np.uint64(0xFF << (8 * pos))
            z = [lanes * 4, np.full(64, 0xFFFFFFFF, np.uint64), np.zeros(64, np.uint64), g.integers(0, 1 << 32, 64, dtype=np.uint64)][q]
            cases.append((v | fill, (v[::-1] | fill), z))
    for _ in range(48):
        cases.append(tuple(g.integers(0, 1 << 32, 64, dtype=np.uint64) for _ in range(3)))
    return np.array(cases, dtype=np.uint64).astype(np.uint32)


def run_emu(inp):
    inp = np.ascontiguousarray(inp)
    out = np.full((N_OPS, inp.shape[0], 64), 0xA5A5A5A5, np.uint32)
    assert emu().ta_tab_parity_run(inp.ctypes.data, out.ctypes.data, inp.shape[0], None) == 0
    return out
