"""not-gpu: the table form of the band kernel with its strings taken from the parked registers (lev_bits_tab_body.h: no string rings in
LDS) on the 64-lane host emulation (tests/emu_tab, as it is), answer by answer against the oracle: 70 pairs -- two wavefronts, the second
ragged -- of every geometry of tab_regs_cases.GEOMETRIES, over the alphabets {0}, {0x0C, 0x0D} and 0..255, half of them mutated copies
within k and half unrelated.  The driver refuses nothing (every geometry is inside the table form's domain) and its probe finds the
nibble tables, rebuilt from the window's rows in front of every 16th column, equal to the incrementally kept ones."""
import numpy as np
import pytest

import tab_regs_cases as RC
from test_emu_lev_bits_tab import lib

N = 70


def test_geometries_cover_every_offset_of_the_window():
    lo = {RC.nlo(la, lb, k) for la, lb, k in RC.GEOMETRIES}
    assert {x % 16 for x in lo} == set(range(16))
    assert {RC.nlo(la, lb, k) % 16 for la, lb, k in RC.GEOMETRIES if la > lb} == set(range(16))
    assert {RC.nlo(la, lb, k) % 16 for la, lb, k in RC.GEOMETRIES if la < lb} | {0} == set(range(16))
    assert 0 in lo and 32 in lo and 16 in lo
    lengths = {x for la, lb, _ in RC.GEOMETRIES for x in (la, lb)}
    assert {129, 143, 144, 255, 256, 257, 272, 385} <= lengths


@pytest.mark.parametrize("la,lb,k", RC.GEOMETRIES)
def test_geometry(la, lb, k):
    a, b = RC.pairs(la, lb, k, N)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    out, probe = np.full(N, 0x12345678, np.uint32), np.zeros(2, np.uint64)
    rc = lib().emu_lev_bits_tab(a.ctypes.data, la, b.ctypes.data, lb, N, k, 1, out.ctypes.data, probe.ctypes.data)
    assert rc == 0, "outside the table form's domain"
    want = RC.want(la, lb, k, N)
    print("nlo", RC.nlo(la, lb, k), "blocks", int(probe[0]), "bad words", int(probe[1]), "differing", int((out != want).sum()))
    assert np.array_equal(out, want), np.flatnonzero(out != want)[:10]
    assert probe[0] > 0 and probe[0] == 2 * ((lb + 15) // 16) and probe[1] == 0, probe
    assert (want[0::2] != RC.NONE).all(), "the mutated copies are within k"
    assert (want[5::6] == RC.NONE).any(), "unrelated pairs over all byte values are beyond k"
