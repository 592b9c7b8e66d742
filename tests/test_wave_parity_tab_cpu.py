"""not-gpu: the host emulation of the table form's operations (EmuTab, tests/emu_tab/emu_tab_ops.h; device side: DevTab,
triple_accel_amd/csrc/wave_tab.h) against an independent statement of each in numpy -- byte 1 of the two address registers <- the low and the high
nibble of byte N of x, their other three bytes kept; a dword of LDS read and XOR-ed by its address from the start of the block's LDS; a table
flip followed by a lookup as the kernel body issues them -- and completeness: every operation the body takes from its policy T and every
member of DevTab has a row, and the device library holds a gfx950 code object."""
import os
import re

import numpy as np
import pytest

import tab_parity_lib as TP

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "triple_accel_amd", "csrc")


@pytest.fixture(scope="module")
def run():
    inp = TP.build_cases()
    return inp, TP.run_emu(inp)


def test_every_table_operation_has_a_row():
    covered = {r.split(":")[0] for r in TP.ROWS}
    dev = open(os.path.join(CSRC, "wave_tab.h")).read()
    members = set(re.findall(r"static __device__ __forceinline__ [^(;{]*?\b(\w+)\(", dev))
    assert members == {"nib_to_byte1", "lds_abs_read32", "lds_abs_xor32", "lds_address"}, members
    assert members <= covered
    used = set(re.findall(r"\bT::(?:template )?(\w+)", open(os.path.join(CSRC, "lev_bits_tab_body.h")).read()))
    assert used and used <= covered, used - covered


def test_the_device_library_holds_a_gfx950_code_object():
    TP.dev()
    blob = open(os.path.join(TP._DIR, "libta_tab_parity.so"), "rb").read()
    assert b"gfx950" in blob and b"ta_tab_parity_kernel" in blob


def test_nibble_addresses_against_their_statement(run):
    inp, out = run
    x, z = inp[:, 0], inp[:, 2]
    for n in range(4):
        byte = (x >> np.uint32(8 * n)) & np.uint32(0xFF)
        keep = np.uint32(0xFFFF00FF)
        assert np.array_equal(out[n], (z & keep) | ((byte & np.uint32(15)) << np.uint32(8)))
        assert np.array_equal(out[4 + n], (~z & keep) | ((byte >> np.uint32(4)) << np.uint32(8)))
        assert len(np.unique(byte)) == 256                  # every byte value in every position
    assert ((z & np.uint32(0xFF00)) != 0).any() and ((z & np.uint32(0xFFFF0000)) != 0).any()


def test_absolute_lds_accesses_against_their_statement(run):
    inp, out = run
    x, y = inp[:, 0], inp[:, 1]
    lanes = np.arange(64)
    assert (out[8] == 0).all()
    assert np.array_equal(out[9], (x ^ y)[:, (lanes + 7) & 63])
    assert np.array_equal(out[10], (x ^ y)[:, (lanes + 9) & 63])


def test_flip_then_lookup_against_its_statement(run):
    inp, out = run
    x, y = inp[:, 0], inp[:, 1]
    same = ((x >> np.uint32(16)) & np.uint32(0xFF)) == ((y >> np.uint32(8)) & np.uint32(0xFF))
    bit = (np.uint32(1) << (np.arange(inp.shape[0], dtype=np.uint32) & np.uint32(31)))[:, None]
    assert np.array_equal(out[11], np.where(same, bit, np.uint32(0)))
    assert same.any() and not same.all()
