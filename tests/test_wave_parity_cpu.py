"""The wave vocabulary's parity harness (tests/wave_parity/), the part that runs without a GPU.

* completeness: every static member of DevWave (wave.h) and every W::name the kernel bodies use has a row in the op table of
  wave_ops_body.h or a reason in the exclusion table -- a primitive added later without coverage fails here;
* EmuWave against an independent statement of each non-trivial primitive, in numpy, written from the instruction set's description
  (v_perm_b32's whole selector table, v_alignbit / v_alignbyte, v_bfe_u32, v_dot4 without clamp, v_ffbh, the carry of v_addc, the DPP wave
  shifts, v_bitop3's truth table) and not from either implementation.  Whether the DEVICE agrees is tests/test_gpu_wave_parity.py's part;
* the device library cross-compiles for gfx950."""
import glob
import os
import re

import numpy as np
import pytest

import wave_parity_lib as WP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "triple_accel_amd", "csrc")
M32 = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def run():
    inp, hdr, tags = WP.build_cases()
    names = WP.op_names()
    out = WP.run_emu(inp, hdr, names)
    hdrs = hdr[WP.HDR_GLOBAL:].reshape(-1, WP.HDR_WORDS)
    return inp, hdr, hdrs, tags, names, out


def covered(names):
    return {n.split(":")[0] for n in names}


def test_every_devwave_member_is_covered_or_excluded():
    src = open(os.path.join(CSRC, "wave.h")).read()
    dev = src[src.index("struct DevWave"):]
    members = set(re.findall(r"static __device__ __forceinline__ [^(;{]*?\b(\w+)\(", dev))
    assert len(members) > 80 and {"lane", "gload_line_keep", "byte_eq_or", "wave_sum"} <= members, sorted(members)
    have = covered(WP.op_names())
    assert not (have & set(WP.EXCLUDED)), have & set(WP.EXCLUDED)
    missing = members - have - set(WP.EXCLUDED)
    assert not missing, "DevWave primitives without a parity row or an exclusion: %s" % sorted(missing)


def test_every_primitive_the_bodies_use_is_covered():
    used = set()
    bodies = sorted(glob.glob(os.path.join(CSRC, "*_body.h")))
    assert len(bodies) >= 10
    for path in bodies:
        text = open(path).read()
        used |= set(re.findall(r"\bW::(?:template )?(\w+)", text))
        if re.search(r"\bbitop3<", text):
            used.add("bitop3")
    have = covered(WP.op_names())
    missing = used - have - set(WP.EXCLUDED) - WP.TYPES
    assert not missing, "used by a kernel body, not in the parity table: %s" % sorted(missing)


def test_every_constant_perm_selector_of_the_bodies_is_in_the_table():
    """the selectors are template expressions: evaluate them over the ranges of their parameters"""
    want = set()
    for BI in range(4):                                         # lev_band_body.h advance_a / advance_b<BI>, every intake byte ibm
        want |= {0x0605000C | (BI << 8), 0x00070605 | (BI << 24)}
        for ibm in (1, 2, 3):
            s0 = BI if ibm == 1 else 0x05
            s1 = 0x0C if ibm == 1 else (BI if ibm == 2 else 0x06)
            s2 = BI if ibm == 3 else 0x0C
            want.add((0x0C << 24) | (s2 << 16) | (s1 << 8) | s0)
    for c in range(4):                                          # lev_bits2_body.h step<C>
        want.add(c * 0x0101 + (4 + c) * 0x01010000)
    for e in (0, 2):
        want.add(0x00030001 | ((4 + e) << 8) | ((5 + e) << 24))
    want |= {0x05010400, 0x07030602}
    have = {int(n.split(":")[1], 16) for n in WP.op_names() if n.startswith("perm:")}
    assert want <= have, ["%08x" % s for s in sorted(want - have)]
    # and the source holds no perm<> this list does not know of
    n_sites = sum(len(re.findall(r"W::template perm<", open(p).read())) for p in glob.glob(os.path.join(CSRC, "*_body.h")))
    assert n_sites == 9, n_sites


def test_the_op_tables_of_both_builds_agree():
    assert WP.op_names(WP.emu()) == WP.op_names(WP.dev())       # the device library cross-compiled for gfx950, and loads
    names = WP.op_names()
    assert len(names) == len(set(names))
    assert sum(n.startswith("bitop3:") for n in names) == 256 and sum(n.startswith("alignbit:") for n in names) == 32


def test_the_device_library_holds_a_gfx950_code_object():
    WP.dev()
    blob = open(WP.DEV_SO, "rb").read()
    assert b"gfx950" in blob and b"ta_wave_parity_kernel" in blob


def test_cases_cover_what_the_issue_asks(run):
    inp, hdr, hdrs, tags, names, out = run
    x, y, z = (inp[:, j].astype(np.uint64) for j in range(3))
    assert len(tags) <= 512                                     # one launch, a fraction of a second
    assert set(hdrs[:, WP.H_S]) == set(range(32)) and set(hdrs[:, WP.H_KAPPA]) == set(range(8))
    assert set(WP.MASKS) <= set(int(v) for v in hdrs[:, WP.H_M]) and set(WP.DIVS) <= set(int(v) for v in hdrs[:, WP.H_D])
    pairs = {(int(o), int(w)) for h in hdrs for o, w in zip(h[WP.H_BFE_OFF:WP.H_BFE_OFF + 8], h[WP.H_BFE_W:WP.H_BFE_W + 8])}
    assert pairs == set(WP.BFE) and len(WP.BFE) == 527
    cross = [i for i, t in enumerate(tags) if t == "cross"]
    assert sorted(int(hdrs[i, WP.H_L]) for i in cross) == list(range(64))
    assert all(len(set(x[i])) == 64 for i in cross)
    sel_bytes = {(pos, int(v)) for i, t in enumerate(tags) if t == "perm_sel" for pos in range(4) for v in (z[i] >> np.uint64(8 * pos)) & np.uint64(255)}
    assert {(pos, v) for pos in range(4) for v in range(256)} <= sel_bytes
    assert {int(v) & 7 for i, t in enumerate(tags) if t in ("clz", "shifts") for v in z[i]} == set(range(8))
    g = [i for i, t in enumerate(tags) if t == "gload"]
    assert {int(v) for i in g for v in x[i] & np.uint64(511)} == set(range(512))
    keep = {(int(hdrs[i, WP.H_KAPPA]), int((z[i] & np.uint64(1)).sum())) for i, t in enumerate(tags) if t == "line_keep"}
    assert keep == {(k, n) for k in range(8) for n in (64, 0, 32, 1)}
    first = {tuple(np.flatnonzero(z[i] & np.uint64(1))) for i in cross[:8]}
    assert (0,) in first and (63,) in first and any(len(f) == 1 and 0 < f[0] < 63 for f in first) and any(len(f) > 8 for f in first)
    sums = x.sum(axis=1)
    assert any(s >> np.uint64(32) for s in sums[[i for i, t in enumerate(tags) if t == "wave_sum"]])
    assert (x == 0).any() and (x == M32).any()                  # clz(0), dot4 of 0xFF bytes


# ---- the instruction set's description, in numpy (uint64 arithmetic, masked to 32 bits) -----------------------------------------------
def isa_perm(hi, lo, sel):
    """v_perm_b32 D = byte-permute of {S0 = hi, S1 = lo} by S2: selector 0..3 byte of S1, 4..7 byte of S0, 8..11 the sign of byte 1, 3, 5, 7
    replicated, 12 the constant 0x00, 13 and above 0xFF"""
    src = (hi << np.uint64(32)) | lo
    out = np.zeros_like(lo)
    for k in range(4):
        s = (sel >> np.uint64(8 * k)) & np.uint64(255)
        byte = (src >> (np.uint64(8) * (s & np.uint64(7)))) & np.uint64(255)
        sign_of = np.uint64(2) * (s & np.uint64(3)) + np.uint64(1)
        sign = ((src >> (np.uint64(8) * sign_of + np.uint64(7))) & np.uint64(1)) * np.uint64(255)
        b = np.where(s >= 13, np.uint64(255), np.where(s == 12, np.uint64(0), np.where(s >= 8, sign, byte)))
        out |= b << np.uint64(8 * k)
    return out


def bytes_of(a, signed):
    bs = [((a >> np.uint64(8 * k)) & np.uint64(255)).astype(np.int64) for k in range(4)]
    return [np.where(b >= 128, b - 256, b) if signed else b for b in bs]


def isa_dot4(a, b, acc, signed):
    t = acc.astype(np.int64)
    for p, q in zip(bytes_of(a, signed), bytes_of(b, signed)):
        t = t + p * q
    return (t & 0xFFFFFFFF).astype(np.uint64)                   # no clamp: modulo 2^32


def isa_clz(a):
    return np.array([32 - int(v).bit_length() for v in a.reshape(-1)], dtype=np.uint64).reshape(a.shape)


def test_emulation_against_the_isa_statements(run):
    inp, hdr, hdrs, tags, names, out = run
    x, y, z = (inp[:, j].astype(np.uint64) for j in range(3))
    p = (z & np.uint64(1)) != 0
    H = lambda k: hdrs[:, k].astype(np.uint64)[:, None]
    pair = (x << np.uint64(32)) | y                             # {hi = x, lo = y}
    want = {}
    for n in names:                                             # perm<SEL>
        if n.startswith("perm:"):
            want[n] = isa_perm(x, y, np.full_like(x, int(n.split(":")[1], 16)))
    want["perm_sel:v"] = isa_perm(x, y, z)
    want["ne12:v"] = isa_perm(np.full_like(x, 0xFFFFFFFF), np.full_like(x, 0xFFFFFFFF), x)
    for k in range(4):
        want["alignbyte:%d" % k] = (pair >> np.uint64(8 * k)) & M32
        want["splat_byte_n:%d" % k] = isa_perm(x, x, np.full_like(x, 0x04040404 + 0x01010101 * k))
        want["slide_in_byte:%d" % k] = isa_perm(x, y, np.full_like(x, 0x00030201 | ((4 + k) << 24)))
        want["dot4_byte:%d" % k] = isa_dot4(x, np.broadcast_to(H(WP.H_M8) << np.uint64(8 * k), x.shape), z, False)
    want["splat_byte:v"] = isa_perm(x, x, np.full_like(x, 0x04040404))
    want["alignbyte_v:v"] = (pair >> (np.uint64(8) * (z & np.uint64(3)))) & M32
    for k in range(32):
        want["alignbit:%d" % k] = (pair >> np.uint64(k)) & M32
    want["alignbit_rt:v"] = (pair >> H(WP.H_S)) & M32
    want["shr_u:v"] = x >> H(WP.H_S)
    want["lshl_add:v"] = ((x << H(WP.H_S)) + y) & M32
    for j in range(8):
        off, w = H(WP.H_BFE_OFF + j), H(WP.H_BFE_W + j)
        want["bfe:%d" % j] = (x >> off) & ((np.uint64(1) << w) - np.uint64(1))
    want["dot4:v"] = isa_dot4(x, y, z, False)
    want["sdot4:v"] = isa_dot4(x, y, z, True)
    want["sdot4_first:v"] = isa_dot4(x, y, np.zeros_like(x), True)       # |sum| <= 4 * 128 * 128: the clamp of this form cannot act
    want["clz:v"] = isa_clz(x)
    full = x + y + p.astype(np.uint64)
    want["addc:sum"], want["addc:cout"] = full & M32, full >> np.uint64(32)
    want["add_carry_mask:sum"], want["add_carry_mask:mask"] = (x + y) & M32, (x + y) >> np.uint64(32)
    want["from_lower:v"] = np.concatenate([y[:, :1], x[:, :-1]], axis=1)         # DPP wave_shr:1, lane 0 keeps `old`
    want["from_upper:v"] = np.concatenate([x[:, 1:], y[:, 63:]], axis=1)         # DPP wave_shl:1, lane 63 keeps `old`
    want["comp:dpp_back_to_back"] = np.concatenate([want["from_lower:v"][:, 1:], z[:, 63:]], axis=1)
    want["shfl:v"] = np.take_along_axis(x, (y & np.uint64(63)).astype(np.int64), axis=1)    # ds_bpermute: byte address (src << 2) mod 256
    want["wave_max:v"] = np.broadcast_to(x.max(axis=1)[:, None], x.shape)
    want["wave_sum:v"] = np.broadcast_to((x.sum(axis=1) & M32)[:, None], x.shape)
    want["readlane:v"] = np.take_along_axis(x, np.broadcast_to(H(WP.H_L), x.shape).astype(np.int64), axis=1)
    want["writelane:v"] = np.where(np.arange(64)[None, :] == H(WP.H_L), H(WP.H_M), x)
    want["lane:v"] = np.broadcast_to(np.arange(64, dtype=np.uint64), x.shape)
    a, b, c = x, y, z
    for tt in range(256):                                       # result bit = bit (4a + 2b + c) of the table
        r = np.zeros_like(x)
        for row in range(8):
            if (tt >> row) & 1:
                r |= (a if row & 4 else ~a) & (b if row & 2 else ~b) & (c if row & 1 else ~c)
        want["bitop3:%02X" % tt] = r & M32
    eqb = lambda k: ((x >> np.uint64(8 * k)) & np.uint64(255)) == ((y >> np.uint64(8 * k)) & np.uint64(255))
    for k in range(4):
        want["byte_eq:%d" % k] = eqb(k).astype(np.uint64)
        want["byte_eq_or:%d" % k] = (eqb(k) | (want["add_carry_mask:mask"] != 0)).astype(np.uint64)
    assert set(want) <= set(names), sorted(set(want) - set(names))
    bad = []
    for n, w in want.items():
        got = out[names.index(n)].astype(np.uint64)
        if not np.array_equal(got, w):
            c, l = np.argwhere(got != w)[0]
            bad.append("%s: case %d lane %d x=%08x y=%08x z=%08x emulation=%08x isa=%08x" % (n, c, l, x[c, l], y[c, l], z[c, l], got[c, l], w[c, l]))
    assert not bad, "\n".join(bad)
    assert len(want) > 350


def test_side_effect_rows_and_untouched_lanes(run):
    inp, hdr, hdrs, tags, names, out = run
    x, z = inp[:, 0], inp[:, 2]
    p, q = (z & 1) != 0, (z & 2) != 0
    st = out[names.index("store_u32:v")]
    cnt, lst = out[names.index("append_u32:count")], out[names.index("append_u32:list")]
    for c in range(len(tags)):
        perm = np.arange(64) ^ int(hdrs[c, WP.H_XS])
        want = np.full(64, WP.FILL, dtype=np.uint32)
        want[perm[p[c]]] = x[c][p[c]]
        assert np.array_equal(st[c], want), c
        n = int(q[c].sum())
        assert cnt[c, 0] == n and np.all(cnt[c, 1:] == WP.FILL)
        assert sorted(lst[c, :n]) == sorted(x[c][q[c]]) and np.all(lst[c, n:] == WP.FILL)
    # gload_line_keep: the lanes where !p keep the recognisable S
    for j in range(8):
        for w in range(4):
            row = out[names.index("gload_line_keep:%d_w%d" % (j, w))]
            assert np.all(row[~p] == 0x5EED0000 + j)
    # every other row was written in all 64 lanes of every case (the fill pattern survives nowhere by accident of the harness)
    assert (out == WP.FILL).mean() < 0.01
