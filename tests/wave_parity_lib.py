"""ctypes binding of the wave-vocabulary parity libraries (tests/wave_parity/) and the cases both sides run.  TESTS ONLY.

libta_wave_parity_emu.so runs WaveOps<EmuWave> on the host, libta_wave_parity.so runs WaveOps<DevWave> in a gfx950 kernel; both
take the same three buffers (layout: tests/wave_parity/wave_ops_body.h)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_DIR = os.path.join(_HERE, "wave_parity")
EMU_SO = os.path.join(_DIR, "libta_wave_parity_emu.so")
DEV_SO = os.path.join(_DIR, "libta_wave_parity.so")
_libs = {}

CASE_WORDS, HDR_GLOBAL, HDR_WORDS = 192, 256, 32             # wave_ops_body.h
H_S, H_M, H_L, H_KAPPA, H_D, H_TRIPS, H_M8, H_XS, H_BFE_OFF, H_BFE_W, H_STRIDE, H_LEN = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 24, 25
FILL = 0xA5A5A5A5

# primitives of DevWave that no row can observe, each with its reason (the issue's carve-outs)
EXCLUDED = {
    "opaque": "a value barrier for the optimiser: the identity, no instruction",
    "opaque_s": "the same for a wave-uniform value",
    "case_tag": "an assembler comment that keeps switch cases apart: no instruction",
    "mem_fence": "orders this wave's global stores against its later loads: no value of its own",
    "lds_wave_sync": "a compiler barrier around same-wave LDS traffic (the LDS rows run through it): no value of its own",
    "wait_vm0": "waits for the loads of gload_line_keep (whose rows run through it): no value of its own",
}
# named by W:: in the bodies but types, not operations
TYPES = {"U32", "Bool", "Ptr", "Q", "Mask"}


def _make():
    subprocess.check_call(["make", "-C", _DIR, "-s"])


def _bind(path):
    L = C.CDLL(path)
    L.ta_wave_parity_run.restype = C.c_int
    L.ta_wave_parity_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.ta_wave_parity_op_name.restype = C.c_char_p
    L.ta_wave_parity_op_name.argtypes = [C.c_int]
    L.ta_wave_parity_n_ops.restype = C.c_int
    return L


def emu():
    if "emu" not in _libs:
        _make()
        _libs["emu"] = _bind(EMU_SO)
    return _libs["emu"]


def dev():
    """the device library (loading it needs the HIP runtime, not a GPU)"""
    if "dev" not in _libs:
        _make()
        _libs["dev"] = _bind(DEV_SO)
    return _libs["dev"]


def op_names(L=None):
    L = L or emu()
    return [L.ta_wave_parity_op_name(i).decode() for i in range(L.ta_wave_parity_n_ops())]


def aligned_u32(n_words, fill=0):
    """uint32 array whose data starts on a 256-byte boundary"""
    raw = np.empty(n_words + 64, dtype=np.uint32)
    skip = (-raw.ctypes.data % 256) // 4
    a = raw[skip:skip + n_words]
    a[:] = fill
    assert a.ctypes.data % 256 == 0
    return a


# ---------------------------------------------------------------------------------------------------------------- the cases
EDGE = [0, 1, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0x0C0C0C0C, 0x0D0C0B0A, 0x0C0D0C0D, 0x00FF00FF, 0xFF00FF00, 0x80808080, 0x7F7F7F7F,
        0x01020304] + [v << (8 * k) for k in range(4) for v in (0x0B, 0x0C, 0x0D)]
# the constant masks the bodies pass to bfi / bfi_k (lev_search_wave_body.h, lev_bits_body.h, lev_bits2_body.h), the and_or chain's, 0, ~0
MASKS = [0xFFFF0000, 0x01010101, 0x04040404, 0x10101010, 0x40404040, 0x0F0F0F0F, 0x03030303, 0x30303030, 0x02020202, 0x08080808,
         0x20202020, 0x80808080, 0, 0xFFFFFFFF]
# lev_band_body.h divides by the lanes per pair L (a power of two up to 64) and the band's diagonal count D
DIVS = [1, 2, 4, 8, 16, 32, 64, 3, 5, 7, 9, 17, 33, 65, 127, 255]
BFE = [(off, w) for w in range(1, 32) for off in range(0, 33 - w)]
WAVE_MAX_LANES = [0, 15, 16, 31, 32, 47, 48, 63]
KEEP_PREDS = ["all", "none", "alternating", "one"]


class Cases:
    def __init__(self):
        self.x, self.y, self.z, self.h, self.tag = [], [], [], [], []

    def add(self, x, y, z, tag, **hdr):
        i = len(self.x)
        for dst, v in ((self.x, x), (self.y, y), (self.z, z)):
            a = np.zeros(64, dtype=np.uint32)
            v = np.asarray(v, dtype=np.uint64).astype(np.uint32)
            a[:len(v)] = v
            dst.append(a)
        h = np.zeros(HDR_WORDS, dtype=np.uint32)
        h[H_S], h[H_M], h[H_L], h[H_KAPPA] = i % 32, MASKS[i % len(MASKS)], (i * 5) % 64, i % 8
        h[H_D], h[H_TRIPS], h[H_M8], h[H_XS] = DIVS[i % len(DIVS)], 1 + i % 8, (1, 255, 0, 0x80, 0x7F, 3)[i % 6], (i * 7) % 64
        for j in range(8):
            h[H_BFE_OFF + j], h[H_BFE_W + j] = BFE[(8 * i + j) % len(BFE)]
        h[H_STRIDE], h[H_LEN] = i % 13, (i * 37) & 0xFFFF
        for k, v in hdr.items():
            h[globals()["H_" + k.upper()]] = v
        self.h.append(h)
        self.tag.append(tag)


def build_cases():
    """-> (inp (n, 3, 64) uint32 view of an aligned buffer, hdr aligned uint32 buffer, tags): deterministic"""
    rng = np.random.default_rng(0x7A11E)
    r64 = lambda: rng.integers(0, 1 << 32, 64, dtype=np.uint64)
    lanes = np.arange(64, dtype=np.uint64)
    cs = Cases()
    # pure per-lane operations: the cross product of the edge words, then 2,048 random triples (lanes are independent: 64 triples a case)
    trip = np.array(list(itertools.product(EDGE, EDGE, EDGE)), dtype=np.uint64)
    trip = np.concatenate([trip, rng.integers(0, 1 << 32, (2048, 3), dtype=np.uint64)])
    for i in range(0, len(trip), 64):
        t = trip[i:i + 64]
        cs.add(t[:, 0], t[:, 1], t[:, 2], "pure")
    # perm_sel: every selector code in every byte position (the other three positions hold in-range selectors)
    sels = np.array([(0x07020500 & ~(0xFF << (8 * pos))) | (v << (8 * pos)) for pos in range(4) for v in range(256)], dtype=np.uint64)
    for i in range(0, len(sels), 64):
        cs.add(r64() | 0x80000000 * (i // 64 % 2), r64() | 0x00800000 * (i // 128 % 2), sels[i:i + 64], "perm_sel")
    # sdot4 / dot4: extreme bytes against accumulators at both ends of the range (no clamp: the sums wrap)
    bw = [0x7F7F7F7F, 0x80808080, 0xFFFFFFFF, 0x7F80FF01, 0x80FF7F00]
    accs = [0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0, 0x7FFF0000, 0x8000FFFF, 0xFFFC0400, 1]
    st = np.array(list(itertools.product(bw, bw, accs)), dtype=np.uint64)
    for i in range(0, len(st), 64):
        cs.add(st[i:i + 64, 0], st[i:i + 64, 1], st[i:i + 64, 2], "dot4")
    # clz of every single bit and of every run of low ones; per-lane shift counts 0..31 and byte counts 0..7 (alignbyte_v takes s & 3)
    cs.add(1 << (lanes % 32), r64(), lanes, "clz")
    cs.add((1 << (lanes % 33)) - 1, r64(), lanes, "clz")
    cs.add(r64(), r64(), lanes[::-1], "shifts")
    # cross-lane: lane-distinct values, every l for readlane / writelane; shfl sources: permutations, broadcasts, sources >= 64
    for l in range(64):
        kind = l % 4
        src = [rng.permutation(64).astype(np.uint64), np.full(64, l, dtype=np.uint64), r64(), lanes + 64 * (l + 1)][kind]
        z = r64()
        if l < 8:       # first_u32: the predicate (bit 0 of z) in exactly lane 0, lane 63, one random lane, many lanes
            z &= ~np.uint64(1)
            z[[0, 63, int(rng.integers(1, 63)), 0][l % 4]] |= np.uint64(1)
            if l % 4 == 3:
                z |= r64() & np.uint64(1)
        cs.add(rng.permutation(1 << 16)[:64].astype(np.uint64) * 65537 + 1, src, z, "cross", l=l)
    # wave_max: the maximum in the first and last lane of every DPP row, all equal, all zero, 0xFFFFFFFF; wave_sum wraps 2^32
    for L in WAVE_MAX_LANES:
        x = rng.integers(0, 1000, 64, dtype=np.uint64)
        x[L] = 0x80000000 + L
        cs.add(x, r64(), r64(), "wave_max")
    cs.add(np.full(64, 77), r64(), r64(), "wave_max")
    cs.add(np.zeros(64), r64(), r64(), "wave_max")
    x = rng.integers(0, 1000, 64, dtype=np.uint64)
    x[37] = 0xFFFFFFFF
    cs.add(x, r64(), r64(), "wave_max")
    cs.add(np.full(64, 0x04000001), r64(), r64(), "wave_sum")                    # 64 * 0x04000001 = 2^32 + 64
    cs.add(0xF0000000 + lanes, r64(), r64(), "wave_sum")
    # gload_line_keep: every kappa against the predicate on everywhere, nowhere, in alternating lanes, in one lane
    for kappa in range(8):
        for pk in KEEP_PREDS:
            z = r64() & ~np.uint64(1)
            if pk == "all":
                z |= np.uint64(1)
            elif pk == "alternating":
                z |= (lanes + kappa) & np.uint64(1)
            elif pk == "one":
                z[(kappa * 9 + 5) % 64] |= np.uint64(1)
            cs.add(r64(), r64(), z, "line_keep", kappa=kappa)
    # gload16 / gload16_all / gload16_nt / gload_u8: every byte offset of the block (so every offset mod 16), predicates both ways
    for k in range(8):
        cs.add(lanes + 64 * k, r64(), r64() | (3 if k % 2 else 0), "gload")
    n = len(cs.x)
    inp = aligned_u32(n * CASE_WORDS).reshape(n, 3, 64)
    inp[:, 0], inp[:, 1], inp[:, 2] = np.array(cs.x), np.array(cs.y), np.array(cs.z)
    hdr = aligned_u32(HDR_GLOBAL + n * HDR_WORDS)
    csr = np.sort(rng.integers(0, 769, 65, dtype=np.uint64))
    csr[0], csr[10], csr[64] = 0, csr[11], 768                                  # (an empty string among them)
    hdr[:130] = np.sort(csr).view(np.uint32)
    hdr[HDR_GLOBAL:] = np.array(cs.h).reshape(-1)
    return inp, hdr, cs.tag


def new_out(n_cases, names):
    out = aligned_u32(len(names) * n_cases * 64, FILL).reshape(len(names), n_cases, 64)
    out[names.index("append_u32:count"), :, 0] = 0
    return out


def run_emu(inp, hdr, names=None):
    names = names or op_names()
    out = new_out(inp.shape[0], names)
    rc = emu().ta_wave_parity_run(inp.ctypes.data, hdr.ctypes.data, out.ctypes.data, inp.shape[0], None)
    assert rc == 0, rc
    return out


def canonical(out, names):
    """the append list's order is not defined: sort the entries each case appended (in place)"""
    li, ci = names.index("append_u32:list"), names.index("append_u32:count")
    for c in range(out.shape[1]):
        n = min(int(out[ci, c, 0]), 64)
        out[li, c, :n] = np.sort(out[li, c, :n])
    return out


def carved_out(name):
    """lanes whose value the contract leaves open (wave.h: "the edge lane's value is overridden by the caller anyway")"""
    return {"from_lower0:v": [0], "from_upper0:v": [63]}.get(name, [])


def mismatches(got, want, names, inp, which=None, limit=10):
    """-> report lines: per op the first `limit` (case, lane) where got != want outside the carve-outs"""
    lines = []
    for i, name in enumerate(names):
        if which is not None and not which(name):
            continue
        bad = got[i] != want[i]
        bad[:, carved_out(name)] = False
        if not bad.any():
            continue
        cl = np.argwhere(bad)
        lines.append("%s: %d words differ" % (name, len(cl)))
        for c, l in cl[:limit]:
            lines.append("    case %d lane %d  x=%08x y=%08x z=%08x  device=%08x emulation=%08x"
                         % (c, l, inp[c, 0, l], inp[c, 1, l], inp[c, 2, l], got[i, c, l], want[i, c, l]))
    return lines
