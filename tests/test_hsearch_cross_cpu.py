"""not-gpu: hamming_search_cross under host emulation (tests/emu_hsearch_cross: ham_search_cross_body.h as the kernels run it -- the
[256][64] mismatch table built by 512 emulated threads and compared with ham_bits_mis column by column, 64 lanes per wavefront with every
group's own G, the step loop over several haystacks per wavefront, the bit-sliced counters with every plane count, the online Best
fold, the fused NUL scan, the ballot-ordered append, the packed minimum word and the finish) against the oracle
hamming_search_simd_with_opts(.., Best) over EVERY (needle, haystack) pair of every batch: sorted records, count, nearest, best,
per-haystack.  Plus the conditions the GPU tests rely on, asserted on the oracle join alone, the argument errors of
ta_hamming_search_cross and its refusal to run without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import datagen as Dg
import hsearch_cross_cases as X

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_hsearch_cross")
NHS = (1, 63, 64, 65, 257)

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(EMU_DIR, "libta_emu_hsearch_cross.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        _lib.emu_hsearch_cross.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, vp, vp, u64, vp, vp, vp, vp, vp, vp]
        _lib.emu_hsearch_cross.restype = C.c_int
    return _lib


def _side(strings, fill):
    """CSR blob with 16 bytes of `fill` as read slack -> (keepalive, blob address, offsets)"""
    data = b"".join(strings)
    raw = np.full(len(data) + 16, fill, np.uint8)
    raw[:len(data)] = np.frombuffer(data, np.uint8)
    off = np.zeros(len(strings) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return raw, raw.ctypes.data, off


def emu(needles, hays, k, hpw=0, cap=None, nearest=True, best=True, per=True, seen=False):
    """-> dict(records sorted, kept, count, nearest, best, per, seen, planes, steps) of one emulated call"""
    nn, nh = len(needles), len(hays)
    nraw, naddr, noff = _side(needles, 0x00)                                   # (NUL bytes around the strings are nobody's)
    hraw, haddr, hoff = _side(hays, 0x00)
    cap = nn * nh if cap is None else cap
    hits = np.full((max(cap, 1), 6), 7, np.uint32)
    count = np.full(1, 9, np.uint64)
    near = np.full(max(nh, 1), 9, np.uint64) if nearest else None
    bst = np.full((max(nh, 1), 6), 9, np.uint32) if best else None            # ta_match: u64 start, u64 end, u32 k, u32 pad
    cnt = np.full(max(nh, 1), 9, np.uint32) if per else None
    sn = np.zeros((max(nh, 1), max(nn, 1)), np.uint32) if seen else None
    planes, steps = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data                       # noqa: E731
    rc = lib().emu_hsearch_cross(naddr, noff.ctypes.data, nn, haddr, hoff.ctypes.data, nh, k, hpw, ptr(hits) if cap else None,
                                 count.ctypes.data, cap, ptr(near), ptr(bst), ptr(cnt), ptr(sn), planes.ctypes.data, steps.ctypes.data)
    assert rc == 0, ("the emulation caught", rc)
    n = int(count[0])
    kept = [tuple(int(x) for x in r) for r in hits[:min(n, cap)]]
    out = {"records": sorted(kept), "kept": kept, "count": n, "planes": int(planes[0]), "steps": int(steps[0]), "seen": sn}
    out["nearest"] = None if near is None else [int(w) for w in near[:nh]]
    out["per"] = None if cnt is None else [int(c) for c in cnt[:nh]]
    if bst is not None:
        b64 = bst[:nh].copy().view(np.uint64).reshape(nh, 3) if nh else np.zeros((0, 3), np.uint64)
        out["best"] = [(int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF) for r in b64]
        assert all(int(r[2]) >> 32 == 0 for r in b64)                          # pad_ = 0
    else:
        out["best"] = None
    return out


def check(needles, hays, k, **kw):
    want = X.join(needles, hays, k)
    got = emu(needles, hays, k, **kw)
    where = (len(needles), len(hays), k, kw)
    assert got["count"] == len(want[0]) and got["records"] == want[0], where
    assert got["nearest"] == want[1], where
    assert got["best"] == want[2], where
    assert got["per"] == want[3], where
    if needles and hays:
        assert got["planes"] == X.planes(k, needles), where
    return want, got


def std():
    """the batch most GPU tests share: 33 needles of every length but one byte (one group, G = 64, 31 idle columns), 257 reads"""
    needles = X.panel(900, 33, lens=X.STD_LENS)
    return needles, X.reads(901, 257, needles)


@pytest.mark.parametrize("nn", X.PANELS)
def test_every_panel_size_read_count_and_k(nn):
    """one needle to three groups: every G (1, 2, 4, 8, 16, 32, 64), a last group with its own G, idle columns; read counts on both
    sides of the wavefront edge; every plane count, k >= n for the short needles of a mixed group, k above every needle.  The forced
    haystacks per workgroup make a wavefront walk three or more haystacks, the last step ragged"""
    needles = X.panel(300 + nn, nn)
    seen_planes, total = set(), 0
    for nh in NHS:
        hays = X.reads(400 + nn + nh, nh, needles)
        G = 1
        while G < min(nn, 64):
            G <<= 1
        per_step = 8 * (64 // G)                                   # haystacks a workgroup takes per step
        for k in X.KS:
            hpw = min(nh, 3 * per_step + 1)                        # three full steps and one haystack more, or one ragged workgroup
            want, got = check(needles, hays, k, hpw=hpw, seen=(k == 2))
            assert got["steps"] >= (4 if hpw > 3 * per_step else 1)
            if k == 2:
                assert (got["seen"][:nh, :nn] == 1).all()          # the scan met every pair exactly once
            seen_planes.add(got["planes"])
            total += len(want[0])
    assert total > 0
    assert seen_planes >= ({1, 2, 3, 4, 5, 6} if max(len(x) for x in needles) == 32 else {1, 2, 3})


@pytest.mark.parametrize("alphabet", ["acgt", "bytes"])
def test_alphabets(alphabet):
    al = X.ACGT if alphabet == "acgt" else X.BYTES
    needles = X.panel(500, 33, al)
    hays = X.reads(501, 99, needles, al)
    for k in (0, 2, 5, 33):
        want, _ = check(needles, hays, k, hpw=40)
        assert len(want[0]) >= 20


def test_the_conditions_the_gpu_tests_rely_on():
    """asserted on the oracle join alone: the standard batch at k = 2 holds every case the comparisons are about"""
    needles, hays = std()
    recs, nearest, best, per = X.join(needles, hays, 2)
    assert all(any(r[4] == d for r in recs) for d in (0, 1, 2))    # a hit at each distance
    assert any(r[5] >= 2 for r in recs)                            # several windows at the minimum
    ties = 0
    for i in range(len(hays)):
        row = [r for r in recs if r[0] == i]
        if row:
            kmin = min(r[4] for r in row)
            tied = [r[1] for r in row if r[4] == kmin]
            if len(tied) >= 2:
                ties += 1
                assert nearest[i] == (kmin << 32 | min(tied))      # the tie goes to the lower index
    assert ties >= 1
    assert any(c == 0 for c in per)                                # a haystack with no hit
    nul = [i for i, h in enumerate(hays) if 0 in h]
    longest_short = min(len(nd) for nd in needles if nd)
    assert any(per[i] == X.NONE for i in nul)                      # a NUL haystack marked ...
    assert any(per[i] == 0 and len(hays[i]) < longest_short for i in nul)      # ... and one shorter than every non-empty needle: not marked
    assert all(per[i] in (0, X.NONE) and nearest[i] == X.ALL_ONES and best[i] == (0, 0, X.NONE) for i in nul)
    assert len(recs) >= 64                                         # (the cap test halves them)
    # overlapping windows at the same count are both kept: there is no fold
    assert any(r[5] >= 2 and len(needles[r[1]]) > 3 and X._period(needles[r[1]]) for r in recs)
    want, got = check(needles, hays, 2)
    assert got["planes"] == 2


def test_planted_twice_overlapping_and_k_above_the_needle():
    g = Dg.rng(700)
    nd = b"ACGTTGCATGCAAGTC"
    other = bytes(g.choice(X.ACGT, 16))
    fill = lambda n: b"T" * n                                      # noqa: E731
    twice = fill(20) + nd + fill(30) + nd + fill(20)
    rep = b"ACAC" * 4
    overlap = fill(20) + rep + b"AC" + fill(20)                    # the repeat matches at two shifts: equal count, overlapping, both kept
    want, _ = check([other, nd, rep], [twice, overlap], 1)
    recs = {(r[0], r[1]): r for r in want[0]}
    assert recs[(0, 1)][2:] == (20, 36, 0, 2)                      # n_matches = 2
    assert recs[(1, 2)][2:] == (20, 36, 0, 2)
    # k >= n: every window is a candidate, Best reports the windows at the minimum -- all h - n + 1 of them in a constant read
    want, _ = check([b"GG", b"T", b""], [fill(50)], 7)
    recs = {(r[0], r[1]): r for r in want[0]}
    assert recs[(0, 0)][2:] == (0, 2, 2, 49) and recs[(0, 1)][2:] == (0, 1, 0, 50) and (0, 2) not in recs


def test_duplicate_needles_tie_to_the_lower_index():
    g = Dg.rng(600)
    a, b = bytes(g.choice(X.ACGT, 20)), bytes(g.choice(X.ACGT, 24))
    needles = [b, a, a, b, a]
    hays = [bytes(g.choice(X.ACGT, 60)) + a + bytes(g.choice(X.ACGT, 60)), bytes(g.choice(X.ACGT, 150)),
            bytes(g.choice(X.ACGT, 10)) + b + bytes(g.choice(X.ACGT, 90)) + X.substitute(g, a, 1, X.ACGT)]
    want, got = check(needles, hays, 2)
    assert got["nearest"][0] == (0 << 32 | 1) and got["per"][0] == 3 and got["best"][0] == (60, 80, 0)
    assert got["nearest"][1] == X.ALL_ONES and got["per"][1] == 0 and got["best"][1] == (0, 0, X.NONE)
    assert got["nearest"][2] == (0 << 32 | 0) and got["per"][2] == 5 and got["best"][2] == (10, 34, 0)


def test_the_nul_rule_keeps_the_reference_order():
    needles = [b"", b"ACGTACGT", b"AC\x00T", b"C" * 32]            # (a NUL in a needle is an ordinary byte)
    hays = [b"", b"\x00", b"A\x00C", b"AC\x00T", b"ACGTAC\x00T", b"ACGTACGT\x00", b"C" * 31 + b"\x00", b"C" * 32 + b"\x00", b"ACGTACGT"]
    for k in (0, 1, 4, 40):
        want, got = check(needles, hays, k)
        # shorter than every non-empty needle: not marked; else marked, whatever the needles are
        assert got["per"][:3] == [0, 0, 0] and got["per"][3:8] == [X.NONE] * 5 and got["per"][8] >= 1
        assert all(r[0] == 8 for r in want[0])
    for needles, hays in (([], [b"ACGT", b"A\x00"]), ([b"ACGT"], []), ([], []), ([b""], [b"\x00\x00", b"ACGT"])):
        got = emu(needles, hays, 2)
        assert got["count"] == 0 and got["nearest"] == [X.ALL_ONES] * len(hays) and got["per"] == [0] * len(hays)
        assert got["best"] == [(0, 0, X.NONE)] * len(hays)


def test_short_haystacks():
    needles = [b"", b"A", b"ACGTACGT", b"ACGTACGTA" * 3, b"C" * 32]
    hays = [b"", b"A", b"ACG", b"ACGT", b"ACGTA", b"ACGTACG", b"C" * 31, b"C" * 32, b"C" * 33]
    for k in X.KS:
        check(needles, hays, k)


def test_forced_haystacks_per_workgroup_equal_the_unforced_result():
    needles, hays = std()
    _, one = check(needles, hays, 2)
    assert one["steps"] == 1
    for hpw in (1, 7, 100, 257):
        _, got = check(needles, hays, 2, hpw=hpw)
        assert got["records"] == one["records"] and got["steps"] == (hpw + 7) // 8


def test_cap_cuts_the_records_not_the_count_and_optional_outputs():
    needles, hays = std()
    want = X.join(needles, hays, 2)
    cap = len(want[0]) // 2
    got = emu(needles, hays, 2, cap=cap)
    assert got["count"] == len(want[0]) and len(got["kept"]) == cap and len(set(r[:2] for r in got["kept"])) == cap
    assert set(got["kept"]) <= set(want[0])
    assert got["nearest"] == want[1] and got["best"] == want[2] and got["per"] == want[3]
    got = emu(needles, hays, 2, cap=0)
    assert got["count"] == len(want[0]) and got["nearest"] == want[1] and got["best"] == want[2] and got["per"] == want[3]
    got = emu(needles, hays, 2, nearest=False)                     # best without nearest
    assert got["nearest"] is None and got["best"] == want[2] and got["per"] == want[3]
    got = emu(needles, hays, 2, best=False)
    assert got["nearest"] == want[1] and got["best"] is None
    got = emu(needles, hays, 2, nearest=False, best=False, per=False)
    assert got["records"] == want[0]


# ---------------------------------------------------------------- the C ABI: argument errors come first, no CPU fallback
def _abi():
    from triple_accel_amd import _native as N
    return N


def _call(needles, nn, haystacks, nh, k=1, hits=None, count=None, cap=0, nearest=None, best=None, per=None):
    return _abi().lib().ta_hamming_search_cross(needles, nn, haystacks, nh, k, hits, count, cap, nearest, best, per, None)


def test_abi_symbol_is_declared_and_exported():
    N = _abi()
    assert "ta_hamming_search_cross" in N.ABI_SYMBOLS and hasattr(N.lib(), "ta_hamming_search_cross")
    header = open(os.path.join(os.path.dirname(HERE), "include", "triple_accel_amd.h")).read()
    at = header.index("int ta_hamming_search_cross(")
    comment = header[header.rindex("/*", 0, at):at]
    assert "src/hamming.rs:454-475" in comment and ":96-146" in comment and "per_haystack_dev" in comment and "0x00" in comment


def test_abi_errors_in_their_order_before_the_device():
    N = _abi()
    blob = (C.c_uint8 * 128)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 8, 8, 0)
    S = C.byref(s)
    fake = C.c_void_p(0x1000)
    # NULL needles / haystacks / count_dev
    assert _call(None, 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, None, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=None) == N.TA_ERR_ARG
    assert _call(S, 0, S, 0, count=None) == N.TA_ERR_ARG
    # then the blobs, the hit buffer, the overflow
    noblob = N.StringsC(0, 0, 8, 8, 0)
    assert _call(C.byref(noblob), 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, C.byref(noblob), 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=fake, cap=4, hits=None) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=fake, cap=1 << 60, hits=fake) == N.TA_ERR_ARG
    # an argument error wins over an unsupported length
    long_needle = N.StringsC(ptr, 0, 33, 33, 0)
    assert _call(C.byref(long_needle), 1, S, 1, count=fake, cap=4, hits=None) == N.TA_ERR_ARG
    # then the limits
    assert _call(C.byref(long_needle), 1, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED
    long_csr_needle = N.StringsC(ptr, 0x1000, 0, 0, 33)
    assert _call(C.byref(long_csr_needle), 1, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED
    assert _call(S, 65536, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED
    huge = N.StringsC(ptr, 0, 1 << 32, 1 << 32, 0)
    assert _call(S, 1, C.byref(huge), 1, count=fake) == N.TA_ERR_UNSUPPORTED
    huge_csr = N.StringsC(ptr, 0x1000, 0, 0, 1 << 32)
    assert _call(S, 1, C.byref(huge_csr), 1, count=fake) == N.TA_ERR_UNSUPPORTED
    assert _call(S, 1, S, 1 << 32, count=fake) == N.TA_ERR_UNSUPPORTED


def test_no_cpu_fallback():
    """without a device the entry answers TA_ERR_HIP, the empty call included: its outputs are initialised on the device"""
    import torch
    N = _abi()
    blob = (C.c_uint8 * 128)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 8, 8, 0)
    count = (C.c_uint64 * 1)()
    cnt = C.cast(count, C.c_void_p)
    if not torch.cuda.is_available():
        for k in (0, 3, 0xFFFFFFFF):
            assert _call(C.byref(s), 1, C.byref(s), 1, k=k, count=cnt) == N.TA_ERR_HIP
        assert _call(C.byref(s), 0, C.byref(s), 4, count=cnt) == N.TA_ERR_HIP
    from triple_accel_amd import batch as B
    assert callable(B.hamming_search_cross)
