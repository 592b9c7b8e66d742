"""not-gpu: hamming_search_cross_with_opts' two-word route under host emulation (tests/emu_hsearch_cross_w2: ham_bits2_body.h and
ham_search_cross_w2_body.h as the kernel runs them -- the [256][32] table of two-word entries built by 512 emulated threads and compared
with ham_bits2_mis column by column, 64 lanes per wavefront with every group's own G, two haystacks or more per step, the two-word
counters with every plane count 1..7, the online Best fold from the high words, the fused NUL scan, the ballot-ordered append, the packed
minimum word and the finish) against the oracle hamming_search_simd_with_opts(.., Best) over EVERY (needle, haystack) pair of every
batch.  Plus the counters alone against a byte loop, the hand-made pairs around the word boundary, the conditions the GPU tests rely on
(asserted on the oracle join alone), the agreement of short needles in a long panel with the one-word emulation, the argument errors of
ta_hamming_search_cross_with_opts and its refusal to run without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import datagen as Dg
import hsearch_cross_opts_cases as Y

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_hsearch_cross_w2")
NHS = (1, 2, 65, 257)

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(EMU_DIR, "libta_emu_hsearch_cross_w2.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        _lib.emu_hsearch_cross_w2.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, vp, vp, u64, vp, vp, vp, vp, vp, vp]
        _lib.emu_hsearch_cross_w2.restype = C.c_int
        _lib.emu_ham_bits2_windows.argtypes = [vp, u32, vp, u32, u32, vp, vp]
        _lib.emu_ham_bits2_windows.restype = C.c_int
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
    rc = lib().emu_hsearch_cross_w2(naddr, noff.ctypes.data, nn, haddr, hoff.ctypes.data, nh, k, hpw, ptr(hits) if cap else None,
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
    want = Y.join(needles, hays, k)
    got = emu(needles, hays, k, **kw)
    where = (len(needles), len(hays), k, kw)
    assert got["count"] == len(want[0]) and got["records"] == want[0], where
    assert got["nearest"] == want[1], where
    assert got["best"] == want[2], where
    assert got["per"] == want[3], where
    if needles and hays:
        assert got["planes"] == Y.planes(k, needles), where
    return want, got


# ---------------------------------------------------------------- the counters alone
@pytest.mark.parametrize("n", [1, 31, 32, 33, 34, 63, 64])
def test_ham_bits2_against_a_byte_loop(n):
    """bit 63 of OV and the count from the planes' high words at every window of a 200-byte haystack, for every plane count the
    threshold can take; the haystack holds the needle with 0..n substitutions in turn, so that counts on both sides of k occur"""
    g = Dg.rng(2000 + n)
    needle = bytes(g.choice(Y.ACGT, n))
    hay = bytearray(g.choice(Y.ACGT, 200))
    at = 3
    for d in (0, 1, 2, 3, 8, 31, 33, n):                           # planted copies with d substitutions (clamped), back to back
        if at + n > 200:
            break
        hay[at:at + n] = Y.substitute(g, needle, min(d, n), Y.ACGT)
        at += n + 1
    hay = bytes(hay)
    nd, hy = np.frombuffer(needle, np.uint8).copy(), np.frombuffer(hay, np.uint8).copy()
    seen_planes, below = set(), 0
    for k in sorted({min(k, n) for k in (0, 1, 2, 3, 7, 8, 31, 32, 33, 63, 64)}):
        over, count = np.full(200, 7, np.uint8), np.full(200, 7, np.uint32)
        B = lib().emu_ham_bits2_windows(nd.ctypes.data, n, hy.ctypes.data, 200, k, over.ctypes.data, count.ctypes.data)
        assert B == next(b for b in range(1, 8) if (1 << b) - 1 >= k)
        seen_planes.add(B)
        for i in range(200):
            if i + 1 < n:
                assert over[i] == 1, (n, k, i)                     # fewer than n bytes consumed: nobody's window
                continue
            mism = sum(1 for j in range(n) if hay[i + 1 - n + j] != needle[j])
            assert over[i] == (1 if mism > k else 0), (n, k, i, mism)
            if mism <= k:
                assert count[i] == mism, (n, k, i)
                below += 1
    assert below > 0 and (n < 64 or seen_planes == {1, 2, 3, 4, 5, 6, 7})


# ---------------------------------------------------------------- the whole call
@pytest.mark.parametrize("nn", Y.PANELS)
def test_every_panel_size_read_count_and_k(nn):
    """one needle to three groups of 32: G = 1, 8, 32, a last group of one needle, idle columns; read counts from one to several steps;
    every plane count 1..7; k >= n for the short needles of a mixed group, k above every needle.  The forced haystacks per workgroup
    make a wavefront walk three steps and one haystack more, the last step ragged"""
    needles = Y.panel(300 + nn, nn)
    longest = max(len(x) for x in needles)
    seen_planes, total = set(), 0
    for nh in NHS:
        hays = Y.reads(400 + nn + nh, nh, needles)
        G = 1
        while G < min(nn, 32):
            G <<= 1
        per_step = 8 * (64 // G)                                   # haystacks a workgroup takes per step
        for k in Y.KS:
            hpw = min(nh, 3 * per_step + 1)
            want, got = check(needles, hays, k, hpw=hpw, seen=(k == 3))
            assert got["steps"] >= (4 if hpw > 3 * per_step else 1)
            if k == 3:
                assert (got["seen"][:nh, :nn] == 1).all()          # the scan met every pair exactly once
            if longest == 64:
                assert got["planes"] == Y.PLANES_AT_64[k], (k, got["planes"])
            seen_planes.add(got["planes"])
            total += len(want[0])
    assert total > 0
    assert longest < 64 or seen_planes == {1, 2, 3, 4, 5, 6, 7} - {3}
    if longest == 64:                                              # B = 3 is no k of the list: one more call
        _, got = check(needles, Y.reads(400 + nn, 65, needles), 5)
        assert got["planes"] == 3


def test_bytes_alphabet():
    needles = Y.panel(500, 33, Y.BYTES)
    hays = Y.reads(501, 99, needles, Y.BYTES)
    for k in (0, 2, 5, 40):
        want, _ = check(needles, hays, k, hpw=40)
        assert len(want[0]) >= 20


def test_hand_made_pairs_around_the_word_boundary():
    cases = Y.hand_made()
    assert {len(c[1]) for c in cases} == {33, 64}
    for tag, nd, hay, k, want in cases:                            # on the oracle alone ...
        recs = Y.join([nd], [hay], k)[0]
        assert recs == ([] if want is None else [(0, 0) + want]), tag
        assert 0 <= len(hay) - len(nd)
    ends = [c for c in cases if c[0].startswith("ends")]
    for tag, nd, hay, k, want in ends:                             # (one window at offset 0, one ending on the last byte)
        assert hay[:len(nd)] == nd and hay[-len(nd):] == nd and want[3] == 2
    for tag, nd, hay, k, want in cases:                            # ... then through the emulation, alone
        w, got = check([nd], [hay], k)
        assert got["records"] == ([] if want is None else [(0, 0) + want]), tag
    for k in sorted({c[3] for c in cases}):                        # ... and every needle against every haystack in one panel
        check([c[1] for c in cases[::7]] + [b"ACGT"], [c[2] for c in cases], k)


def test_the_conditions_the_gpu_tests_rely_on():
    """asserted on the oracle join alone: the standard batch at k = 3 holds every case the comparisons are about"""
    needles, hays = Y.std()
    assert len(needles) == 33 and max(map(len, needles)) == 64
    recs, nearest, best, per = Y.join(needles, hays, 3)
    is_long = lambda r: len(needles[r[1]]) > 32                    # noqa: E731
    assert all(any(r[4] == d and is_long(r) for r in recs) for d in (0, 1, 2, 3))   # a hit at each distance for a needle beyond 32 bytes
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
    shortest = min(len(nd) for nd in needles if nd)
    assert any(per[i] == Y.NONE for i in nul)                      # a NUL haystack marked ...
    assert any(per[i] == 0 and len(hays[i]) < shortest for i in nul)           # ... and one shorter than every non-empty needle: not marked
    assert all(per[i] in (0, Y.NONE) and nearest[i] == Y.ALL_ONES and best[i] == (0, 0, Y.NONE) for i in nul)
    assert len(recs) >= 64                                         # (the cap test halves them)
    # overlapping windows at the same count are both kept: there is no fold
    import hsearch_cross_cases as X
    assert any(r[5] >= 2 and is_long(r) and X._period(needles[r[1]]) for r in recs)
    want, got = check(needles, hays, 3)
    assert got["planes"] == 2


def test_short_needles_in_a_long_panel_equal_the_one_word_emulation():
    import hsearch_cross_cases as X
    import test_hsearch_cross_cpu as One
    short = X.panel(910, 40)                                       # needles of 0..32 bytes
    assert max(map(len, short)) == 32
    hays = X.reads(911, 130, short)
    g = Dg.rng(912)
    long_panel = short + [bytes(g.choice(X.ACGT, 40))]
    for k in (0, 2, 9, 31, 32, 40):
        one = One.emu(short, hays, k)
        two = emu(long_panel, hays, k)
        assert [r for r in two["records"] if r[1] < len(short)] == one["records"], k
        assert len(one["records"]) > 0
        assert two["planes"] == Y.planes(k, long_panel)


def test_the_nul_rule_and_short_haystacks():
    needles = [b"", b"ACGTACGT", b"AC\x00T" * 9, b"C" * 64, b"G" * 33]            # (a NUL in a needle is an ordinary byte)
    hays = [b"", b"\x00", b"A\x00C", b"ACGTAC\x00T", b"C" * 63 + b"\x00", b"C" * 64 + b"\x00", b"C" * 63, b"C" * 64, b"C" * 65, b"G" * 32, b"G" * 33,
            b"AC\x00T" * 9]
    for k in (0, 1, 4, 40, 70):
        want, got = check(needles, hays, k)
        assert got["per"][:3] == [0, 0, 0] and got["per"][3:6] == [Y.NONE] * 3 and got["per"][11] == Y.NONE
    for needles, hays in (([], [b"ACGT", b"A\x00"]), ([b"ACGT" * 10], []), ([], []), ([b""], [b"\x00\x00", b"ACGT"])):
        got = emu(needles, hays, 2)
        assert got["count"] == 0 and got["nearest"] == [Y.ALL_ONES] * len(hays) and got["per"] == [0] * len(hays)
        assert got["best"] == [(0, 0, Y.NONE)] * len(hays)


def test_forced_haystacks_per_workgroup_equal_the_unforced_result():
    needles, hays = Y.std()
    _, one = check(needles, hays, 3)
    for hpw in (1, 7, 100, len(hays)):
        _, got = check(needles, hays, 3, hpw=hpw)
        assert got["records"] == one["records"] and got["steps"] == (hpw + 15) // 16          # 8 wavefronts of two haystacks per step


def test_cap_cuts_the_records_not_the_count_and_optional_outputs():
    needles, hays = Y.std()
    want = Y.join(needles, hays, 3)
    cap = len(want[0]) // 2
    got = emu(needles, hays, 3, cap=cap)
    assert got["count"] == len(want[0]) and len(got["kept"]) == cap and len(set(r[:2] for r in got["kept"])) == cap
    assert set(got["kept"]) <= set(want[0])
    assert got["nearest"] == want[1] and got["best"] == want[2] and got["per"] == want[3]
    got = emu(needles, hays, 3, cap=0)
    assert got["count"] == len(want[0]) and got["nearest"] == want[1] and got["best"] == want[2] and got["per"] == want[3]
    got = emu(needles, hays, 3, nearest=False)                     # best without nearest
    assert got["nearest"] is None and got["best"] == want[2] and got["per"] == want[3]
    got = emu(needles, hays, 3, best=False)
    assert got["nearest"] == want[1] and got["best"] is None
    got = emu(needles, hays, 3, nearest=False, best=False, per=False)
    assert got["records"] == want[0]


# ---------------------------------------------------------------- the C ABI: argument errors come first, no CPU fallback
def _abi():
    from triple_accel_amd import _native as N
    return N


def _call(needles, nn, haystacks, nh, k=1, flags=0, hits=None, count=None, cap=0, nearest=None, best=None, per=None):
    return _abi().lib().ta_hamming_search_cross_with_opts(needles, nn, haystacks, nh, k, flags, hits, count, cap, nearest, best, per, None)


def test_abi_symbol_is_declared_and_exported():
    N = _abi()
    assert "ta_hamming_search_cross_with_opts" in N.ABI_SYMBOLS and hasattr(N.lib(), "ta_hamming_search_cross_with_opts")
    header = open(os.path.join(os.path.dirname(HERE), "include", "triple_accel_amd.h")).read()
    at = header.index("int ta_hamming_search_cross_with_opts(")
    comment = header[header.rindex("/*", 0, at):at]
    assert "src/hamming.rs:454-475" in comment and ":96-146" in comment and "flags" in comment and "64 bytes" in comment
    assert "ham_search_cross_w2_kernel<B>" in comment and "pay" in comment
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    assert callable(B.hamming_search_cross_with_opts)
    assert callable(T.hamming_search_cross_with_opts_many) and callable(T.hamming_search_nearest_with_opts_many)


def test_abi_errors_in_their_order_before_the_device():
    N = _abi()
    blob = (C.c_uint8 * 128)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 8, 8, 0)
    S = C.byref(s)
    fake = C.c_void_p(0x1000)
    # NULL needles / haystacks / count_dev: before the flags
    assert _call(None, 1, S, 1, count=fake, flags=1) == N.TA_ERR_ARG
    assert _call(S, 1, None, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=None) == N.TA_ERR_ARG
    assert _call(S, 0, S, 0, count=None) == N.TA_ERR_ARG
    # then the flags word: reserved, every bit
    too_long = N.StringsC(ptr, 0, 65, 65, 0)
    for bit in (0, 1, 31):
        assert _call(S, 1, S, 1, count=fake, flags=1 << bit) == N.TA_ERR_ARG
        assert _call(C.byref(too_long), 1, S, 1, count=fake, flags=1 << bit) == N.TA_ERR_ARG        # (wins over an unsupported length)
    # then the blobs, the hit buffer, the overflow
    noblob = N.StringsC(0, 0, 8, 8, 0)
    assert _call(C.byref(noblob), 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, C.byref(noblob), 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=fake, cap=4, hits=None) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=fake, cap=1 << 60, hits=fake) == N.TA_ERR_ARG
    assert _call(C.byref(too_long), 1, S, 1, count=fake, cap=4, hits=None) == N.TA_ERR_ARG
    # then the limits: 65 bytes, not 33
    assert _call(C.byref(too_long), 1, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED
    long_csr_needle = N.StringsC(ptr, 0x1000, 0, 0, 65)
    assert _call(C.byref(long_csr_needle), 1, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED
    assert _call(S, 65536, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED
    huge = N.StringsC(ptr, 0, 1 << 32, 1 << 32, 0)
    assert _call(S, 1, C.byref(huge), 1, count=fake) == N.TA_ERR_UNSUPPORTED
    huge_csr = N.StringsC(ptr, 0x1000, 0, 0, 1 << 32)
    assert _call(S, 1, C.byref(huge_csr), 1, count=fake) == N.TA_ERR_UNSUPPORTED
    assert _call(S, 1, S, 1 << 32, count=fake) == N.TA_ERR_UNSUPPORTED
    # ta_hamming_search_cross keeps its own limit
    n33 = N.StringsC(ptr, 0, 33, 33, 0)
    assert N.lib().ta_hamming_search_cross(C.byref(n33), 1, S, 1, 1, None, fake, 0, None, None, None, None) == N.TA_ERR_UNSUPPORTED


def test_no_cpu_fallback():
    """without a device the entry answers TA_ERR_HIP, the empty call and a 64-byte needle included"""
    import torch
    N = _abi()
    blob = (C.c_uint8 * 256)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 8, 8, 0)
    n64 = N.StringsC(ptr, 0, 64, 64, 0)
    h = N.StringsC(ptr, 0, 100, 100, 0)
    count = (C.c_uint64 * 1)()
    cnt = C.cast(count, C.c_void_p)
    if not torch.cuda.is_available():
        for k in (0, 3, 0xFFFFFFFF):
            assert _call(C.byref(s), 1, C.byref(s), 1, k=k, count=cnt) == N.TA_ERR_HIP
            assert _call(C.byref(n64), 1, C.byref(h), 1, k=k, count=cnt) == N.TA_ERR_HIP
        assert _call(C.byref(s), 0, C.byref(s), 4, count=cnt) == N.TA_ERR_HIP
