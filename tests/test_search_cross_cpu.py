"""not-gpu: levenshtein_search_cross under host emulation (tests/emu_search_cross: lev_search_cross_body.h as the kernels run it -- the
[256][64] table built by 512 emulated threads, 64 lanes per wavefront with every group's own G, the candidate rule, the exact pass over
the spans, the nearest / per-haystack / finish logic, the sub-batch loop) against the oracle levenshtein_search_naive_with_opts over
EVERY (needle, haystack) pair of every batch: sorted records, count, nearest, best, per-haystack.  Plus the argument errors of
ta_levenshtein_search_cross and its refusal to run without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import datagen as Dg
import search_cross_cases as X

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_search_cross")

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(EMU_DIR, "libta_emu_search_cross.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        vp, u32, u64, i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        _lib.emu_search_cross.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, u32, u32, i, u32, i, i, u32, vp, vp, u64, vp, vp, vp, vp, vp]
        _lib.emu_search_cross.restype = i
    return _lib


def _side(strings, fill):
    """CSR blob with 16 bytes of `fill` as read slack -> (keepalive, blob address, offsets)"""
    data = b"".join(strings)
    raw = np.full(len(data) + 16, fill, np.uint8)
    raw[:len(data)] = np.frombuffer(data, np.uint8)
    off = np.zeros(len(strings) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return raw, raw.ctypes.data, off


def emu(needles, hays, k, costs, anchored=False, packed=False, sub=0, cap=None, nearest=True, best=True, per=True, spans=False):
    """-> dict(records sorted, count, nearest, best, per, spans, subs, kept) of one emulated call"""
    mc, gc, sg, t = costs
    nn, nh = len(needles), len(hays)
    nraw, naddr, noff = _side(needles, 0x5A)
    hraw, haddr, hoff = _side(hays, 0xA5)
    cap = nn * nh if cap is None else cap
    hits = np.full((max(cap, 1), 6), 7, np.uint32)
    count = np.full(1, 9, np.uint64)
    near = np.full(max(nh, 1), 9, np.uint64) if nearest else None
    bst = np.full((max(nh, 1), 6), 9, np.uint32) if best else None            # ta_match: u64 start, u64 end, u32 k, u32 pad
    cnt = np.full(max(nh, 1), 9, np.uint32) if per else None
    sp = np.full((max(nh, 1), max(nn, 1), 2), 0xFFFFFFFF, np.uint32) if spans else None
    subs = np.zeros(1, np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data                       # noqa: E731
    rc = lib().emu_search_cross(naddr, noff.ctypes.data, nn, haddr, hoff.ctypes.data, nh, k, mc, gc, sg, int(t is not None), t or 0,
                                int(anchored), int(packed), sub, ptr(hits) if cap else None, count.ctypes.data, cap, ptr(near), ptr(bst),
                                ptr(cnt), ptr(sp), subs.ctypes.data)
    assert rc == 0, ("the emulation caught", rc)
    n = int(count[0])
    kept = [tuple(int(x) for x in r) for r in hits[:min(n, cap)]]
    out = {"records": sorted(kept), "kept": kept, "count": n, "subs": int(subs[0]), "spans": sp}
    out["nearest"] = None if near is None else [int(w) for w in near[:nh]]
    out["per"] = None if cnt is None else [int(c) for c in cnt[:nh]]
    if bst is not None:
        b64 = bst[:nh].copy().view(np.uint64).reshape(nh, 3) if nh else np.zeros((0, 3), np.uint64)
        out["best"] = [(int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF) for r in b64]
        assert all(int(r[2]) >> 32 == 0 for r in b64)                          # pad_ = 0
    else:
        out["best"] = None
    return out


def check(needles, hays, k, costs, anchored=False, **kw):
    want = X.join(needles, hays, k, costs, anchored)
    got = emu(needles, hays, k, costs, anchored, **kw)
    where = (len(needles), len(hays), k, costs, anchored, kw)
    assert got["count"] == len(want[0]) and got["records"] == want[0], where
    assert got["nearest"] == want[1], where
    assert got["best"] == want[2], where
    assert got["per"] == want[3], where
    return want, got


@pytest.mark.parametrize("costs", X.COSTS)
def test_every_cost_set_anchored_and_not(costs):
    """mixed needle lengths, so that at k = 3 and k = 9 needles with kf >= n and needles with kf < n share a group"""
    total = 0
    for nn in (5, 33):
        needles = X.panel(100 + nn, nn)
        hays = X.reads(200 + nn, 40, needles)
        for anchored in (False, True):
            for k in (0, 3, 9):
                want, _ = check(needles, hays, k, costs, anchored)
                total += len(want[0])
    assert total > 100


@pytest.mark.parametrize("nn", X.PANELS)
def test_every_panel_size(nn):
    """one needle to three groups: every G (1, 2, 4, 8, 16, 32, 64), a last group with its own G, idle columns"""
    needles = X.panel(300 + nn, nn)
    hays = X.reads(400 + nn, 24, needles)
    for costs in (X.COSTS[0], X.COSTS[5]):
        for anchored in (False, True):
            want, _ = check(needles, hays, 3, costs, anchored)
            assert anchored or len(want[0]) >= 8                   # (an anchored match starts at 0: the planted ones rarely do)


@pytest.mark.parametrize("alphabet", ["acgt", "bytes"])
def test_alphabets_and_every_hit_inside_its_scanned_span(alphabet):
    al = X.ACGT if alphabet == "acgt" else X.BYTES
    needles = X.panel(500, 33, al)
    hays = X.reads(501, 48, needles, al)
    for costs in (X.COSTS[0], X.COSTS[1], X.COSTS[7]):
        for k in (2, 4):
            want, got = check(needles, hays, k, costs, spans=True)
            sp = got["spans"]
            assert (sp[:len(hays), :len(needles), 0] != 0xFFFFFFFF).all()      # the scan met every pair exactly once
            ends = 0
            for i, p, start, end, kk, n in want[0]:
                first, last = int(sp[i, p, 0]), int(sp[i, p, 1])
                if end:                                            # (the end == 0 match needs no span)
                    assert first >= 1 and first <= end <= last, (i, p, start, end, first, last)
                    ends += 1
            assert ends > 20
            # a pair the scan finished (no candidate end) has no hit
            hit = {(i, p) for i, p, *_ in want[0]}
            assert all((i, p) not in hit for i in range(len(hays)) for p in range(len(needles)) if sp[i, p, 0] == 0)


def test_duplicate_needles_tie_to_the_lower_index():
    g = Dg.rng(600)
    a, b = bytes(g.choice(X.ACGT, 20)), bytes(g.choice(X.ACGT, 24))
    needles = [b, a, a, b, a]
    hays = [bytes(g.choice(X.ACGT, 60)) + a + bytes(g.choice(X.ACGT, 60)), bytes(g.choice(X.ACGT, 150)),
            bytes(g.choice(X.ACGT, 10)) + b + bytes(g.choice(X.ACGT, 90)) + X.mutate(g, a, 1, X.ACGT)]
    want, got = check(needles, hays, 2, X.COSTS[0])
    assert got["nearest"][0] == (0 << 32 | 1) and got["per"][0] == 3
    assert got["nearest"][1] == X.ALL_ONES and got["per"][1] == 0 and got["best"][1] == (0, 0, X.NONE)
    assert got["nearest"][2] == (0 << 32 | 0) and got["per"][2] == 5 and got["best"][2] == (10, 34, 0)


def test_planted_twice_and_overlapping():
    g = Dg.rng(700)
    nd = b"ACGTTGCATGCAAGTC"
    other = bytes(g.choice(X.ACGT, 16))
    fill = lambda n: bytes(g.choice(np.frombuffer(b"T", np.uint8), n))         # noqa: E731
    twice = fill(20) + nd + fill(30) + nd + fill(20)
    rep = b"ACAC" * 4
    overlap = fill(20) + rep + b"AC" + fill(20)                    # the repeat matches at two shifts: equal cost, overlapping
    for costs in (X.COSTS[0], X.COSTS[5]):
        want, got = check([other, nd, rep], [twice, overlap], 1, costs)
        recs = {(i, p): r for r in want[0] for i, p in [r[:2]]}
        assert recs[(0, 1)][4] == 0 and recs[(0, 1)][5] == 2       # n_matches = 2
        assert (1, 2) in recs and recs[(1, 2)][4] == 0


def test_short_haystacks_and_empty_sides():
    needles = [b"", b"A", b"ACGTACGT", b"ACGTACGTA" * 3, b"C" * 32]
    hays = [b"", b"A", b"ACG", b"ACGT", b"ACGTA", b"ACGTACG", b"C" * 31]
    for costs in X.COSTS:
        for anchored in (False, True):
            for k in (0, 1, 8, 40):
                check(needles, hays, k, costs, anchored)
    for needles, hays in (([], [b"ACGT"]), ([b"ACGT"], []), ([], [])):
        got = emu(needles, hays, 2, X.COSTS[0])
        assert got["count"] == 0 and got["nearest"] == [X.ALL_ONES] * len(hays) and got["per"] == [0] * len(hays)
        assert got["best"] == [(0, 0, X.NONE)] * len(hays)


def test_packed_form_equals_the_register_form():
    g = Dg.rng(800)
    for n in (1, 7, 8, 9, 24, 32):
        needles = [bytes(g.choice(X.ACGT, n)) for _ in range(20)]
        hays = X.reads(801 + n, 24, needles)
        for costs in (X.COSTS[0], X.COSTS[5]):
            for anchored in (False, True):
                check(needles, hays, 3, costs, anchored, packed=True)


def test_forced_sub_batches_of_64_on_257_haystacks():
    needles = X.panel(900, 33)
    hays = X.reads(901, 257, needles)
    for anchored in (False, True):
        want, got = check(needles, hays, 3, X.COSTS[0], anchored, sub=64)
        assert got["subs"] == 5                                    # 64 + 64 + 64 + 64 + 1
        _, one = check(needles, hays, 3, X.COSTS[0], anchored)
        assert one["subs"] == 1 and one["records"] == got["records"]


def test_cap_cuts_the_records_not_the_count_and_optional_outputs():
    needles = X.panel(1000, 16)
    hays = X.reads(1001, 40, needles)
    want = X.join(needles, hays, 3, X.COSTS[0], False)
    assert len(want[0]) >= 40
    cap = len(want[0]) // 2
    got = emu(needles, hays, 3, X.COSTS[0], cap=cap)
    assert got["count"] == len(want[0]) and len(got["kept"]) == cap and len(set(r[:2] for r in got["kept"])) == cap
    assert set(got["kept"]) <= set(want[0])
    assert got["nearest"] == want[1] and got["best"] == want[2] and got["per"] == want[3]
    got = emu(needles, hays, 3, X.COSTS[0], cap=0)
    assert got["count"] == len(want[0]) and got["nearest"] == want[1] and got["best"] == want[2] and got["per"] == want[3]
    got = emu(needles, hays, 3, X.COSTS[0], nearest=False)         # best without nearest
    assert got["nearest"] is None and got["best"] == want[2] and got["per"] == want[3]
    got = emu(needles, hays, 3, X.COSTS[0], nearest=False, best=False, per=False)
    assert got["records"] == want[0]


# ---------------------------------------------------------------- the C ABI: argument errors come first, no CPU fallback
def _abi():
    from triple_accel_amd import _native as N
    return N


def _call(needles, nn, haystacks, nh, k=1, costs=(1, 1, 0, None), anchored=0, hits=None, count=None, cap=0, nearest=None, best=None, per=None):
    N = _abi()
    cc = None if costs is None else N.EditCostsC(costs[0], costs[1], costs[2], int(costs[3] is not None), costs[3] or 0)
    return N.lib().ta_levenshtein_search_cross(needles, nn, haystacks, nh, k, None if cc is None else C.byref(cc), anchored, hits, count, cap,
                                               nearest, best, per, None)


def test_abi_symbol_is_declared_and_exported():
    N = _abi()
    assert "ta_levenshtein_search_cross" in N.ABI_SYMBOLS and hasattr(N.lib(), "ta_levenshtein_search_cross")
    header = open(os.path.join(os.path.dirname(HERE), "include", "triple_accel_amd.h")).read()
    assert "ta_search_cross_hit" in header and "src/levenshtein.rs:1911-1966" in header and ":1693-1706" in header and ":1812-1835" in header
    assert C.sizeof(N.SearchCrossHitC) == 24


def test_abi_errors_in_their_order_before_the_device():
    N = _abi()
    blob = (C.c_uint8 * 128)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 8, 8, 0)
    S = C.byref(s)
    fake = C.c_void_p(0x1000)
    # NULL costs / needles / haystacks / count_dev
    assert _call(S, 1, S, 1, costs=None, count=fake) == N.TA_ERR_ARG
    assert _call(None, 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, None, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=None) == N.TA_ERR_ARG
    assert _call(S, 0, S, 0, count=None) == N.TA_ERR_ARG
    # then the costs: EditCosts::new and check_search, whatever else is wrong behind them
    noblob = N.StringsC(0, 0, 8, 8, 0)
    assert _call(S, 1, S, 1, costs=(0, 1, 0, None), count=fake) == N.TA_ERR_BAD_COSTS
    assert _call(C.byref(noblob), 1, S, 1, costs=(1, 0, 0, None), count=fake, cap=4) == N.TA_ERR_BAD_COSTS
    assert _call(None, 1, S, 1, costs=(0, 1, 0, None), count=fake) == N.TA_ERR_ARG       # (a NULL side comes before the costs)
    # then the blobs, the hit buffer, the overflow
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
    import torch
    N = _abi()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    blob = (C.c_uint8 * 128)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 8, 8, 0)
    count = (C.c_uint64 * 1)()
    cnt = C.cast(count, C.c_void_p)
    for anchored in (0, 1):
        for k in (0, 3, 0xFFFFFFFF):
            assert _call(C.byref(s), 1, C.byref(s), 1, k=k, anchored=anchored, count=cnt) == N.TA_ERR_HIP
    assert _call(C.byref(s), 0, C.byref(s), 4, count=cnt) == N.TA_ERR_HIP              # the outputs are initialised on the device
