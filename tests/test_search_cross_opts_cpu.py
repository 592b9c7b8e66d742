"""not-gpu: levenshtein_search_cross_with_opts' two-word route under host emulation (tests/emu_search_cross_w2:
lev_search_cross_w2_body.h as the kernels run it -- the [256][32][2] table built by 512 emulated threads and compared with
lev_filter_peq_word, 64 lanes per wavefront with every group's own G, the candidate list in ballot order, the exact pass over the spans
with its column in memory, the nearest / per-haystack / finish logic, the sub-batch loop) against the oracle
levenshtein_search_naive_with_opts over EVERY (needle, haystack) pair of every batch: sorted records, count, nearest, best,
per-haystack.  Plus the host rules of ta_levenshtein_search_cross_with_opts without a device: the error order, the flags word, the
64-byte limit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import search_cross_cases as X
import search_cross_opts_cases as Y

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_search_cross_w2")

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(EMU_DIR, "libta_emu_search_cross_w2.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        vp, u32, u64, i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        _lib.emu_search_cross_w2.argtypes = [vp, vp, u32, vp, vp, u32, u32, u32, u32, u32, i, u32, i, u32, vp, vp, u64, vp, vp, vp, vp, vp]
        _lib.emu_search_cross_w2.restype = i
        _lib.emu_search_cross_w2_lanes.argtypes = [u64]
        _lib.emu_search_cross_w2_lanes.restype = u32
    return _lib


def _side(strings, fill):
    """CSR blob with 16 bytes of `fill` as read slack -> (keepalive, blob address, offsets)"""
    data = b"".join(strings)
    raw = np.full(len(data) + 16, fill, np.uint8)
    raw[:len(data)] = np.frombuffer(data, np.uint8)
    off = np.zeros(len(strings) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return raw, raw.ctypes.data, off


def emu(needles, hays, k, costs, anchored=False, sub=0, cap=None, nearest=True, best=True, per=True, spans=False):
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
    rc = lib().emu_search_cross_w2(naddr, noff.ctypes.data, nn, haddr, hoff.ctypes.data, nh, k, mc, gc, sg, int(t is not None), t or 0,
                                   int(anchored), sub, ptr(hits) if cap else None, count.ctypes.data, cap, ptr(near), ptr(bst),
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


@pytest.mark.parametrize("nn", Y.PANELS)
def test_every_panel_size(nn):
    """one needle to three groups of 32: every G (1, 2, 4, 8, 16, 32), a last group with its own G, idle columns; 65 haystacks"""
    needles = Y.panel(300 + nn, nn)
    assert max(map(len, needles)) > 32                             # (the library would take the two-word route)
    hays = X.reads(400 + nn, 65, needles)
    for costs, k in ((Y.LEVENSHTEIN, 2), (Y.RDAMERAU, 5), (X.COSTS[5], 5)):
        for anchored in (False, True):
            want, _ = check(needles, hays, k, costs, anchored)
            assert anchored or len(want[0]) >= 8                   # (an anchored match starts at 0: the planted ones rarely do)


@pytest.mark.parametrize("k", [0, 2, 5, 40])
@pytest.mark.parametrize("nn", [33, 96])
def test_257_haystacks_every_k(nn, k):
    """at k = 40 the needles of up to 40 bytes are unscanned (kf >= n) beside scanned long ones in one group"""
    needles = Y.panel(500 + nn, nn)
    hays = X.reads(600 + nn, 257, needles)
    for costs in (Y.LEVENSHTEIN, Y.RDAMERAU):
        want, _ = check(needles, hays, k, costs)
        assert len(want[0]) > 30
    check(needles, hays, k, Y.LEVENSHTEIN, True)


@pytest.mark.parametrize("costs", X.COSTS)
def test_every_cost_set_anchored_and_not(costs):
    needles = Y.panel(133, 33)
    hays = X.reads(233, 65, needles)
    total = 0
    for anchored in (False, True):
        for k in (0, 2, 5, 40):
            want, _ = check(needles, hays, k, costs, anchored)
            total += len(want[0])
    assert total > 100


@pytest.mark.parametrize("alphabet", ["acgt", "zero", "zero_0c", "bytes"])
def test_alphabets_and_every_hit_inside_its_scanned_span(alphabet):
    al = {"acgt": X.ACGT, "zero": Y.ZERO, "zero_0c": Y.ZERO_0C, "bytes": X.BYTES}[alphabet]
    needles = Y.panel(700, 33, al)
    hays = X.reads(701, 65, needles, al)
    for costs in (Y.LEVENSHTEIN, Y.RDAMERAU, X.COSTS[7]):
        for k in (2, 5):
            want, got = check(needles, hays, k, costs, spans=True)
            sp = got["spans"]
            assert (sp[:len(hays), :len(needles), 0] != 0xFFFFFFFF).all()      # the scan met every pair exactly once
            for i, p, start, end, kk, n in want[0]:
                first, last = int(sp[i, p, 0]), int(sp[i, p, 1])
                if end:                                            # (the end == 0 match needs no span)
                    assert first >= 1 and first <= end <= last, (i, p, start, end, first, last)
            hit = {(i, p) for i, p, *_ in want[0]}                 # a pair the scan finished (no candidate end) has no hit
            assert all((i, p) not in hit for i in range(len(hays)) for p in range(len(needles)) if sp[i, p, 0] == 0)
            assert len(want[0]) > 20


def test_hand_made_pairs_where_two_words_can_go_wrong():
    needles, hays = Y.hand_made()
    for costs in (Y.LEVENSHTEIN, Y.RDAMERAU, X.COSTS[5]):
        for anchored in (False, True):
            for k in (0, 1, 2, 3):
                check(needles, hays, k, costs, anchored)
    want = X.join(needles, hays, 1, Y.RDAMERAU, False)
    recs = {(i, p): r for r in want[0] for i, p in [r[:2]]}
    assert recs[(0, 0)][4] == 0                                    # the run of one byte: found exactly
    assert recs[(1, 1)][4] == 1 and recs[(2, 2)][4] == 1           # each transposition costs 1
    assert recs[(3, 3)][4] == 1                                    # the first byte alone
    assert recs[(4, 4)][4] == 1                                    # the needle's last byte is missing
    lev = X.join(needles, hays, 1, Y.LEVENSHTEIN, False)
    assert (2, 2) not in {r[:2] for r in lev[0]}                   # (without the transposition term it costs 2; bytes 0 and 1: a free start makes it 1)


def test_short_haystacks_and_empty_sides():
    needles = [b"", b"A", b"ACGTACGT", b"ACGTACGTA" * 4, b"C" * 33, b"C" * 64]
    hays = [b"", b"A", b"ACG", b"ACGTACG", b"C" * 32, b"C" * 33, b"C" * 63, b"C" * 65]
    for costs in X.COSTS:
        for anchored in (False, True):
            for k in (0, 1, 8, 70):
                check(needles, hays, k, costs, anchored)
    for needles, hays in (([], [b"ACGT"]), ([b"ACGT" * 10], []), ([], [])):
        got = emu(needles, hays, 2, X.COSTS[0])
        assert got["count"] == 0 and got["nearest"] == [X.ALL_ONES] * len(hays) and got["per"] == [0] * len(hays)
        assert got["best"] == [(0, 0, X.NONE)] * len(hays)


def test_forced_sub_batches_of_64_on_257_haystacks():
    needles = Y.panel(900, 33)
    hays = X.reads(901, 257, needles)
    for anchored in (False, True):
        want, got = check(needles, hays, 3, X.COSTS[0], anchored, sub=64)
        assert got["subs"] == 5                                    # 64 + 64 + 64 + 64 + 1
        _, one = check(needles, hays, 3, X.COSTS[0], anchored)
        assert one["subs"] == 1 and one["records"] == got["records"]


def test_cap_cuts_the_records_not_the_count_and_optional_outputs():
    needles = Y.panel(1000, 16)
    hays = X.reads(1001, 65, needles)
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


def test_the_exact_pass_columns_stay_within_the_budget():
    """one column of 6 x 65 words per resident lane, whole workgroups, at most 256 MB of them whatever the sub-batch holds"""
    L = lib().emu_search_cross_w2_lanes
    assert L(0) == 256 and L(1) == 256 and L(256) == 256 and L(257) == 512
    top = L(1 << 40)
    assert top % 256 == 0 and top * 6 * 65 * 4 <= 256 << 20 < (top + 256) * 6 * 65 * 4
    assert L(top) == top and L(top + 1) == top


# ---------------------------------------------------------------- the C ABI: argument errors come first, no CPU fallback
def _abi():
    from triple_accel_amd import _native as N
    return N


def _call(needles, nn, haystacks, nh, k=1, costs=(1, 1, 0, None), anchored=0, flags=0, hits=None, count=None, cap=0, nearest=None, best=None,
          per=None):
    N = _abi()
    cc = None if costs is None else N.EditCostsC(costs[0], costs[1], costs[2], int(costs[3] is not None), costs[3] or 0)
    return N.lib().ta_levenshtein_search_cross_with_opts(needles, nn, haystacks, nh, k, None if cc is None else C.byref(cc), anchored, flags,
                                                         hits, count, cap, nearest, best, per, None)


def test_abi_symbol_is_declared_and_exported():
    N = _abi()
    assert "ta_levenshtein_search_cross_with_opts" in N.ABI_SYMBOLS and hasattr(N.lib(), "ta_levenshtein_search_cross_with_opts")
    header = open(os.path.join(os.path.dirname(HERE), "include", "triple_accel_amd.h")).read()
    at = header.index("int ta_levenshtein_search_cross_with_opts(")
    comment = header[header.rindex("/*", 0, at):at]
    assert "src/levenshtein.rs:1911-1966" in comment and ":1693-1706" in comment and ":1812-1835" in comment and "two calls" in comment


def test_abi_errors_in_their_order_before_the_device():
    N = _abi()
    blob = (C.c_uint8 * 128)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 8, 8, 0)
    S = C.byref(s)
    fake = C.c_void_p(0x1000)
    msg = lambda: N.lib().ta_last_error().decode()                 # noqa: E731
    # NULL costs / needles / haystacks / count_dev
    assert _call(S, 1, S, 1, costs=None, count=fake) == N.TA_ERR_ARG
    assert _call(None, 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, None, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=None) == N.TA_ERR_ARG
    assert _call(S, 0, S, 0, count=None) == N.TA_ERR_ARG
    # then the flags: every bit is reserved, whatever else is wrong behind it
    for bit in (1, 2, 1 << 31):
        assert _call(S, 1, S, 1, flags=bit, count=fake) == N.TA_ERR_ARG and "flag" in msg()
    assert _call(S, 1, S, 1, flags=1, costs=(0, 1, 0, None), count=fake) == N.TA_ERR_ARG and "flag" in msg()
    assert _call(S, 1, S, 1, flags=1, count=None) == N.TA_ERR_ARG and "null" in msg()          # (a NULL pointer comes before the flags)
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
    long_needle = N.StringsC(ptr, 0, 65, 65, 0)
    assert _call(C.byref(long_needle), 1, S, 1, count=fake, cap=4, hits=None) == N.TA_ERR_ARG
    # then the limits: 65 bytes, strided and CSR
    assert _call(C.byref(long_needle), 1, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED and "64 bytes" in msg()
    long_csr_needle = N.StringsC(ptr, 0x1000, 0, 0, 65)
    assert _call(C.byref(long_csr_needle), 1, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED and "64 bytes" in msg()
    # a 64-byte bound passes the needle limit: the NEXT limit answers (65,536 needles), where a 65-byte bound still names the needle
    top, top_csr = N.StringsC(ptr, 0, 64, 64, 0), N.StringsC(ptr, 0x1000, 0, 0, 64)
    for side in (top, top_csr):
        assert _call(C.byref(side), 65536, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED and "65,535" in msg()
    assert _call(C.byref(long_needle), 65536, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED and "64 bytes" in msg()
    assert _call(S, 65536, S, 1, count=fake) == N.TA_ERR_UNSUPPORTED
    huge = N.StringsC(ptr, 0, 1 << 32, 1 << 32, 0)
    assert _call(S, 1, C.byref(huge), 1, count=fake) == N.TA_ERR_UNSUPPORTED
    huge_csr = N.StringsC(ptr, 0x1000, 0, 0, 1 << 32)
    assert _call(S, 1, C.byref(huge_csr), 1, count=fake) == N.TA_ERR_UNSUPPORTED
    assert _call(S, 1, S, 1 << 32, count=fake) == N.TA_ERR_UNSUPPORTED


def test_the_32_byte_entry_keeps_its_limit_and_its_message():
    N = _abi()
    blob = (C.c_uint8 * 128)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 8, 8, 0)
    nd33 = N.StringsC(ptr, 0, 33, 33, 0)
    cc = N.EditCostsC(1, 1, 0, 0, 0)
    rc = N.lib().ta_levenshtein_search_cross(C.byref(nd33), 1, C.byref(s), 1, 1, C.byref(cc), 0, None, C.c_void_p(0x1000), 0, None, None, None, None)
    assert rc == N.TA_ERR_UNSUPPORTED and "32 bytes" in N.lib().ta_last_error().decode()


def test_no_cpu_fallback_without_a_device():
    """with every argument in order and no device the answer is TA_ERR_HIP, a 64-byte needle included (with a device the GPU tests run it)"""
    import torch
    N = _abi()
    if torch.cuda.is_available():
        return
    blob = (C.c_uint8 * 128)()
    ptr = C.cast(blob, C.c_void_p).value
    s, nd = N.StringsC(ptr, 0, 8, 8, 0), N.StringsC(ptr, 0, 64, 64, 0)
    count = (C.c_uint64 * 1)()
    cnt = C.cast(count, C.c_void_p)
    for anchored in (0, 1):
        for k in (0, 3, 0xFFFFFFFF):
            assert _call(C.byref(nd), 1, C.byref(s), 1, k=k, anchored=anchored, count=cnt) == N.TA_ERR_HIP
    assert _call(C.byref(nd), 0, C.byref(s), 4, count=cnt) == N.TA_ERR_HIP              # the outputs are initialised on the device
