"""gpu: hamming_search over batches of (needle, haystack) pairs (ta_hamming_search_batch) against the oracle hamming_search_simd_with_opts
on EVERY pair: CSR and strided haystacks, shared / strided / CSR needles, All and Best, the forced general route against the default one
bit for bit, batch sizes on both sides of the wavefront and of the ordering threshold, the NUL verdict among ordinary pairs, cap cutting,
caller-supplied outputs, graph capture, single calls, hamming_search_many, and one batch of a million reads."""
import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
SIZES = (1, 63, 64, 65, 4095, 4096, 20000)


def _mods():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    return torch, T, B


def _kernel():
    import triple_accel_amd as T
    return T._n.lib().ta_last_kernel_name().decode()


def _no_nul(*sides):
    for side in sides:
        assert all(0 not in s for s in side), "data meant to be NUL-free holds a zero byte"


def _subst(g, s, subs, alphabet):
    s = bytearray(s)
    for _ in range(subs):
        s[int(g.integers(len(s)))] = int(g.choice(alphabet))
    return bytes(s)


def _reads(seed, n, needle_of, lo=0, hi=120, alphabet=ACGT, fixed=None):
    """haystacks over `alphabet`; every other one holds a copy of its needle with 0-2 substitutions"""
    g = Dg.rng(seed)
    hays = []
    for i in range(n):
        h = bytearray(g.choice(alphabet, fixed if fixed is not None else int(g.integers(lo, hi + 1))))
        nd = needle_of(i)
        if i % 2 and len(h) >= len(nd) and nd:
            p = int(g.integers(0, len(h) - len(nd) + 1))
            h[p:p + len(nd)] = _subst(g, nd, int(g.integers(0, 3)), alphabet)
        hays.append(bytes(h))
    return hays


def _want(needles, hays, k, st):
    out = []
    for nd, h in zip(needles, hays):
        try:
            w = O.hamming_search_simd_with_opts(nd, h, k, st)
            out.append((len(w), w))
        except ValueError:
            out.append((-1, []))
    return out


def _got(m, c, cut=False):
    m, c = m.cpu().numpy(), c.cpu().numpy()
    cap = m.shape[1]
    if not cut:
        assert int(c.max(initial=0)) <= cap, "the test's cap cuts a result"
    return [(int(c[i]), [tuple(int(x) for x in r) for r in m[i, :max(0, min(int(c[i]), cap))]]) for i in range(len(c))]


def _hay_side(B, hays, strided):
    if strided:
        return B.Strings.from_fixed(np.frombuffer(b"".join(hays), np.uint8).reshape(len(hays), -1))
    return B.Strings.from_list(hays)


def _run(B, torch, needle_side, hs, k, st, cap):
    m, c = B.hamming_search_batch(needle_side, hs, k, st, cap=cap)
    torch.cuda.synchronize()
    return m, c


def _same(torch, a, b):
    """two device results bit for bit: the counts, and every row a count makes meaningful"""
    (m1, c1), (m2, c2) = a, b
    if not torch.equal(c1, c2):
        return False
    cap = m1.shape[1]
    live = torch.arange(cap, device=c1.device)[None, :] < c1.clamp(0, cap)[:, None].to(torch.int64)
    return torch.equal(m1[live], m2[live])


@pytest.mark.parametrize("n", SIZES)
def test_shared_needle_csr_both_routes_every_pair(n, monkeypatch):
    torch, T, B = _mods()
    needle = b"ACGTTGCAAGGCTTACGGATCCAT"                        # 24 bytes
    hays = _reads(100 + n, n, lambda i: needle, 0, 120)
    _no_nul([needle], hays)
    hs = B.Strings.from_list(hays)
    side = B.Strings.shared(needle, n)
    for st in (O.ALL, O.BEST):
        for k in (2, 6):
            cap = 16 if k == 2 else 100
            r1 = _run(B, torch, side, hs, k, st, cap)
            k1 = _kernel()
            monkeypatch.setenv("TA_HSEARCH_BATCH_GENERAL", "1")
            r2 = _run(B, torch, side, hs, k, st, cap)
            k2 = _kernel()
            monkeypatch.delenv("TA_HSEARCH_BATCH_GENERAL")
            assert "bits" in k1 and k2 == "ham_search_batch_kernel<8>", (k1, k2)
            assert _same(torch, r1, r2)
            assert _got(*r1) == _want([needle] * n, hays, k, st), (n, st, k)


@pytest.mark.parametrize("n", (64, 4096))
def test_shared_needle_strided_haystacks(n, monkeypatch):
    torch, T, B = _mods()
    for needle, k in ((b"GATTACAG", 1), (b"ACGTTGCAAGGCTTACGGATCCATACGTACGTAAGGCCTTAGCATCGATCGGATTACAGGCATGCA", 8), (b"TTGACCAGTAGC" * 6, 20)):
        hays = _reads(200 + n + len(needle), n, lambda i: needle, fixed=151)
        _no_nul([needle], hays)
        hs = _hay_side(B, hays, True)
        side = B.Strings.shared(needle, n)
        for st in (O.ALL, O.BEST):
            r1 = _run(B, torch, side, hs, k, st, 32)
            k1 = _kernel()
            monkeypatch.setenv("TA_HSEARCH_BATCH_GENERAL", "1")
            r2 = _run(B, torch, side, hs, k, st, 32)
            monkeypatch.delenv("TA_HSEARCH_BATCH_GENERAL")
            assert ("bits" in k1) == (len(needle) <= 32), k1
            assert _same(torch, r1, r2)
            assert _got(*r1) == _want([needle] * n, hays, k, st), (n, len(needle), st)


@pytest.mark.parametrize("n", (65, 4096, 20000))
def test_per_pair_needles_csr_and_strided(n):
    torch, T, B = _mods()
    g = Dg.rng(300 + n)
    needles = [bytes(g.choice(ACGT, int(g.integers(1, 33)))) for _ in range(n)]
    hays = _reads(301 + n, n, lambda i: needles[i], 0, 100)
    _no_nul(needles, hays)
    for st in (O.ALL, O.BEST):
        r = _run(B, torch, B.Strings.from_list(needles), B.Strings.from_list(hays), 2, st, 100)
        assert _kernel() == "ham_search_batch_kernel<8>"
        assert _got(*r) == _want(needles, hays, 2, st), (n, st)
    # strided needles (12 bytes each) over strided haystacks
    fixed_n = [bytes(g.choice(ACGT, 12)) for _ in range(n)]
    fixed_h = _reads(302 + n, n, lambda i: fixed_n[i], fixed=64)
    _no_nul(fixed_n, fixed_h)
    nd_side = B.Strings.from_fixed(np.frombuffer(b"".join(fixed_n), np.uint8).reshape(n, 12))
    for st in (O.ALL, O.BEST):
        r = _run(B, torch, nd_side, _hay_side(B, fixed_h, True), 3, st, 64)
        assert _kernel() == "ham_search_batch_kernel<4>"
        assert _got(*r) == _want(fixed_n, fixed_h, 3, st), (n, st)


def test_mixed_batch_nul_empty_short_and_long_needles():
    """NUL pairs, empty needles, empty haystacks, h < n (with and without a NUL), needles over 32 and over 64 bytes, all in one call"""
    torch, T, B = _mods()
    g = Dg.rng(400)
    needles, hays = [], []
    for i in range(5000):
        kind = i % 10
        n = int(g.integers(1, 30)) if kind < 6 else int(g.integers(33, 65)) if kind < 8 else int(g.integers(65, 140))
        nd = bytes(g.integers(1, 256, size=n, dtype=np.uint8)) if i % 3 else bytes(g.choice(ACGT, n))
        h = bytearray(g.choice(ACGT, int(g.integers(n, 200))))
        p = int(g.integers(0, len(h) - n + 1))
        h[p:p + n] = _subst(g, nd, int(g.integers(0, 4)), ACGT)
        what = int(g.integers(12))
        if what == 0:
            nd = b""
        elif what == 1:
            h = bytearray()
        elif what == 2:
            h = h[:max(0, n - 1 - int(g.integers(3)))]
        elif what == 3 and len(h):
            h[int(g.integers(len(h)))] = 0                     # the NUL verdict
        elif what == 4 and n > 1:
            h = h[:n - 1]
            h[int(g.integers(len(h)))] = 0                     # a NUL in a haystack shorter than its needle: no verdict
        elif what == 5:
            nd = bytes([0]) + nd[1:]                           # a NUL in the needle: no verdict
        needles.append(nd)
        hays.append(bytes(h))
    assert max(len(x) for x in needles) > 64
    for st in (O.ALL, O.BEST):
        for k in (0, 3, 40):
            want = _want(needles, hays, k, st)
            r = _run(B, torch, B.Strings.from_list(needles), B.Strings.from_list(hays), k, st, 200)
            assert _kernel() == "ham_search_batch_mem_kernel"
            assert _got(*r) == want, (st, k)
    kinds = {c for c, _ in want}
    assert -1 in kinds and 0 in kinds and max(kinds) > 1
    # the same pairs with the needles capped at 64 bytes: the widest register form
    needles64 = [nd[:64] for nd in needles]
    r = _run(B, torch, B.Strings.from_list(needles64), B.Strings.from_list(hays), 3, O.BEST, 200)
    assert _kernel() == "ham_search_batch_kernel<16>"
    assert _got(*r) == _want(needles64, hays, 3, O.BEST)


def test_shared_needle_with_nul_pairs_and_k_at_least_n(monkeypatch):
    torch, T, B = _mods()
    g = Dg.rng(500)
    needle = b"ACGTTGCAAG"
    hays = [bytearray(h) for h in _reads(501, 3000, lambda i: needle, 0, 90)]
    for i in range(0, 3000, 7):
        if len(hays[i]):
            hays[i][int(g.integers(len(hays[i])))] = 0
    hays = [bytes(h) for h in hays]
    hs, side = B.Strings.from_list(hays), B.Strings.shared(needle, len(hays))
    for st in (O.ALL, O.BEST):
        for k in (0, 1, 2, 3, 9, 10, 15):                      # 4 k > n: the general route; k >= n: every offset is a match (All)
            want = _want([needle] * len(hays), hays, k, st)
            r1 = _run(B, torch, side, hs, k, st, 100)
            assert ("bits" in _kernel()) == (4 * k <= len(needle))
            monkeypatch.setenv("TA_HSEARCH_BATCH_GENERAL", "1")
            r2 = _run(B, torch, side, hs, k, st, 100)
            monkeypatch.delenv("TA_HSEARCH_BATCH_GENERAL")
            assert _same(torch, r1, r2)
            assert _got(*r1) == want, (st, k)
            assert any(c == -1 for c, _ in want) and any(c > 0 for c, _ in want)
    all10 = _want([needle] * len(hays), hays, 10, O.ALL)
    assert all(c == len(h) - len(needle) + 1 for (c, _), h in zip(all10, hays) if c > 0)


def test_cap_cut_counts_only_and_caller_outputs():
    torch, T, B = _mods()
    g = Dg.rng(600)
    bits = np.frombuffer(b"ab", np.uint8)
    needle = b"abbab"
    hays = [bytes(g.choice(bits, int(g.integers(0, 80)))) for _ in range(500)]
    _no_nul([needle], hays)
    hs, side = B.Strings.from_list(hays), B.Strings.shared(needle, len(hays))
    for st in (O.ALL, O.BEST):
        want = _want([needle] * len(hays), hays, 2, st)
        cap = 4
        assert any(c > cap for c, _ in want) and any(0 < c <= cap for c, _ in want)
        full = _got(*_run(B, torch, side, hs, 2, st, 100))
        assert full == want
        cut = _got(*_run(B, torch, side, hs, 2, st, cap), cut=True)
        assert cut == [(c, rows[:cap]) for c, rows in want]
        m0, c0 = _run(B, torch, side, hs, 2, st, 0)
        assert m0.shape == (len(hays), 0, 3) and c0.cpu().tolist() == [c for c, _ in want]
        # caller-supplied tensors are the ones written and returned
        m = torch.full((len(hays), cap, 3), -7, dtype=torch.int64, device="cuda")
        c = torch.full((len(hays),), -7, dtype=torch.int32, device="cuda")
        m2, c2 = B.hamming_search_batch(side, hs, 2, st, cap=cap, matches=m, counts=c)
        torch.cuda.synchronize()
        assert m2 is m and c2 is c and _got(m, c, cut=True) == cut
        with pytest.raises(ValueError):
            B.matches_to_lists(m, c)
        assert [[tuple(x) for x in r] for r in B.matches_to_lists(m, c, allow_cut=True)] == [rows for _, rows in cut]


def test_single_calls_search_many_and_the_nul_error():
    torch, T, B = _mods()
    g = Dg.rng(700)
    needle = b"ACCGTTAGCA"
    hays = _reads(701, 300, lambda i: needle, 0, 150)
    _no_nul([needle], hays)
    for st in (T.SearchType.Best, T.SearchType.All):
        got = T.hamming_search_many(needle, hays, 3, st)
        assert got == [list(T.hamming_search_simd_with_opts(needle, h, 3, st)) for h in hays]
    assert T.hamming_search_many(needle, hays) == [list(T.hamming_search(needle, h)) for h in hays]
    needles = [bytes(g.choice(ACGT, int(g.integers(1, 20)))) for _ in hays]
    got = T.hamming_search_many(needles, hays, 2, T.SearchType.All)
    assert got == [list(T.hamming_search_simd_with_opts(nd, h, 2, T.SearchType.All)) for nd, h in zip(needles, hays)]
    assert any(got)
    with pytest.raises(ValueError):
        T.hamming_search_many(needles[:-1], hays, 2)
    with pytest.raises(ValueError):
        T.hamming_search_many(needles, hays)
    # the NUL verdict: -1 in counts, PanicError from matches_to_lists and from hamming_search_many, as from the single call
    bad = list(hays)
    bad[17] = b"ACGT\x00" + b"ACGTACGTAC"
    bad[40] = b"\x00"                                         # shorter than the needle: not an error
    m, c = B.hamming_search_batch(B.Strings.shared(needle, len(bad)), B.Strings.from_list(bad), 3)
    torch.cuda.synchronize()
    assert int(c[17]) == -1 and int(c[40]) == 0 and int((c < 0).sum()) == 1
    with pytest.raises(T.PanicError, match="No zero/null bytes allowed in the string!.*17"):
        B.matches_to_lists(m, c)
    with pytest.raises(T.PanicError):
        T.hamming_search_many(needle, bad, 3)
    with pytest.raises(T.PanicError):
        T.hamming_search_simd_with_opts(needle, bad[17], 3, T.SearchType.Best)
    assert list(T.hamming_search_simd_with_opts(needle, bad[40], 3, T.SearchType.Best)) == []


def test_graph_capture_follows_changed_haystacks(monkeypatch):
    torch, T, B = _mods()
    needle = b"TTGACCAGTAGG"
    n = 5000
    variants = [_reads(800 + v, n, lambda i: needle, fixed=96) for v in range(3)]
    for v in variants:
        _no_nul(v)
    off = np.arange(n + 1, dtype=np.int64) * 96
    blob = torch.zeros(n * 96 + 16, dtype=torch.uint8, device="cuda")

    def put(v):
        blob[: n * 96] = torch.frombuffer(bytearray(b"".join(variants[v])), dtype=torch.uint8).cuda()

    hs = B.Strings(blob, torch.from_numpy(off).cuda(), max_len=96)       # CSR with its bound given: ordered, no synchronisation
    side = B.Strings.shared(needle, n)
    for general in (False, True):
        if general:
            monkeypatch.setenv("TA_HSEARCH_BATCH_GENERAL", "1")
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            put(0)
            m0, c0 = B.hamming_search_batch(side, hs, 2, O.BEST, cap=8)          # eager: sizes the scratch
            s.synchronize()
            assert _got(m0, c0) == _want([needle] * n, variants[0], 2, O.BEST)
            m, c = torch.full_like(m0, -7), torch.full_like(c0, -7)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                B.hamming_search_batch(side, hs, 2, O.BEST, cap=8, matches=m, counts=c)
            for v in (1, 2):
                put(v)
                graph.replay()
                s.synchronize()
                assert _got(m, c) == _want([needle] * n, variants[v], 2, O.BEST), (general, v)
        if general:
            monkeypatch.delenv("TA_HSEARCH_BATCH_GENERAL")


def test_a_million_reads():
    """1,048,576 ACGT haystacks of 100-250 bytes, a shared 24-byte needle planted with 0-2 substitutions in every other one, Best k = 2:
    count properties on every pair, the oracle on a fixed sample of 2,000"""
    torch, T, B = _mods()
    n, nl = 1 << 20, 24
    g = Dg.rng(900)
    needle = bytes(g.choice(ACGT, nl))
    lens = g.integers(100, 251, size=n).astype(np.int64)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    blob = g.choice(ACGT, int(off[-1]) + 16).astype(np.uint8)
    planted = np.arange(n) % 2 == 1
    pos = (g.random(n) * (lens - nl + 1)).astype(np.int64)
    subs = g.integers(0, 3, size=n)
    copies = np.tile(np.frombuffer(needle, np.uint8), (n, 1))
    for s in range(2):
        rows = np.nonzero(subs > s)[0]
        copies[rows, g.integers(0, nl, size=rows.size)] = g.choice(ACGT, rows.size)
    idx = (off[:-1] + pos)[planted, None] + np.arange(nl)[None, :]
    blob[idx] = copies[planted]
    assert not (blob[: int(off[-1])] == 0).any()
    hs = B.Strings(torch.from_numpy(blob).cuda(), torch.from_numpy(off).cuda(), max_len=250)
    m, c = B.hamming_search_batch(B.Strings.shared(needle, n), hs, 2, O.BEST, cap=8)
    torch.cuda.synchronize()
    assert "bits" in _kernel()
    m, c = m.cpu().numpy(), c.cpu().numpy().astype(np.int64)
    assert (c >= 0).all() and (c <= lens - nl + 1).all()
    assert (c[planted] >= 1).all()                            # a copy with <= 2 substitutions is a window of <= 2 mismatches
    live = np.arange(8)[None, :] < np.minimum(c, 8)[:, None]
    ks = np.where(live, m[:, :, 2], -1)
    first_k = m[:, 0, 2]
    assert ((ks == -1) | (ks == first_k[:, None])).all()      # Best: every kept window at one count ...
    assert (first_k[c > 0] <= 2).all() and (first_k[planted] <= subs[planted]).all()
    assert (np.where(live, m[:, :, 1] - m[:, :, 0], nl) == nl).all()
    starts = np.where(live, m[:, :, 0], np.iinfo(np.int64).max)
    assert (np.diff(starts, axis=1)[live[:, 1:]] > 0).all()   # ... in increasing start
    assert (np.where(live, m[:, :, 1], 0) <= lens[:, None]).all()
    sample = Dg.rng(901).choice(n, 2000, replace=False)
    for i in sample:
        hay = blob[off[i]:off[i + 1]].tobytes()
        want = O.hamming_search_simd_with_opts(needle, hay, 2, O.BEST)
        assert int(c[i]) == len(want) and [tuple(int(x) for x in r) for r in m[i, :min(int(c[i]), 8)]] == want[:8], int(i)
