"""gpu: levenshtein_search over batches of (needle, haystack) pairs (ta_levenshtein_search_batch) against the scalar oracle per pair:
CSR and strided haystacks, shared and per-pair needles, All and Best, anchored, every cost family, the scan route against the exact
route bit for bit, the packed form against the unpacked one, cap cutting, graph capture, and levenshtein_search_many against a loop of
single calls."""
import os

import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

pytestmark = pytest.mark.gpu

COSTS = [(1, 1, 0, None), (1, 1, 0, 1), (3, 1, 0, None), (1, 1, 2, None), (2, 1, 2, None), (2, 2, 1, 3), (1, 2, 0, 1), (2, 3, 1, None)]
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _mods():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    return torch, T, B


def _mutate(g, s, edits):
    s = bytearray(s)
    for _ in range(edits):
        op, p = int(g.integers(3)), int(g.integers(len(s) + 1))
        if op == 0 or not s:
            s.insert(p, int(g.choice(ACGT)))
        elif op == 1:
            del s[min(p, len(s) - 1)]
        else:
            s[min(p, len(s) - 1)] = int(g.choice(ACGT))
    return bytes(s)


def _reads(seed, n, needle, lo=0, hi=120, alphabet=ACGT):
    """haystacks over a small alphabet, a mutated copy of `needle` planted in every other one, empty ones mixed in"""
    g = Dg.rng(seed)
    hays = []
    for i in range(n):
        h = bytearray(g.choice(alphabet, int(g.integers(lo, hi + 1))))
        if i % 2 and len(h) > len(needle) and needle:
            m = _mutate(g, needle, int(g.integers(0, 3)))
            p = int(g.integers(0, len(h) - len(m) + 1))
            h[p:p + len(m)] = m
        hays.append(bytes(h))
    return hays


def _want(needles, hays, k, st, costs, anchored):
    return [O.levenshtein_search_naive_with_opts(nd, h, k, st, costs, anchored) for nd, h in zip(needles, hays)]


def _got(m, c, B):
    return [[tuple(x) for x in r] for r in B.matches_to_lists(m, c)]


def _run(needle_side, hays, k, st, costs, anchored, strided=False, cap=None):
    torch, T, B = _mods()
    if strided:
        hs = B.Strings.from_fixed(np.frombuffer(b"".join(hays), np.uint8).reshape(len(hays), -1) if hays else np.zeros((0, 0), np.uint8))
    else:
        hs = B.Strings.from_list(hays)
    cap = max([len(h) + 2 for h in hays] + [1]) if cap is None else cap
    m, c = B.levenshtein_search_batch(needle_side, hs, k, st, costs, anchored, cap=cap)
    torch.cuda.synchronize()
    return m, c


@pytest.mark.parametrize("costs", COSTS)
def test_shared_needle_csr_all_best_anchored(costs):
    torch, T, B = _mods()
    needle = b"ACGTTGCAAGGCTTAC"
    hays = _reads(1, 300, needle)
    for st in (O.ALL, O.BEST):
        for anchored in (False, True):
            for k in (0, 3, 9):
                m, c = _run(B.Strings.shared(needle, len(hays)), hays, k, st, costs, anchored)
                assert _got(m, c, B) == _want([needle] * len(hays), hays, k, st, costs, anchored), (st, anchored, k)


@pytest.mark.parametrize("costs", COSTS)
def test_per_pair_needles_csr_and_strided(costs):
    torch, T, B = _mods()
    g = Dg.rng(2)
    needles = [bytes(g.choice(ACGT, int(g.integers(0, 45)))) for _ in range(200)]
    hays = [_reads(10 + i, 1, nd, 0, 90)[0] if i % 2 == 0 else _mutate(g, bytes(g.choice(ACGT, 30)) + nd + bytes(g.choice(ACGT, 20)), 2)
            for i, nd in enumerate(needles)]
    for st in (O.ALL, O.BEST):
        for anchored in (False, True):
            m, c = _run(B.Strings.from_list(needles), hays, 4, st, costs, anchored)
            assert _got(m, c, B) == _want(needles, hays, 4, st, costs, anchored), (st, anchored)
    # strided haystacks and strided (fixed-length) needles: the packed form applies
    fixed_n = [bytes(g.choice(ACGT, 12)) for _ in range(100)]
    fixed_h = [bytes(g.choice(ACGT, 64)) for _ in range(100)]
    fixed_h = [h[:20] + _mutate(g, nd, 1)[:12].ljust(12, b"A") + h[32:] for h, nd in zip(fixed_h, fixed_n)]
    nd_side = B.Strings.from_fixed(np.frombuffer(b"".join(fixed_n), np.uint8).reshape(100, 12))
    for st in (O.ALL, O.BEST):
        m, c = _run(nd_side, fixed_h, 3, st, costs, False, strided=True)
        assert _got(m, c, B) == _want(fixed_n, fixed_h, 3, st, costs, False)


def test_edges_empty_pairs_n0_n1_and_binary_ties():
    torch, T, B = _mods()
    for costs in COSTS:
        needles = [b"", b"ab", b"", b"abc" * 5, b"a"]
        hays = [b"", b"", b"abab", b"ab", b"\x00a\x00"]
        for st in (O.ALL, O.BEST):
            for anchored in (False, True):
                m, c = _run(B.Strings.from_list(needles), hays, 3, st, costs, anchored, cap=8)
                assert _got(m, c, B) == _want(needles, hays, 3, st, costs, anchored)
    # n = 0 and n = 1
    m, c = _run(B.Strings.shared(b"ACG", 0), [], 1, O.BEST, COSTS[0], False, cap=4)
    assert m.shape[0] == 0 and c.numel() == 0
    m, c = _run(B.Strings.shared(b"ACG", 1), [b"TTACGTT"], 1, O.ALL, COSTS[0], False, cap=16)
    assert _got(m, c, B) == _want([b"ACG"], [b"TTACGTT"], 1, O.ALL, COSTS[0], False)
    # binary alphabets: ties, Q2
    g = Dg.rng(3)
    bits = np.frombuffer(b"ab", np.uint8)
    needle = b"abbab"
    hays = [bytes(g.choice(bits, int(g.integers(0, 60)))) for _ in range(200)]
    for costs in COSTS:
        for st in (O.ALL, O.BEST):
            m, c = _run(B.Strings.shared(needle, len(hays)), hays, 2, st, costs, False)
            assert _got(m, c, B) == _want([needle] * len(hays), hays, 2, st, costs, False)


def test_long_haystack_among_short_ones_and_long_needles():
    torch, T, B = _mods()
    needle = b"GATTACAGATTACAGATTACA"
    hays = _reads(4, 400, needle, 0, 200)
    g = Dg.rng(4)
    big = bytearray(g.choice(ACGT, 200 * 1024))
    for p in range(1000, len(big) - 100, 20000):
        big[p:p + len(needle)] = _mutate(g, needle, 1)
    hays.insert(123, bytes(big))
    for costs in (COSTS[0], COSTS[5]):
        for st in (O.ALL, O.BEST):
            m, c = _run(B.Strings.shared(needle, len(hays)), hays, 3, st, costs, False, cap=64)
            assert _got(m, c, B) == _want([needle] * len(hays), hays, 3, st, costs, False)
    long_needle = bytes(g.choice(ACGT, 50))                    # 33..64 bytes: two-word scan + memory-backed column
    hays = _reads(5, 300, long_needle, 0, 200)
    for costs in COSTS:
        m, c = _run(B.Strings.shared(long_needle, len(hays)), hays, 6, O.BEST, costs, False, cap=8)
        assert _got(m, c, B) == _want([long_needle] * len(hays), hays, 6, O.BEST, costs, False)
    longer = bytes(g.choice(ACGT, 90))
    hays = _reads(6, 64, longer, 0, 160)
    m, c = _run(B.Strings.shared(longer, len(hays)), hays, 10, O.ALL, COSTS[3], True, cap=200)
    assert _got(m, c, B) == _want([longer] * len(hays), hays, 10, O.ALL, COSTS[3], True)


def test_cap_cut_prefix_and_counts_only():
    torch, T, B = _mods()
    needle = b"ACGT"
    hays = [b"ACGT" * 20, b"TTTT", b"ACG", b""]
    full_m, full_c = _run(B.Strings.shared(needle, 4), hays, 2, O.ALL, COSTS[0], False, cap=200)
    full = _got(full_m, full_c, B)
    assert full == _want([needle] * 4, hays, 2, O.ALL, COSTS[0], False)
    for cap in (0, 1, 5):
        m, c = _run(B.Strings.shared(needle, 4), hays, 2, O.ALL, COSTS[0], False, cap=cap)
        assert c.cpu().tolist() == full_c.cpu().tolist()
        assert [[tuple(x) for x in r] for r in B.matches_to_lists(m, c, allow_cut=True)] == [r[:cap] for r in full]
        if cap < max(len(r) for r in full):
            with pytest.raises(ValueError):
                B.matches_to_lists(m, c)


def _kernel():
    import triple_accel_amd as T
    return T._n.lib().ta_last_kernel_name().decode()


def test_scan_route_equals_exact_route_and_packed_equals_unpacked(monkeypatch):
    torch, T, B = _mods()
    needle = b"ACGTACGTTGCAGGCATTCA"
    hays = _reads(7, 5000, needle, 60, 200)
    hs = B.Strings.from_list(hays)
    for costs in (COSTS[0], COSTS[1], COSTS[5], COSTS[7]):
        for st in (O.ALL, O.BEST):
            side = B.Strings.shared(needle, len(hays))
            m1, c1 = B.levenshtein_search_batch(side, hs, 4, st, costs, cap=16)
            torch.cuda.synchronize()
            k1 = _kernel()
            monkeypatch.setenv("TA_SEARCH_BATCH_NO_SCAN", "1")
            m2, c2 = B.levenshtein_search_batch(side, hs, 4, st, costs, cap=16)
            torch.cuda.synchronize()
            k2 = _kernel()
            monkeypatch.setenv("TA_SEARCH_BATCH_UNPACKED", "1")
            m3, c3 = B.levenshtein_search_batch(side, hs, 4, st, costs, cap=16)
            torch.cuda.synchronize()
            k3 = _kernel()
            monkeypatch.delenv("TA_SEARCH_BATCH_NO_SCAN")
            monkeypatch.delenv("TA_SEARCH_BATCH_UNPACKED")
            assert "scan" in k1 and "scan" not in k2 and "true>" in k2 and "false>" in k3, (k1, k2, k3)
            assert torch.equal(c1, c2) and torch.equal(c1, c3)
            l1, l2, l3 = (B.matches_to_lists(m, c) for m, c in ((m1, c1), (m2, c2), (m3, c3)))
            assert l1 == l2 == l3
            idx = list(range(0, len(hays), 97))
            assert [[tuple(x) for x in l1[i]] for i in idx] == _want([needle] * len(idx), [hays[i] for i in idx], 4, st, costs, False)


def test_graph_capture_replays_the_eager_result():
    torch, T, B = _mods()
    needle = b"TTGACCAGTA"
    hays = _reads(8, 3000, needle, 40, 160)
    n = len(hays)
    import numpy as np_
    off = np_.zeros(n + 1, np_.int64)
    off[1:] = np_.cumsum([len(h) for h in hays])
    blob = torch.zeros(int(off[-1]) + 16, dtype=torch.uint8)
    blob[: int(off[-1])] = torch.frombuffer(bytearray(b"".join(hays)), dtype=torch.uint8)
    hs = B.Strings(blob.cuda(), torch.from_numpy(off).cuda(), max_len=max(len(h) for h in hays))
    side = B.Strings.shared(needle, n)
    for costs, anchored in ((COSTS[0], False), (COSTS[5], False), (COSTS[3], True)):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            m0, c0 = B.levenshtein_search_batch(side, hs, 3, O.BEST, costs, anchored, cap=8)     # eager: sizes the scratch
            s.synchronize()
            want_m, want_c = m0.clone(), c0.clone()
            m, c = torch.full_like(m0, -7), torch.full_like(c0, -7)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                B.levenshtein_search_batch(side, hs, 3, O.BEST, costs, anchored, cap=8, matches=m, counts=c)
            g.replay()
            s.synchronize()
        assert torch.equal(c, want_c)
        assert B.matches_to_lists(m, c) == B.matches_to_lists(want_m, want_c)


def test_search_many_equals_a_loop_of_single_calls():
    torch, T, B = _mods()
    g = Dg.rng(9)
    needle = b"ACCGTTAGCA"
    hays = _reads(9, 200, needle, 0, 150)
    for st, costs, anchored in ((T.SearchType.Best, T.LEVENSHTEIN_COSTS, False), (T.SearchType.All, T.EditCosts(2, 2, 1, 3), False),
                                (T.SearchType.All, T.RDAMERAU_COSTS, True)):
        got = T.levenshtein_search_many(needle, hays, 3, st, costs, anchored)
        want = [list(T.levenshtein_search_simd_with_opts(needle, h, 3, st, costs, anchored)) for h in hays]
        assert got == want
    assert T.levenshtein_search_many(needle, hays) == [list(T.levenshtein_search(needle, h)) for h in hays]
    needles = [bytes(g.choice(ACGT, int(g.integers(1, 20)))) for _ in hays]
    got = T.levenshtein_search_many(needles, hays, 2, T.SearchType.All)
    assert got == [list(T.levenshtein_search_simd_with_opts(nd, h, 2, T.SearchType.All, T.LEVENSHTEIN_COSTS, False)) for nd, h in zip(needles, hays)]
