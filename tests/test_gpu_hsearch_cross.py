"""gpu: every needle of a panel in every haystack within k mismatches (ta_hamming_search_cross) against the oracle
hamming_search_simd_with_opts(.., Best) over EVERY (needle, haystack) pair of every batch -- sorted records, count, nearest, best and
per-haystack with its NUL mark -- with the joins memoised per batch (tests/hsearch_cross_cases.py; the conditions these comparisons rely
on are asserted on the join alone in tests/test_hsearch_cross_cpu.py): batch sizes on both sides of the lane, wavefront and workgroup
edges times every panel size (every G, a last group with its own G) with k rotating through every plane count, strided and CSR sides,
cap cutting, counting only, every optional output left out in turn, empty sides, the limits, the error order, forced haystacks per
workgroup, streams, repeated calls, graph capture, the Python helpers, and the loop of shared-needle hamming_search_batch calls it
replaces."""
import numpy as np
import pytest

import datagen as Dg
import hsearch_cross_cases as X

pytestmark = pytest.mark.gpu

NHS = (1, 63, 64, 65, 257, 513)


def _mods():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    return torch, T, B


def _got(B, torch, out, cut=False):
    """(hits, count, nearest, best, per_haystack) of a call -> (sorted records, count, nearest words, best rows, per-haystack counts)"""
    hits, count, nearest, best, per = out
    torch.cuda.synchronize()
    cols = B.search_cross_to_arrays(hits, count, allow_cut=cut)
    recs = [tuple(int(x) for x in r) for r in zip(*cols)]
    words = None if nearest is None else [int(w) for w in nearest.cpu().numpy().view(np.uint64)]
    rows = None
    if best is not None:
        b = best.cpu().numpy().view(np.uint64).reshape(-1, 3)
        assert all(int(r[2]) >> 32 == 0 for r in b)                # pad_ = 0
        rows = [(int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF) for r in b]
    counts = None if per is None else [int(c) for c in per.cpu().numpy().view(np.uint32)]
    return recs, int(count.item()), words, rows, counts


def _check(B, torch, T, nd, hs, needles, hays, k):
    want = X.join(needles, hays, k)
    out = B.hamming_search_cross(nd, hs, k, cap=max(len(needles) * len(hays), 1), nearest=True, best=True, per_haystack=True)
    got = _got(B, torch, out)
    where = (len(needles), len(hays), k)
    assert got[1] == len(want[0]) and got[0] == want[0], where
    assert got[2] == want[1], where
    assert got[3] == want[2], where
    assert got[4] == want[3], where
    assert T.last_kernel_name() == "ham_search_cross_kernel<%d>" % X.planes(k, needles), (T.last_kernel_name(), where)
    return want


def _std():
    """the batch most tests share: 33 needles of every length but one byte (one group, G = 64, 31 idle columns), 257 reads -- what it
    holds is asserted in tests/test_hsearch_cross_cpu.py"""
    needles = X.panel(900, 33, lens=X.STD_LENS)
    return needles, X.reads(901, 257, needles)


@pytest.mark.parametrize("nn", X.PANELS)
@pytest.mark.parametrize("nh", NHS)
def test_every_pair_equals_the_oracle(nh, nn):
    """mixed needle lengths (k >= n and k < n in one group), every haystack length class, NUL reads; k rotates with the case, so that
    every plane count meets several shapes"""
    torch, T, B = _mods()
    case = NHS.index(nh) * len(X.PANELS) + X.PANELS.index(nn)
    k = X.KS[case % len(X.KS)]
    needles = X.panel(300 + nn, nn)
    hays = X.reads(400 + nn, nh, needles)
    want = _check(B, torch, T, B.Strings.from_list(needles), B.Strings.from_list(hays), needles, hays, k)
    assert len(want[0]) > 0 or nh == 1


@pytest.mark.parametrize("k", X.KS)
def test_every_plane_count_and_alphabet(k):
    torch, T, B = _mods()
    needles, hays = _std()
    _check(B, torch, T, B.Strings.from_list(needles), B.Strings.from_list(hays), needles, hays, k)
    assert T.last_kernel_name() == "ham_search_cross_kernel<%d>" % {0: 1, 1: 1, 2: 2, 3: 2, 4: 3, 8: 4, 16: 5, 31: 5, 32: 6, 40: 6}[k]
    al = X.BYTES                                                   # bytes 1..255
    needles = X.panel(134, 16, al)
    hays = X.reads(234, 64, needles, al)
    _check(B, torch, T, B.Strings.from_list(needles), B.Strings.from_list(hays), needles, hays, k)


@pytest.mark.parametrize("nform", ["strided", "csr", "csr_unmeasured"])
@pytest.mark.parametrize("hform", ["strided", "csr", "csr_unmeasured"])
def test_strided_and_csr_sides(nform, hform):
    torch, T, B = _mods()
    g = Dg.rng(1100)
    needles = [bytes(g.choice(X.ACGT, 21)) for _ in range(20)]     # 21 bytes: every string starts at another alignment
    hays = [h[:121] for h in X.reads(1101, 65, needles, lo=121, hi=250) if len(h) >= 121]
    assert len(hays) > 50

    def side(strings, form):
        if form == "strided":
            return B.Strings.from_fixed(np.frombuffer(b"".join(strings), np.uint8).reshape(len(strings), -1))
        s = B.Strings.from_list(strings)
        if form == "csr_unmeasured":
            s.max_len = 0                                          # "let the library measure it": one synchronisation
        return s

    nd, hs = side(needles, nform), side(hays, hform)
    for k in (2, 6):
        want = _check(B, torch, T, nd, hs, needles, hays, k)
        assert len(want[0]) >= 30


def test_cap_cuts_the_records_not_the_count_and_every_optional_output():
    torch, T, B = _mods()
    needles, hays = _std()
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    k = 2
    want = X.join(needles, hays, k)
    assert len(want[0]) >= 64
    cap = len(want[0]) // 2
    out = B.hamming_search_cross(nd, hs, k, cap=cap, nearest=True, best=True, per_haystack=True)
    recs, n, near, best, per = _got(B, torch, out, cut=True)
    assert n == len(want[0])                                       # the count is unchanged
    assert len(recs) == cap and len(set(r[:2] for r in recs)) == cap   # no record twice
    assert set(recs) <= set(want[0])                               # every record is a true hit
    assert near == want[1] and best == want[2] and per == want[3]  # none depends on cap
    with pytest.raises(ValueError, match="larger cap"):
        B.search_cross_to_arrays(out[0], out[1])
    # cap = 0 with a NULL hits buffer, then each optional output NULL in turn (best without nearest included)
    nh = len(hays)
    for use in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 1, 0), (0, 0, 0)):
        count0 = torch.full((1,), 5, dtype=torch.int64, device="cuda")
        near0 = torch.full((nh,), 5, dtype=torch.int64, device="cuda")
        best0 = torch.full((nh, 3), 5, dtype=torch.int64, device="cuda")
        per0 = torch.full((nh,), 5, dtype=torch.int32, device="cuda")
        rc = T._n.lib().ta_hamming_search_cross(nd._ref(), nd.n, hs._ref(), hs.n, k, None, count0.data_ptr(), 0,
                                                near0.data_ptr() if use[0] else None, best0.data_ptr() if use[1] else None,
                                                per0.data_ptr() if use[2] else None, None)
        torch.cuda.synchronize()
        assert rc == 0 and int(count0.item()) == len(want[0]), use
        assert [int(w) for w in near0.cpu().numpy().view(np.uint64)] == (want[1] if use[0] else [5] * nh), use
        rows = [(int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF) for r in best0.cpu().numpy().view(np.uint64)]
        assert rows == (want[2] if use[1] else [(5, 5, 5)] * nh), use
        assert [int(c) for c in per0.cpu().numpy().view(np.uint32)] == (want[3] if use[2] else [5] * nh), use


def test_empty_sides():
    torch, T, B = _mods()
    some = B.Strings.from_list([b"ACGT", b"AC", b"T\x00T"])
    none = B.Strings.from_list([])
    for nd, hs in ((some, none), (none, some), (none, none)):
        n = max(hs.n, 1)
        count = torch.full((1,), 9, dtype=torch.int64, device="cuda")
        nearest = torch.full((n,), 9, dtype=torch.int64, device="cuda")
        best = torch.full((n, 3), 9, dtype=torch.int64, device="cuda")
        per = torch.full((n,), 9, dtype=torch.int32, device="cuda")
        B.hamming_search_cross(nd, hs, 3, cap=4, count=count, nearest=nearest, best=best, per_haystack=per)
        torch.cuda.synchronize()
        assert int(count.item()) == 0
        assert (nearest[:hs.n] == -1).all() and (per[:hs.n] == 0).all()
        assert best[:hs.n].cpu().tolist() == [[0, 0, 0xFFFFFFFF]] * hs.n


def test_limits_and_the_error_order():
    torch, T, B = _mods()
    N = T._n
    hs = B.Strings.from_list([b"ACGTACGTACGT"])
    with pytest.raises(NotImplementedError, match="32 bytes"):
        B.hamming_search_cross(B.Strings.from_list([b"A" * 33]), hs, 2)
    long_measured = B.Strings.from_list([b"A" * 10, b"C" * 33])
    long_measured.max_len = 0
    with pytest.raises(NotImplementedError, match="32 bytes"):
        B.hamming_search_cross(long_measured, hs, 2)
    many = B.Strings.from_fixed(np.full((65536, 4), 65, np.uint8))
    with pytest.raises(NotImplementedError, match="65,535"):
        B.hamming_search_cross(many, hs, 1, cap=0)
    ok = B.Strings.from_fixed(np.full((65535, 4), 65, np.uint8))   # the largest panel: 1,024 groups
    _, count, *_ = B.hamming_search_cross(ok, B.Strings.from_list([b"TTAAAATT", b"CCCC", b"AA"]), 0, cap=0)
    assert int(count.item()) == 65535
    # the order: NULL arguments, the buffers, the limits
    nd = B.Strings.from_list([b"ACGT"])
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib = N.lib()
    long_needle = B.Strings.from_list([b"A" * 33])

    def call(needles, haystacks, cnt, cap=0, hits=None):
        return lib.ta_hamming_search_cross(needles, 1, haystacks, 1, 2, hits, cnt, cap, None, None, None, None)

    assert call(None, hs._ref(), count.data_ptr()) == N.TA_ERR_ARG
    assert call(long_needle._ref(), None, count.data_ptr()) == N.TA_ERR_ARG
    assert call(long_needle._ref(), hs._ref(), None) == N.TA_ERR_ARG
    assert call(long_needle._ref(), hs._ref(), count.data_ptr(), cap=4) == N.TA_ERR_ARG
    assert call(long_needle._ref(), hs._ref(), count.data_ptr(), cap=1 << 60, hits=count.data_ptr()) == N.TA_ERR_ARG
    assert call(long_needle._ref(), hs._ref(), count.data_ptr()) == N.TA_ERR_UNSUPPORTED
    assert call(nd._ref(), hs._ref(), count.data_ptr()) == N.TA_OK
    torch.cuda.synchronize()
    assert int(count.item()) == 1                                  # ACGT in ACGTACGTACGT within 2


def test_forced_haystacks_per_workgroup_equal_the_unforced_result(monkeypatch):
    """513 reads: TA_HSEARCH_CROSS_HPW makes a wavefront walk several steps, the last one ragged"""
    torch, T, B = _mods()
    for nn in (33, 12, 130):
        needles = X.panel(1400 + nn, nn)
        hays = X.reads(1401 + nn, 513, needles)
        nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
        want = _check(B, torch, T, nd, hs, needles, hays, 2)
        for hpw in ("1", "100", "513"):
            monkeypatch.setenv("TA_HSEARCH_CROSS_HPW", hpw)        # (read at every call under TA_TUNING)
            forced = _check(B, torch, T, nd, hs, needles, hays, 2)
            monkeypatch.delenv("TA_HSEARCH_CROSS_HPW")
            assert forced is want


def test_streams_repeated_calls_and_graph_replay():
    torch, T, B = _mods()
    needles = X.panel(1200, 33)
    variants = [X.reads(1201 + v, 130, needles, lo=100, hi=180) for v in range(3)]
    nh, hl = 130, 180
    nd = B.Strings.from_list(needles)
    hblob = torch.zeros(nh * hl + 16, dtype=torch.uint8, device="cuda")
    hoff = torch.zeros(nh + 1, dtype=torch.int64, device="cuda")

    def put(v):
        data = b"".join(variants[v])
        hblob[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        hoff[1:] = torch.from_numpy(np.cumsum([len(s) for s in variants[v]])).cuda()

    hs = B.Strings(hblob, hoff, max_len=hl)                         # CSR with the bound given: no synchronisation
    cap = len(needles) * nh
    for k in (2, 9):
        want = lambda v: (lambda j: (j[0], len(j[0]), j[1], j[2], j[3]))(X.join(needles, variants[v], k))   # noqa: E731
        kw = dict(nearest=True, best=True, per_haystack=True)
        s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            put(0)
            out = B.hamming_search_cross(nd, hs, k, cap=cap, **kw)                     # a stream of its own
            s.synchronize()
            assert _got(B, torch, out) == want(0)
            with torch.cuda.stream(s2):                            # a second stream, buffers of its own, while the first goes on
                out2 = B.hamming_search_cross(nd, hs, k, cap=cap, **kw)
            reuse = dict(hits=out[0], count=out[1], nearest=out[2], best=out[3], per_haystack=out[4])
            for _ in range(2):                                     # back to back into the same buffers
                B.hamming_search_cross(nd, hs, k, cap=cap, **reuse)
            s.synchronize()
            s2.synchronize()
            assert _got(B, torch, out) == want(0) and _got(B, torch, out2) == want(0)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                B.hamming_search_cross(nd, hs, k, cap=cap, **reuse)
            for v in (1, 2):
                put(v)
                graph.replay()
                s.synchronize()
                assert _got(B, torch, out) == want(v), v           # every output read after each replay


def test_python_helpers_equal_a_double_loop_of_single_calls():
    torch, T, B = _mods()
    needles = X.panel(1300, 12)
    hays = [h for h in X.reads(1301, 30, needles) if 0 not in h]
    for k in (1, 3, 40):
        want, nearest = [], []
        for i, h in enumerate(hays):
            row = []
            for p, nd in enumerate(needles):
                r = list(T.hamming_search_simd_with_opts(nd, h, k, T.SearchType.Best))
                if r:
                    want.append((i, p, r[0], len(r)))
                    row.append((r[0].k, p, r[0]))
            nearest.append((min(row)[1], min(row)[2], len(row)) if row else (None, None, 0))
        assert T.hamming_search_cross_many(needles, hays, k) == want and len(want) > 20
        assert T.hamming_search_nearest_many(needles, hays, k) == nearest
    # more hits than the first call's room: one more call with room for the count
    many = [b"ACGT"] * 40
    got = T.hamming_search_cross_many(many, [b"TTACGTTT"] * 40, 0)
    assert got == [(i, p, T.Match(2, 6, 0), 1) for i in range(40) for p in range(40)]
    assert T.hamming_search_cross_many([], many, 1) == [] and T.hamming_search_nearest_many([], [b"AC"], 1) == [(None, None, 0)]
    # PanicError where a single call would: a NUL byte in a read that is not shorter than some non-empty needle
    with pytest.raises(T.PanicError):
        list(T.hamming_search_simd_with_opts(b"ACGT", b"TTAC\x00TTT", 1, T.SearchType.Best))
    for fn in (T.hamming_search_cross_many, T.hamming_search_nearest_many):
        with pytest.raises(T.PanicError):
            fn([b"ACGT", b"ACGTACGTACGT"], [b"TTACGTTT", b"TTAC\x00TTT"], 1)
        fn([b"ACGTACGTACGT"], [b"TTACGTTT", b"TTAC\x00TTT"], 1)    # shorter than the only needle: the single call does not panic either


def test_equals_a_loop_of_shared_needle_search_batch_calls():
    """what a caller did before: hamming_search_batch(Strings.shared(needle), ..., Best, cap=1) once per needle, reduced on the host"""
    torch, T, B = _mods()
    needles, hays = _std()
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    for k in (2, 5):
        recs, nul = [], set()
        for p, needle in enumerate(needles):
            m, c = B.hamming_search_batch(B.Strings.shared(needle, len(hays)), hs, k, T.SearchType.Best, cap=1)
            torch.cuda.synchronize()
            m, c = m.cpu().numpy(), c.cpu().numpy()
            nul |= {i for i in range(len(hays)) if c[i] < 0}
            recs += [(i, p, int(m[i, 0, 0]), int(m[i, 0, 1]), int(m[i, 0, 2]) & 0xFFFFFFFF, int(c[i])) for i in range(len(hays)) if c[i] > 0]
        recs.sort()
        near = [min((r[4] << 32 | r[1] for r in recs if r[0] == i), default=X.ALL_ONES) for i in range(len(hays))]
        out = B.hamming_search_cross(nd, hs, k, cap=len(needles) * len(hays), nearest=True, best=True, per_haystack=True)
        got = _got(B, torch, out)
        assert got[0] == recs and got[1] == len(recs) and got[2] == near
        assert got[4] == [X.NONE if i in nul else sum(1 for r in recs if r[0] == i) for i in range(len(hays))]
        assert nul and got[0] == X.join(needles, hays, k)[0]
