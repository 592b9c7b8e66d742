"""gpu: every needle of a panel of needles up to 64 bytes in every haystack within k (ta_levenshtein_search_cross_with_opts) against the
oracle levenshtein_search_naive_with_opts over EVERY (needle, haystack) pair of every batch -- sorted records, count, nearest, best and
per-haystack -- with the joins memoised per batch (tests/search_cross_cases.py, tests/search_cross_opts_cases.py): batch sizes on both
sides of the wavefront edges times panel sizes on both sides of the 32-needle group, needle lengths on both sides of the word boundary,
the eight cost sets anchored and not, strided and CSR sides, cap cutting, every optional output left out in turn, empty sides, the
hand-made two-word pairs, the routing of short panels to ta_levenshtein_search_cross's kernels, forced sub-batches, streams, repeated
calls, graph capture, the Python helpers, and the loop of shared-needle levenshtein_search_batch calls it replaces."""
import ctypes as C

import numpy as np
import pytest

import datagen as Dg
import search_cross_cases as X
import search_cross_opts_cases as Y

pytestmark = pytest.mark.gpu

NHS = (1, 65, 257)
NNS = (1, 5, 31, 32, 33, 65, 96)
SCAN, EXACT = "lev_search_cross_w2_scan_kernel<%s>", "lev_search_cross_w2_exact_kernel<%s>"


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


def _run(B, torch, nd, hs, k, costs, anchored=False, entry=None):
    entry = entry or B.levenshtein_search_cross_with_opts
    return _got(B, torch, entry(nd, hs, k, costs, anchored, cap=max(nd.n * hs.n, 1), nearest=True, best=True, per_haystack=True))


def _check(B, torch, nd, hs, needles, hays, k, costs, anchored=False):
    want = X.join(needles, hays, k, costs, anchored)
    got = _run(B, torch, nd, hs, k, costs, anchored)
    where = (len(needles), len(hays), k, costs, anchored)
    assert got[1] == len(want[0]) and got[0] == want[0], where
    assert got[2] == want[1], where
    assert got[3] == want[2], where
    assert got[4] == want[3], where
    return want


def _two_word_route(T, needles, costs, anchored):
    """a panel whose longest needle is beyond 32 bytes took the two-word kernels; a shorter one did not"""
    name = T.last_kernel_name()
    if max(map(len, needles)) > 32:
        assert name == (EXACT if anchored else SCAN) % ("true" if costs[3] is not None else "false"), name
    else:
        assert "w2" not in name, name


def _std():
    """the batch most tests share: 33 needles of every length of LONG_LENS (two groups: 32 + 1), 65 reads"""
    needles = Y.panel(133, 33)
    return needles, X.reads(233, 65, needles)


@pytest.mark.parametrize("k", [0, 3, 40])
@pytest.mark.parametrize("nn", NNS)
@pytest.mark.parametrize("nh", NHS)
def test_every_pair_equals_the_oracle(nh, nn, k):
    """needle lengths on both sides of the word boundary in one panel; at k = 40 the needles of up to 40 bytes are unscanned (kf >= n)
    beside scanned long ones in one group"""
    torch, T, B = _mods()
    needles = Y.panel(300 + nn, nn)
    hays = X.reads(400 + nn, nh, needles)
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    for costs in (Y.LEVENSHTEIN, Y.RDAMERAU):
        _check(B, torch, nd, hs, needles, hays, k, costs)
        _two_word_route(T, needles, costs, False)


@pytest.mark.parametrize("costs", X.COSTS)
def test_every_cost_set_anchored_and_not(costs):
    torch, T, B = _mods()
    needles, hays = _std()
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    for anchored in (False, True):
        for k in (0, 3, 9):
            _check(B, torch, nd, hs, needles, hays, k, costs, anchored)
            _two_word_route(T, needles, costs, anchored)
    al = X.BYTES                                                   # bytes 0..255
    needles = Y.panel(134, 16, al)
    hays = X.reads(234, 64, needles, al)
    _check(B, torch, B.Strings.from_list(needles), B.Strings.from_list(hays), needles, hays, 4, costs)


@pytest.mark.parametrize("nform", ["strided", "csr", "csr_unmeasured"])
@pytest.mark.parametrize("hform", ["strided", "csr", "csr_unmeasured"])
def test_strided_and_csr_sides(nform, hform):
    torch, T, B = _mods()
    g = Dg.rng(1100)
    needles = [bytes(g.choice(X.ACGT, 40)) for _ in range(20)]     # the strided needle side: 40 bytes fixed
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
    for costs in (X.COSTS[0], X.COSTS[5]):
        for anchored in (False, True):
            want = _check(B, torch, nd, hs, needles, hays, 3, costs, anchored)
            _two_word_route(T, needles, costs, anchored)
            assert anchored or len(want[0]) >= 30


def test_cap_cuts_the_records_not_the_count_and_every_optional_output():
    torch, T, B = _mods()
    needles, hays = _std()
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    k, costs = 3, X.COSTS[0]
    want = X.join(needles, hays, k, costs, False)
    assert len(want[0]) >= 64
    cap = len(want[0]) // 2
    out = B.levenshtein_search_cross_with_opts(nd, hs, k, costs, cap=cap, nearest=True, best=True, per_haystack=True)
    recs, n, near, best, per = _got(B, torch, out, cut=True)
    assert n == len(want[0])                                       # the count is unchanged
    assert len(recs) == cap and len(set(r[:2] for r in recs)) == cap   # no record twice
    assert set(recs) <= set(want[0])                               # every record is a true hit
    assert near == want[1] and best == want[2] and per == want[3]  # none depends on cap
    with pytest.raises(ValueError, match="larger cap"):
        B.search_cross_to_arrays(out[0], out[1])
    # cap = 0 with a NULL hits buffer, then each optional output NULL in turn (best without nearest included)
    nh = len(hays)
    for use in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 1, 0), (1, 0, 0), (0, 0, 1), (0, 0, 0)):
        count0 = torch.full((1,), 5, dtype=torch.int64, device="cuda")
        near0 = torch.full((nh,), 5, dtype=torch.int64, device="cuda")
        best0 = torch.full((nh, 3), 5, dtype=torch.int64, device="cuda")
        per0 = torch.full((nh,), 5, dtype=torch.int32, device="cuda")
        cc = T._costs(costs)._c()
        rc = T._n.lib().ta_levenshtein_search_cross_with_opts(nd._ref(), nd.n, hs._ref(), hs.n, k, C.byref(cc), 0, 0, None, count0.data_ptr(), 0,
                                                              near0.data_ptr() if use[0] else None, best0.data_ptr() if use[1] else None,
                                                              per0.data_ptr() if use[2] else None, None)
        torch.cuda.synchronize()
        assert rc == 0 and int(count0.item()) == len(want[0]), use
        assert [int(w) for w in near0.cpu().numpy().view(np.uint64)] == (want[1] if use[0] else [5] * nh), use
        rows = [(int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF) for r in best0.cpu().numpy().view(np.uint64)]
        assert rows == (want[2] if use[1] else [(5, 5, 5)] * nh), use
        assert per0.cpu().tolist() == (want[3] if use[2] else [5] * nh), use


def test_empty_sides():
    torch, T, B = _mods()
    some = B.Strings.from_list([b"ACGT" * 12, b"AC", b"TTT"])
    none = B.Strings.from_list([])
    for nd, hs in ((some, none), (none, some), (none, none)):
        for anchored in (False, True):
            n = max(hs.n, 1)
            count = torch.full((1,), 9, dtype=torch.int64, device="cuda")
            nearest = torch.full((n,), 9, dtype=torch.int64, device="cuda")
            best = torch.full((n, 3), 9, dtype=torch.int64, device="cuda")
            per = torch.full((n,), 9, dtype=torch.int32, device="cuda")
            B.levenshtein_search_cross_with_opts(nd, hs, 3, anchored=anchored, cap=4, count=count, nearest=nearest, best=best, per_haystack=per)
            torch.cuda.synchronize()
            assert int(count.item()) == 0
            assert (nearest[:hs.n] == -1).all() and (per[:hs.n] == 0).all()
            assert best[:hs.n].cpu().tolist() == [[0, 0, 0xFFFFFFFF]] * hs.n


def test_hand_made_pairs_where_two_words_can_go_wrong():
    torch, T, B = _mods()
    needles, hays = Y.hand_made()
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    for costs in (Y.LEVENSHTEIN, Y.RDAMERAU, X.COSTS[5]):
        for anchored in (False, True):
            for k in (0, 1, 2, 3):
                _check(B, torch, nd, hs, needles, hays, k, costs, anchored)
                _two_word_route(T, needles, costs, anchored)
    recs = {r[:2]: r for r in _run(B, torch, nd, hs, 1, Y.RDAMERAU)[0]}
    assert recs[(0, 0)][4] == 0 and recs[(1, 1)][4] == 1 and recs[(2, 2)][4] == 1 and recs[(3, 3)][4] == 1 and recs[(4, 4)][4] == 1
    assert (2, 2) not in {r[:2] for r in _run(B, torch, nd, hs, 1, Y.LEVENSHTEIN)[0]}


def test_limits_flags_and_exceptions():
    torch, T, B = _mods()
    N = T._n
    hs = B.Strings.from_list([b"ACGTACGTACGT" * 8])
    ok = B.Strings.from_list([b"A" * 64])
    _, count, *_ = B.levenshtein_search_cross_with_opts(ok, hs, 60, cap=0)
    assert int(count.item()) == 1
    with pytest.raises(NotImplementedError, match="64 bytes"):
        B.levenshtein_search_cross_with_opts(B.Strings.from_list([b"A" * 65]), hs, 2)
    long_measured = B.Strings.from_list([b"A" * 10, b"C" * 65])
    long_measured.max_len = 0
    with pytest.raises(NotImplementedError, match="64 bytes"):
        B.levenshtein_search_cross_with_opts(long_measured, hs, 2)
    many = B.Strings.from_fixed(np.full((65536, 4), 65, np.uint8))
    with pytest.raises(NotImplementedError, match="65,535"):
        B.levenshtein_search_cross_with_opts(many, hs, 1, cap=0)
    with pytest.raises(T.PanicError):
        B.levenshtein_search_cross_with_opts(ok, hs, 2, (1, 0, 0, None))       # check_search: a free gap
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    good, bad = N.EditCostsC(1, 1, 0, 0, 0), N.EditCostsC(0, 1, 0, 0, 0)

    def call(costs, flags):
        return N.lib().ta_levenshtein_search_cross_with_opts(ok._ref(), 1, hs._ref(), 1, 2, costs, 0, flags, None, count.data_ptr(), 0, None, None, None, None)

    assert call(C.byref(bad), 1) == N.TA_ERR_ARG                   # the flags word comes before the costs
    assert call(C.byref(good), 4) == N.TA_ERR_ARG
    assert call(C.byref(bad), 0) == N.TA_ERR_BAD_COSTS
    assert call(C.byref(good), 0) == N.TA_OK
    torch.cuda.synchronize()


def test_a_short_panel_takes_the_32_byte_entrys_kernels():
    """longest needle <= 32: output for output what levenshtein_search_cross gives, by the same kernels; that entry still refuses 33 bytes"""
    torch, T, B = _mods()
    needles = X.panel(900, 33)                                     # search_cross_cases' lengths: 0 .. 32
    hays = X.reads(901, 65, needles)
    assert max(map(len, needles)) == 32
    fixed = [bytes(Dg.rng(902).choice(X.ACGT, 24)) for _ in range(20)]
    for nd, strings in ((B.Strings.from_list(needles), needles), (B.Strings.from_fixed(np.frombuffer(b"".join(fixed), np.uint8).reshape(20, 24)), fixed)):
        hs = B.Strings.from_list(hays)
        for costs, anchored in ((X.COSTS[0], False), (X.COSTS[5], False), (X.COSTS[0], True), (X.COSTS[1], True)):
            old = _run(B, torch, nd, hs, 3, costs, anchored, entry=B.levenshtein_search_cross)
            old_name = T.last_kernel_name()
            new = _run(B, torch, nd, hs, 3, costs, anchored)
            assert T.last_kernel_name() == old_name and "w2" not in old_name, (old_name, T.last_kernel_name())
            assert new == old
            want = X.join(strings, hays, 3, costs, anchored)
            assert new == (want[0], len(want[0]), want[1], want[2], want[3])
    longer = Y.panel(133, 33)
    with pytest.raises(NotImplementedError, match="32 bytes"):
        B.levenshtein_search_cross(B.Strings.from_list(longer), B.Strings.from_list(hays), 3)
    with pytest.raises(NotImplementedError, match="32 bytes"):
        B.levenshtein_search_cross(B.Strings.from_list([b"A" * 33]), B.Strings.from_list(hays), 3)


def test_forced_sub_batches_equal_the_unforced_result(monkeypatch):
    torch, T, B = _mods()
    needles = Y.panel(900, 33)
    hays = X.reads(901, 257, needles)
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    for costs, anchored in ((X.COSTS[0], False), (X.COSTS[5], False), (X.COSTS[0], True)):
        want = _check(B, torch, nd, hs, needles, hays, 3, costs, anchored)
        monkeypatch.setenv("TA_SEARCH_CROSS_SUB", "64")            # (read at every call under TA_TUNING: 64 + 64 + 64 + 64 + 1 haystacks)
        forced = _check(B, torch, nd, hs, needles, hays, 3, costs, anchored)
        monkeypatch.delenv("TA_SEARCH_CROSS_SUB")
        assert forced is want


def test_streams_repeated_calls_and_graph_replay():
    torch, T, B = _mods()
    needles = Y.panel(1200, 33)
    variants = [X.reads(1201 + v, 65, needles, lo=100, hi=180) for v in range(3)]
    nh, hl = 65, 180
    nd = B.Strings.from_list(needles)
    hblob = torch.zeros(nh * hl + 16, dtype=torch.uint8, device="cuda")
    hoff = torch.zeros(nh + 1, dtype=torch.int64, device="cuda")

    def put(v):
        data = b"".join(variants[v])
        hblob[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        hoff[1:] = torch.from_numpy(np.cumsum([len(s) for s in variants[v]])).cuda()

    hs = B.Strings(hblob, hoff, max_len=hl)                         # CSR with the bound given: no synchronisation
    cap = len(needles) * nh
    fn = B.levenshtein_search_cross_with_opts
    for costs, anchored in ((X.COSTS[0], False), (X.COSTS[5], True)):
        want = lambda v: (lambda j: (j[0], len(j[0]), j[1], j[2], j[3]))(X.join(needles, variants[v], 3, costs, anchored))   # noqa: E731
        kw = dict(nearest=True, best=True, per_haystack=True)
        s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            put(0)
            out = fn(nd, hs, 3, costs, anchored, cap=cap, **kw)    # a stream of its own (and the run outside the capture)
            s.synchronize()
            assert _got(B, torch, out) == want(0)
            with torch.cuda.stream(s2):                            # a second stream, buffers of its own, while the first goes on
                out2 = fn(nd, hs, 3, costs, anchored, cap=cap, **kw)
            reuse = dict(hits=out[0], count=out[1], nearest=out[2], best=out[3], per_haystack=out[4])
            for _ in range(2):                                     # back to back into the same buffers
                fn(nd, hs, 3, costs, anchored, cap=cap, **reuse)
            s.synchronize()
            s2.synchronize()
            assert _got(B, torch, out) == want(0) and _got(B, torch, out2) == want(0)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                fn(nd, hs, 3, costs, anchored, cap=cap, **reuse)
            put(1)
            graph.replay()                                         # one replay, on other haystacks
            s.synchronize()
            assert _got(B, torch, out) == want(1)


def test_python_helpers_equal_a_double_loop_of_single_calls():
    torch, T, B = _mods()
    needles = X.panel(1300, 5, lens=(33, 64, 8, 47, 32))
    hays = X.reads(1301, 9, needles)
    assert sorted(map(len, needles)) == [8, 32, 33, 47, 64]
    for costs, anchored in ((T.LEVENSHTEIN_COSTS, False), (T.EditCosts(2, 2, 1, 3), False), (T.RDAMERAU_COSTS, True)):
        want, nearest = [], []
        for i, h in enumerate(hays):
            row = []
            for p, nd in enumerate(needles):
                r = list(T.levenshtein_search_simd_with_opts(nd, h, 3, T.SearchType.Best, costs, anchored))
                if r:
                    want.append((i, p, r[0], len(r)))
                    row.append((r[0].k, p, r[0]))
            nearest.append((min(row)[1], min(row)[2], len(row)) if row else (None, None, 0))
        assert T.levenshtein_search_cross_with_opts_many(needles, hays, 3, costs, anchored) == want and (anchored or len(want) > 4)
        assert T.levenshtein_search_nearest_with_opts_many(needles, hays, 3, costs, anchored) == nearest
    # more hits than the first call's room: one more call with room for the count
    many = [b"ACGT" * 9] * 40
    got = T.levenshtein_search_cross_with_opts_many(many, [b"TT" + b"ACGT" * 9 + b"TT"] * 40, 0)
    assert got == [(i, p, T.Match(2, 38, 0), 1) for i in range(40) for p in range(40)]
    assert T.levenshtein_search_cross_with_opts_many([], many, 1) == []
    assert T.levenshtein_search_nearest_with_opts_many([], [b"AC"], 1) == [(None, None, 0)]


def test_equals_a_loop_of_shared_needle_search_batch_calls():
    """what a caller with long needles did before: levenshtein_search_batch(Strings.shared(needle), ..., Best) once per needle"""
    torch, T, B = _mods()
    needles, hays = _std()
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    for costs, anchored in ((X.COSTS[0], False), (X.COSTS[6], False), (X.COSTS[4], True)):
        recs = []
        for p, needle in enumerate(needles):
            m, c = B.levenshtein_search_batch(B.Strings.shared(needle, len(hays)), hs, 3, T.SearchType.Best, costs, anchored, cap=1)
            torch.cuda.synchronize()
            m, c = m.cpu().numpy(), c.cpu().numpy()
            recs += [(i, p, int(m[i, 0, 0]), int(m[i, 0, 1]), int(m[i, 0, 2]) & 0xFFFFFFFF, int(c[i])) for i in range(len(hays)) if c[i]]
        recs.sort()
        near = [min((r[4] << 32 | r[1] for r in recs if r[0] == i), default=X.ALL_ONES) for i in range(len(hays))]
        got = _run(B, torch, nd, hs, 3, costs, anchored)
        assert got[0] == recs and got[1] == len(recs) and got[2] == near
        assert got[4] == [sum(1 for r in recs if r[0] == i) for i in range(len(hays))]
        assert got[0] == X.join(needles, hays, 3, costs, anchored)[0]
