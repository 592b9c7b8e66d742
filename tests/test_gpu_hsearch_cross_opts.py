"""gpu: every needle of a panel of needles up to 64 bytes in every haystack within k mismatches (ta_hamming_search_cross_with_opts)
against the oracle hamming_search_simd_with_opts(.., Best) over EVERY (needle, haystack) pair of every batch -- sorted records, count,
nearest, best and per-haystack with its NUL mark -- with the joins memoised per batch (tests/hsearch_cross_opts_cases.py; the conditions
these comparisons rely on are asserted on the join alone in tests/test_hsearch_cross_opts_cpu.py): read counts times panel sizes times k,
every plane count 1..7, the route and its kernel name on both sides of 32 bytes, strided and CSR sides, bytes 1..255, cap cutting,
counting only, every optional output left out in turn, empty sides, the hand-made pairs around the word boundary, the error order, forced
haystacks per workgroup, streams, repeated calls, graph capture, the Python helpers, and the loop of shared-needle hamming_search_batch
calls it replaces."""
import os
import subprocess
import sys

import numpy as np
import pytest

import datagen as Dg
import hsearch_cross_cases as X
import hsearch_cross_opts_cases as Y

pytestmark = pytest.mark.gpu

NHS = (1, 65, 257)
KS = (0, 3, 33, 70)


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


def _kernel(k, needles):
    if max(map(len, needles)) > 32:
        return "ham_search_cross_w2_kernel<%d>" % Y.planes(k, needles)
    return "ham_search_cross_kernel<%d>" % X.planes(k, needles)


def _check(B, torch, T, nd, hs, needles, hays, k):
    want = Y.join(needles, hays, k)
    out = B.hamming_search_cross_with_opts(nd, hs, k, cap=max(len(needles) * len(hays), 1), nearest=True, best=True, per_haystack=True)
    got = _got(B, torch, out)
    where = (len(needles), len(hays), k)
    assert got[1] == len(want[0]) and got[0] == want[0], where
    assert got[2] == want[1], where
    assert got[3] == want[2], where
    assert got[4] == want[3], where
    assert T.last_kernel_name() == _kernel(k, needles), (T.last_kernel_name(), where)
    return want


@pytest.mark.parametrize("nn", Y.PANELS)
@pytest.mark.parametrize("nh", NHS)
def test_every_pair_equals_the_oracle(nh, nn):
    """mixed needle lengths 0..64 (k >= n and k < n in one group), every haystack length class, NUL reads, at every k of KS"""
    torch, T, B = _mods()
    needles = Y.panel(300 + nn, nn)
    hays = Y.reads(400 + nn, nh, needles)
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    total = 0
    for k in KS:
        total += len(_check(B, torch, T, nd, hs, needles, hays, k)[0])
        if max(map(len, needles)) == 64:
            assert T.last_kernel_name() == "ham_search_cross_w2_kernel<%d>" % Y.PLANES_AT_64[k]
    assert total > 0


@pytest.mark.parametrize("k,planes", [(5, 3), (8, 4), (31, 5), (64, 7)])
def test_the_remaining_plane_counts(k, planes):
    torch, T, B = _mods()
    needles, hays = Y.std()
    _check(B, torch, T, B.Strings.from_list(needles), B.Strings.from_list(hays), needles, hays, k)
    assert T.last_kernel_name() == "ham_search_cross_w2_kernel<%d>" % planes


def test_the_route_follows_the_longest_needle():
    """a panel of needles up to 32 bytes: the one-word kernel under its own name, results equal to hamming_search_cross; one 33-byte
    needle more: the two-word kernel for the whole panel, the short needles' records unchanged"""
    torch, T, B = _mods()
    short = X.panel(910, 40)
    assert max(map(len, short)) == 32
    hays = X.reads(911, 130, short)
    hs = B.Strings.from_list(hays)
    g = Dg.rng(912)
    longer = short + [bytes(g.choice(X.ACGT, 33))]
    kw = dict(cap=len(longer) * len(hays), nearest=True, best=True, per_haystack=True)
    for k in (2, 9, 40):
        old = _got(B, torch, B.hamming_search_cross(B.Strings.from_list(short), hs, k, **kw))
        assert T.last_kernel_name() == "ham_search_cross_kernel<%d>" % X.planes(k, short)
        new = _got(B, torch, B.hamming_search_cross_with_opts(B.Strings.from_list(short), hs, k, **kw))
        assert T.last_kernel_name() == "ham_search_cross_kernel<%d>" % X.planes(k, short)
        assert new == old and len(old[0]) > 0
        want = _check(B, torch, T, B.Strings.from_list(longer), hs, longer, hays, k)
        assert T.last_kernel_name() == "ham_search_cross_w2_kernel<%d>" % Y.planes(k, longer)
        assert [r for r in want[0] if r[1] < len(short)] == old[0]


@pytest.mark.parametrize("nform", ["strided", "csr", "csr_unmeasured"])
@pytest.mark.parametrize("hform", ["strided", "csr", "csr_unmeasured"])
def test_strided_and_csr_sides(nform, hform):
    torch, T, B = _mods()
    g = Dg.rng(1100)
    needles = [bytes(g.choice(X.ACGT, 40)) for _ in range(20)]     # 40-byte strided needles
    hays = [h[:121] for h in X.reads(1101, 65, needles, lo=121, hi=250) if len(h) >= 121]      # 121 bytes: every string at another alignment
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


def test_bytes_1_to_255():
    torch, T, B = _mods()
    needles = Y.panel(134, 16, Y.BYTES)
    assert max(map(len, needles)) > 32
    hays = Y.reads(234, 64, needles, Y.BYTES)
    for k in (0, 2, 9):
        want = _check(B, torch, T, B.Strings.from_list(needles), B.Strings.from_list(hays), needles, hays, k)
        assert len(want[0]) > 10


def test_cap_cuts_the_records_not_the_count_and_every_optional_output():
    torch, T, B = _mods()
    needles, hays = Y.std()
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    k = 3
    want = Y.join(needles, hays, k)
    assert len(want[0]) >= 64
    cap = len(want[0]) // 2
    out = B.hamming_search_cross_with_opts(nd, hs, k, cap=cap, nearest=True, best=True, per_haystack=True)
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
        rc = T._n.lib().ta_hamming_search_cross_with_opts(nd._ref(), nd.n, hs._ref(), hs.n, k, 0, None, count0.data_ptr(), 0,
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
    some = B.Strings.from_list([b"ACGT" * 12, b"AC", b"T\x00T"])
    none = B.Strings.from_list([])
    for nd, hs in ((some, none), (none, some), (none, none)):
        n = max(hs.n, 1)
        count = torch.full((1,), 9, dtype=torch.int64, device="cuda")
        nearest = torch.full((n,), 9, dtype=torch.int64, device="cuda")
        best = torch.full((n, 3), 9, dtype=torch.int64, device="cuda")
        per = torch.full((n,), 9, dtype=torch.int32, device="cuda")
        B.hamming_search_cross_with_opts(nd, hs, 3, cap=4, count=count, nearest=nearest, best=best, per_haystack=per)
        torch.cuda.synchronize()
        assert int(count.item()) == 0
        assert (nearest[:hs.n] == -1).all() and (per[:hs.n] == 0).all()
        assert best[:hs.n].cpu().tolist() == [[0, 0, 0xFFFFFFFF]] * hs.n


def test_hand_made_pairs_around_the_word_boundary():
    torch, T, B = _mods()
    cases = Y.hand_made()
    for tag, nd, hay, k, want in cases:
        out = B.hamming_search_cross_with_opts(B.Strings.from_list([nd]), B.Strings.from_list([hay]), k, cap=4)
        recs = _got(B, torch, out)[0]
        assert recs == ([] if want is None else [(0, 0) + want]), tag
    needles, hays = [c[1] for c in cases[::7]] + [b"ACGT"], [c[2] for c in cases]
    for k in sorted({c[3] for c in cases}):
        _check(B, torch, T, B.Strings.from_list(needles), B.Strings.from_list(hays), needles, hays, k)


def test_limits_and_the_error_order():
    torch, T, B = _mods()
    N = T._n
    hs = B.Strings.from_list([b"ACGTACGTACGT" * 8])
    with pytest.raises(NotImplementedError, match="64 bytes"):
        B.hamming_search_cross_with_opts(B.Strings.from_list([b"A" * 65]), hs, 2)
    long_measured = B.Strings.from_list([b"A" * 10, b"C" * 65])
    long_measured.max_len = 0
    with pytest.raises(NotImplementedError, match="64 bytes"):
        B.hamming_search_cross_with_opts(long_measured, hs, 2)
    many = B.Strings.from_fixed(np.full((65536, 4), 65, np.uint8))
    with pytest.raises(NotImplementedError, match="65,535"):
        B.hamming_search_cross_with_opts(many, hs, 1, cap=0)
    ok = B.Strings.from_fixed(np.full((65535, 33), 65, np.uint8))  # the largest panel on the two-word route: 2,048 groups
    _, count, *_ = B.hamming_search_cross_with_opts(ok, B.Strings.from_list([b"TT" + b"A" * 34 + b"TT", b"CCCC", b"AA"]), 0, cap=0)
    assert int(count.item()) == 65535 and T.last_kernel_name() == "ham_search_cross_w2_kernel<1>"
    # the order: NULL arguments, the flags, the buffers, the limits
    nd = B.Strings.from_list([b"ACGT" * 10])
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib = N.lib()
    too_long = B.Strings.from_list([b"A" * 65])

    def call(needles, haystacks, cnt, flags=0, cap=0, hits=None):
        return lib.ta_hamming_search_cross_with_opts(needles, 1, haystacks, 1, 2, flags, hits, cnt, cap, None, None, None, None)

    assert call(None, hs._ref(), count.data_ptr(), flags=1) == N.TA_ERR_ARG
    assert call(too_long._ref(), None, count.data_ptr()) == N.TA_ERR_ARG
    assert call(too_long._ref(), hs._ref(), None) == N.TA_ERR_ARG
    assert call(nd._ref(), hs._ref(), count.data_ptr(), flags=1) == N.TA_ERR_ARG
    assert call(too_long._ref(), hs._ref(), count.data_ptr(), flags=1) == N.TA_ERR_ARG
    assert call(too_long._ref(), hs._ref(), count.data_ptr(), cap=4) == N.TA_ERR_ARG
    assert call(too_long._ref(), hs._ref(), count.data_ptr(), cap=1 << 60, hits=count.data_ptr()) == N.TA_ERR_ARG
    assert call(too_long._ref(), hs._ref(), count.data_ptr()) == N.TA_ERR_UNSUPPORTED
    assert call(nd._ref(), hs._ref(), count.data_ptr()) == N.TA_OK
    torch.cuda.synchronize()
    assert int(count.item()) == 1                                  # (ACGT)^10 in (ACGT)^24 within 2


_CHILD = r"""
import os
import sys
sys.path.insert(0, sys.argv[1])
import torch
import triple_accel_amd as T
from triple_accel_amd import batch as B
import hsearch_cross_opts_cases as Y
import test_gpu_hsearch_cross_opts as G
for nn in (33, 12):
    needles = Y.panel(1400 + nn, nn)
    assert max(map(len, needles)) > 32
    hays = Y.reads(1401 + nn, 257, needles)
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)
    for hpw in ("1", "100", "257"):
        os.environ["TA_HSEARCH_CROSS_HPW"] = hpw                   # (read at every call under TA_TUNING)
        G._check(B, torch, T, nd, hs, needles, hays, 3)
print("forced ok")
"""


def test_forced_haystacks_per_workgroup_in_a_child_process():
    """257 reads: TA_HSEARCH_CROSS_HPW makes a wavefront walk several steps, the last one ragged -- against the oracle, in a process of
    its own that has TA_TUNING from its start whatever this process was started with"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, TA_TUNING="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, here], env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "forced ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_streams_repeated_calls_and_graph_replay():
    torch, T, B = _mods()
    needles = Y.panel(1200, 33)
    assert max(map(len, needles)) == 64
    variants = [Y.reads(1201 + v, 130, needles, lo=100, hi=180) for v in range(3)]
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
    for k in (3, 40):
        want = lambda v: (lambda j: (j[0], len(j[0]), j[1], j[2], j[3]))(Y.join(needles, variants[v], k))   # noqa: E731
        kw = dict(nearest=True, best=True, per_haystack=True)
        s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s):
            put(0)
            out = B.hamming_search_cross_with_opts(nd, hs, k, cap=cap, **kw)           # a stream of its own (once outside the capture)
            s.synchronize()
            assert _got(B, torch, out) == want(0)
            assert T.last_kernel_name() == "ham_search_cross_w2_kernel<%d>" % Y.planes(k, needles)
            with torch.cuda.stream(s2):                            # a second stream, buffers of its own, while the first goes on
                out2 = B.hamming_search_cross_with_opts(nd, hs, k, cap=cap, **kw)
            reuse = dict(hits=out[0], count=out[1], nearest=out[2], best=out[3], per_haystack=out[4])
            for _ in range(2):                                     # back to back into the same buffers
                B.hamming_search_cross_with_opts(nd, hs, k, cap=cap, **reuse)
            s.synchronize()
            s2.synchronize()
            assert _got(B, torch, out) == want(0) and _got(B, torch, out2) == want(0)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                B.hamming_search_cross_with_opts(nd, hs, k, cap=cap, **reuse)
            for v in (1, 2):
                put(v)
                graph.replay()
                s.synchronize()
                assert _got(B, torch, out) == want(v), v           # every output read after each replay


def test_python_helpers_equal_a_double_loop_of_single_calls():
    torch, T, B = _mods()
    needles = Y.panel(1300, 12)
    assert max(map(len, needles)) > 32
    hays = [h for h in Y.reads(1301, 30, needles) if 0 not in h]
    for k in (1, 3, 70):
        want, nearest = [], []
        for i, h in enumerate(hays):
            row = []
            for p, nd in enumerate(needles):
                r = list(T.hamming_search_simd_with_opts(nd, h, k, T.SearchType.Best))
                if r:
                    want.append((i, p, r[0], len(r)))
                    row.append((r[0].k, p, r[0]))
            nearest.append((min(row)[1], min(row)[2], len(row)) if row else (None, None, 0))
        assert T.hamming_search_cross_with_opts_many(needles, hays, k) == want and len(want) > 20
        assert T.hamming_search_nearest_with_opts_many(needles, hays, k) == nearest
    # more hits than the first call's room: one more call with room for the count
    many = [b"ACGT" * 9] * 40
    got = T.hamming_search_cross_with_opts_many(many, [b"TT" + b"ACGT" * 9 + b"TT"] * 40, 0)
    assert got == [(i, p, T.Match(2, 38, 0), 1) for i in range(40) for p in range(40)]
    assert T.hamming_search_cross_with_opts_many([], many, 1) == []
    assert T.hamming_search_nearest_with_opts_many([], [b"AC"], 1) == [(None, None, 0)]
    with pytest.raises(NotImplementedError, match="64 bytes"):
        T.hamming_search_cross_with_opts_many([b"A" * 65], [b"A" * 100], 1)
    # PanicError where a single call would: a NUL byte in a read that is not shorter than some non-empty needle
    long_nd = b"ACGT" * 9
    for fn in (T.hamming_search_cross_with_opts_many, T.hamming_search_nearest_with_opts_many):
        with pytest.raises(T.PanicError):
            fn([long_nd, b"ACGT"], [b"TT" + long_nd, b"TTAC\x00TTT"], 1)
        fn([long_nd], [b"TT" + long_nd, b"TTAC\x00TTT"], 1)        # shorter than the only needle: the single call does not panic either


def test_equals_a_loop_of_shared_needle_search_batch_calls():
    """what a caller did before: hamming_search_batch(Strings.shared(needle), ..., Best, cap=1) once per needle, reduced on the host --
    65 reads, 5 needles of up to 64 bytes"""
    torch, T, B = _mods()
    needles = Y.panel(1500, 5, lens=(34, 64, 40, 24, 33))
    assert sorted(map(len, needles)) == [24, 33, 34, 40, 64]
    hays = Y.reads(1501, 65, needles)
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
        near = [min((r[4] << 32 | r[1] for r in recs if r[0] == i), default=Y.ALL_ONES) for i in range(len(hays))]
        out = B.hamming_search_cross_with_opts(nd, hs, k, cap=len(needles) * len(hays), nearest=True, best=True, per_haystack=True)
        got = _got(B, torch, out)
        assert T.last_kernel_name() == "ham_search_cross_w2_kernel<%d>" % Y.planes(k, needles)
        assert got[0] == recs and got[1] == len(recs) and got[2] == near
        assert got[4] == [Y.NONE if i in nul else sum(1 for r in recs if r[0] == i) for i in range(len(hays))]
        assert nul and got[0] == Y.join(needles, hays, k)[0]
