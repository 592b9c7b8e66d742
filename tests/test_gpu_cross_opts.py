"""gpu: every query of up to 256 bytes against every target within k (ta_levenshtein_cross_with_opts) against the oracle's
levenshtein_simd_k_with_opts over EVERY pair of every batch: the sorted hit list, the count, the nearest words and the per-query counts.
Batches on both sides of the lane, wavefront and workgroup edges, CSR sides of mixed lengths and strided ones, a k for every window
width and both sides of each switch, both cost families and a multiple; the upper triangle of a set against itself through both
kernels; short queries through the 64-byte body; agreement with ta_levenshtein_cross; cap cutting, counting only, empty sides, streams,
repeated calls, graph capture, and the Python helpers.

Every batch of 65 pairs or more has to show something: the oracle finds at least 16 hits, at least one at distance exactly k, and at
least 16 non-hits pass the length prefilter (targets are planted for each).  At k = 2^32 - 1 every pair is a hit and none is at
distance k: only the first is asserted there."""
import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

pytestmark = pytest.mark.gpu

ALL_ONES = 0xFFFFFFFFFFFFFFFF
NONE = 0xFFFFFFFF
KMAX = 0xFFFFFFFF
ACGT = np.frombuffer(b"ACGT", np.uint8)
LOWER = np.arange(97, 123, dtype=np.uint8)
FOREIGN = np.arange(48, 58, dtype=np.uint8)                        # symbols no query holds: a planted distance is exact
SHAPES = ((1, 1), (1, 65), (65, 130), (131, 257))
KS = (1, 8, 9, 25, 41)                                             # windows of 2, 2, 3, 4 blocks and the whole column


def _mods():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    return torch, T, B


def _kernel():
    import triple_accel_amd as T
    return T._n.lib().ta_last_kernel_name().decode()


def _ww(unit_k):
    need = (2 * unit_k + 15) // 32 + 2
    return 2 if need <= 2 else 3 if need <= 3 else 4 if need <= 4 else 8


def _win_name(unit_k, costs):
    return "lev_cross_win_kernel<%d, %s>" % (_ww(unit_k), "true" if costs[3] is not None else "false")


def _rand(g, alphabet, n):
    return bytes(g.choice(alphabet, n)) if n else b""


def _edited(g, s, e, alphabet, keep_len):
    """s after e random substitutions, insertions, deletions and adjacent swaps; keep_len: an insertion is paid for by a deletion"""
    s = bytearray(s)
    for _ in range(e):
        kind = int(g.integers(0, 4))
        if kind == 0 and s:
            s[int(g.integers(len(s)))] = int(g.choice(alphabet))
        elif kind == 3 and len(s) > 1:
            p = int(g.integers(len(s) - 1))
            s[p], s[p + 1] = s[p + 1], s[p]
        elif kind == 1 or (keep_len and s):
            s.insert(int(g.integers(len(s) + 1)), int(g.choice(alphabet)))
            if keep_len:
                del s[int(g.integers(len(s)))]
        elif s:
            del s[int(g.integers(len(s)))]
    return bytes(s)


def _planted(g, s, e):
    """s with e symbols replaced by foreign ones: at distance exactly e from s under both cost families"""
    s = bytearray(s)
    for p in g.choice(len(s), min(e, len(s)), replace=False):
        s[int(p)] = int(g.choice(FOREIGN))
    return bytes(s)


def _batch(seed, nq, nt, k, form, alphabet=ACGT, lo=65, hi=256):
    """form: "csr" (query lengths lo .. hi, the first one hi) or a fixed length for both sides.  A quarter of the targets random, a
    quarter a query with 0 .. k + 2 edits, a quarter a query at distance exactly k, a quarter one at distance exactly k + 1"""
    g = Dg.rng(seed)
    kk = min(k, 40)
    fixed = form != "csr"
    qlens = [form] * nq if fixed else [hi, lo][:nq] + [int(x) for x in g.integers(lo, hi + 1, size=max(nq - 2, 0))]
    queries = [_rand(g, alphabet, n) for n in qlens]
    targets = []
    for i in range(nt):
        q = queries[int(g.integers(nq))]
        if i % 4 == 0:
            targets.append(_rand(g, alphabet, len(q) if fixed else max(0, len(q) + int(g.integers(-kk - 1, kk + 2)))))
        elif i % 4 == 1:
            targets.append(_edited(g, q, int(g.integers(0, kk + 3)), alphabet, fixed))
        else:
            targets.append(_planted(g, q, kk + (i % 4 == 3)))
    return queries, targets


def _side(B, strings, form):
    if form == "csr":
        return B.Strings.from_list(strings)
    return B.Strings.from_fixed(np.frombuffer(b"".join(strings), np.uint8).reshape(len(strings), form))


_join_memo = {}


def _dists(queries, targets, k, costs):
    """the oracle over EVERY pair -> (nq, nt) uint32, NONE where it answers None; computed once per distinct batch"""
    key = (tuple(queries), tuple(targets), k, costs)
    if key not in _join_memo:
        a = O.csr_from_list([q for q in queries for _ in targets])
        b = O.csr_from_list(list(targets) * len(queries))
        _join_memo[key] = O.levenshtein_k_batch(a, b, k, costs).reshape(len(queries), len(targets))
    return _join_memo[key]


def _join(queries, targets, k, costs, upper=False):
    """-> (sorted hits [(q, t, d)], nearest words, per-query counts)"""
    d = _dists(queries, targets, k, costs)
    hits, nearest, per_query = [], [], []
    for q in range(len(queries)):
        row = [(q, t, int(d[q, t])) for t in range(len(targets)) if d[q, t] != NONE and (not upper or t > q)]
        hits += row
        nearest.append(min((x << 32 | t) for _, t, x in row) if row else ALL_ONES)
        per_query.append(len(row))
    return hits, nearest, per_query


def _shows_something(queries, targets, k, costs):
    d = _dists(queries, targets, k, costs)
    assert int((d != NONE).sum()) >= 16, (len(queries), len(targets), k)
    if k != KMAX:
        inside = np.array([[abs(len(q) - len(t)) <= k for t in targets] for q in queries])
        assert int((d == k).sum()) >= 1, (len(queries), len(targets), k)
        assert int(((d == NONE) & inside).sum()) >= 16, (len(queries), len(targets), k)


def _got(B, torch, hits, count, nearest, per_query, cut=False):
    torch.cuda.synchronize()
    q, t, d = B.cross_to_arrays(hits, count, allow_cut=cut)
    words = None if nearest is None else [int(w) for w in nearest.cpu().numpy().view(np.uint64)]
    counts = None if per_query is None else [int(c) for c in per_query.cpu().numpy().view(np.uint32)]
    return list(zip(q.tolist(), t.tolist(), d.tolist())), int(count.item()), words, counts


def _check(B, torch, qs, ts, queries, targets, k, costs, upper=False):
    want = _join(queries, targets, k, costs, upper)
    out = B.levenshtein_cross_with_opts(qs, ts, k, costs, cap=max(len(queries) * len(targets), 1), nearest=True, per_query=True, upper=upper)
    got, n, near, counts = _got(B, torch, *out)
    where = (len(queries), len(targets), k, costs, upper)
    assert n == len(want[0]) and got == want[0], where
    assert near == want[1], where
    assert counts == want[2], where
    return want[0]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("form", ["csr", 150, 256])
def test_every_pair_equals_the_oracle(form, shape):
    torch, T, B = _mods()
    nq, nt = shape
    for k in KS:
        queries, targets = _batch(11000 + 7 * nq + k, nq, nt, k, form)
        qs, ts = _side(B, queries, form), _side(B, targets, form if form != "csr" and len({len(t) for t in targets}) == 1 else "csr")
        for costs in (O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS):
            if nq * nt >= 65:
                _shows_something(queries, targets, k, costs)
            _check(B, torch, qs, ts, queries, targets, k, costs)
            assert _kernel() == _win_name(k, costs), (k, costs)


def test_k_of_2_to_the_32_minus_1_hits_every_pair():
    torch, T, B = _mods()
    queries, targets = _batch(11100, 33, 65, KMAX, "csr")
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    for costs in (O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS):
        _shows_something(queries, targets, KMAX, costs)
        assert len(_check(B, torch, qs, ts, queries, targets, KMAX, costs)) == 33 * 65
        assert _kernel() == _win_name(KMAX, costs)


@pytest.mark.parametrize("lens", [(20, 64), (100, 160)])
def test_upper_on_a_set_against_itself(lens):
    torch, T, B = _mods()
    g = Dg.rng(11200 + lens[0])
    base = [_rand(g, ACGT, int(g.integers(lens[0], lens[1] + 1))) for _ in range(20)]
    reads = [_edited(g, base[int(g.integers(20))], int(g.integers(0, 5)), ACGT, False)[:lens[1]] for _ in range(130)]
    s = B.Strings.from_list(reads)
    for k, costs in ((3, O.LEVENSHTEIN_COSTS), (9, O.RDAMERAU_COSTS)):
        full = _check(B, torch, s, s, reads, reads, k, costs)
        upper = _check(B, torch, s, s, reads, reads, k, costs, upper=True)     # (all four outputs against the filtered join)
        assert _kernel().startswith("lev_cross_kernel<" if lens[1] <= 64 else "lev_cross_win_kernel<")
        assert upper == [(q, t, d) for q, t, d in full if q < t] and len(upper) >= 16
        diagonal = sum(1 for q, t, _ in full if q == t)
        assert diagonal == 130 and len(upper) == (len(full) - diagonal) // 2


@pytest.mark.parametrize("hi", [32, 64])
def test_short_queries_take_the_64_byte_body_with_both_new_outputs(hi):
    torch, T, B = _mods()
    for k in (1, 4):
        queries, targets = _batch(11300 + hi + k, 65, 130, k, "csr", LOWER, 1, hi)
        qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
        for costs in (O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS):
            _check(B, torch, qs, ts, queries, targets, k, costs)
            _check(B, torch, qs, ts, queries, targets, k, costs, upper=True)
            assert _kernel() == "lev_cross_kernel<%d, %s>" % (hi // 32, "true" if costs[3] is not None else "false")


def test_without_the_new_outputs_it_equals_levenshtein_cross():
    torch, T, B = _mods()
    queries, targets = _batch(11400, 65, 130, 4, "csr", ACGT, 1, 64)
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    for costs in (O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS, (3, 3, 0, None)):
        old = B.levenshtein_cross(qs, ts, 13, costs, cap=65 * 130, nearest=True)
        new = B.levenshtein_cross_with_opts(qs, ts, 13, costs, cap=65 * 130, nearest=True)
        assert new[3] is None
        a, b = _got(B, torch, *old, None), _got(B, torch, *new)
        assert a == b and a[1] >= 16, costs


def test_cap_cuts_the_records_not_the_count():
    torch, T, B = _mods()
    queries, targets = _batch(11500, 65, 130, 9, "csr")
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    want, want_near, want_counts = _join(queries, targets, 9, O.RDAMERAU_COSTS)
    assert len(want) >= 16
    cap = len(want) // 2
    out = B.levenshtein_cross_with_opts(qs, ts, 9, O.RDAMERAU_COSTS, cap=cap, nearest=True, per_query=True)
    got, n, near, counts = _got(B, torch, *out, cut=True)
    assert n == len(want)                                          # the count is unchanged
    assert len(got) == cap and len(set((q, t) for q, t, _ in got)) == cap   # no record twice
    assert set(got) <= set(want)                                   # every record is a true hit
    assert near == want_near and counts == want_counts             # neither depends on cap
    with pytest.raises(ValueError, match="larger cap"):
        B.cross_to_arrays(out[0], out[1])
    # cap = 0 with a NULL hits buffer: the count, the nearest words and the per-query counts alone
    nearest0 = torch.full((len(queries),), 5, dtype=torch.int64, device="cuda")
    per_query0 = torch.full((len(queries),), 5, dtype=torch.int32, device="cuda")
    count0 = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    import ctypes as C
    cc = T._n.EditCostsC(1, 1, 0, 1, 1)
    fn = T._n.lib().ta_levenshtein_cross_with_opts
    rc = fn(qs._ref(), qs.n, ts._ref(), ts.n, 9, C.byref(cc), 0, None, count0.data_ptr(), 0, nearest0.data_ptr(), per_query0.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(count0.item()) == len(want)
    assert [int(w) for w in nearest0.cpu().numpy().view(np.uint64)] == want_near
    assert per_query0.cpu().tolist() == want_counts
    # and without either per-query output
    rc = fn(qs._ref(), qs.n, ts._ref(), ts.n, 9, C.byref(cc), 0, None, count0.data_ptr(), 0, None, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and int(count0.item()) == len(want)


def test_multiples_of_the_unit_costs():
    torch, T, B = _mods()
    queries, targets = _batch(11600, 65, 130, 9, "csr")
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    for k in (18, 19):                                             # both run with k / g = 9 and report 2 d
        want = _check(B, torch, qs, ts, queries, targets, k, (2, 2, 0, 2))
        assert _kernel() == "lev_cross_win_kernel<3, true>"
        assert len(want) >= 16 and all(d % 2 == 0 for _, _, d in want) and any(d == 18 for _, _, d in want)
        assert [(q, t, d // 2) for q, t, d in want] == _join(queries, targets, 9, O.RDAMERAU_COSTS)[0]


def test_empty_sides():
    torch, T, B = _mods()
    some = B.Strings.from_list([b"ACGT" * 30, b"AC", b"TTT"])
    none = B.Strings.from_list([])
    for qs, ts in ((some, none), (none, some), (none, none)):
        for upper in (False, True):
            count = torch.full((1,), 9, dtype=torch.int64, device="cuda")
            nearest = torch.full((max(qs.n, 1),), 9, dtype=torch.int64, device="cuda")
            per_query = torch.full((max(qs.n, 1),), 9, dtype=torch.int32, device="cuda")
            B.levenshtein_cross_with_opts(qs, ts, 3, cap=4, count=count, nearest=nearest, per_query=per_query, upper=upper)
            torch.cuda.synchronize()
            assert int(count.item()) == 0
            assert (nearest[:qs.n] == -1).all() and (per_query[:qs.n] == 0).all()


def test_a_measured_query_longer_than_256_bytes_is_unsupported():
    torch, T, B = _mods()
    qs = B.Strings.from_list([b"A" * 10, b"C" * 257])
    qs.max_len = 0
    with pytest.raises(NotImplementedError, match="256 bytes"):
        B.levenshtein_cross_with_opts(qs, B.Strings.from_list([b"ACGT"]), 2)
    ok = B.Strings.from_list([b"A" * 10, b"C" * 256])
    ok.max_len = 0                                                 # measured: one synchronisation, then the window kernel
    hits, count, _, _ = B.levenshtein_cross_with_opts(ok, B.Strings.from_list([b"C" * 255]), 2)
    assert _got(B, torch, hits, count, None, None)[0] == [(1, 0, 1)] and _kernel() == "lev_cross_win_kernel<2, false>"


def test_streams_repeated_calls_and_graph_replay():
    torch, T, B = _mods()
    k, costs = 9, O.RDAMERAU_COSTS
    variants = [_batch(11800 + v, 65, 130, k, "csr") for v in range(3)]
    nq, nt, ql, tl = 65, 130, 256, 300
    qblob = torch.zeros(nq * ql + 16, dtype=torch.uint8, device="cuda")
    tblob = torch.zeros(nt * tl + 16, dtype=torch.uint8, device="cuda")
    qoff = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    toff = torch.zeros(nt + 1, dtype=torch.int64, device="cuda")

    def put(v):
        for strings, blob, off in ((variants[v][0], qblob, qoff), (variants[v][1], tblob, toff)):
            data = b"".join(strings)
            blob[:len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            off[1:] = torch.from_numpy(np.cumsum([len(s) for s in strings])).cuda()

    qs, ts = B.Strings(qblob, qoff, max_len=ql), B.Strings(tblob, toff, max_len=tl)   # CSR with the bounds given: no synchronisation
    cap = nq * nt
    want = lambda v: (lambda j: (j[0], len(j[0]), j[1], j[2]))(_join(*variants[v], k, costs))   # noqa: E731
    run = lambda **kw: B.levenshtein_cross_with_opts(qs, ts, k, costs, cap=cap, **kw)   # noqa: E731
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        put(0)
        out = run(nearest=True, per_query=True)                    # a stream of its own (and the run outside the capture)
        s.synchronize()
        assert _got(B, torch, *out) == want(0)
        with torch.cuda.stream(s2):                                # a second stream, buffers of its own, while the first goes on
            out2 = run(nearest=True, per_query=True)
        for _ in range(2):                                         # back to back into the same buffers
            run(hits=out[0], count=out[1], nearest=out[2], per_query=out[3])
        s.synchronize()
        s2.synchronize()
        assert _got(B, torch, *out) == want(0) and _got(B, torch, *out2) == want(0)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            run(hits=out[0], count=out[1], nearest=out[2], per_query=out[3])
        put(1)
        graph.replay()                                             # one replay, on other strings
        s.synchronize()
        assert _got(B, torch, *out) == want(1)


def test_python_helpers_equal_a_double_loop_of_single_calls():
    torch, T, B = _mods()
    queries, targets = _batch(11900, 12, 30, 8, "csr")
    for k, costs in ((8, T.LEVENSHTEIN_COSTS), (9, T.RDAMERAU_COSTS)):
        want, nearest = [], []
        for q, a in enumerate(queries):
            row = []
            for t, b in enumerate(targets):
                d = O.levenshtein_simd_k_with_opts(a, b, k, False, (costs.mismatch_cost, costs.gap_cost, costs.start_gap_cost, costs.transpose_cost))[0]
                if d is not None:
                    want.append((q, t, d))
                    row.append((d, t))
            nearest.append((min(row)[1], min(row)[0], len(row)) if row else None)
        assert T.levenshtein_cross_with_opts_many(queries, targets, k, costs) == want and len(want) > 0
        assert T.levenshtein_nearest_with_opts_many(queries, targets, k, costs) == nearest
        both = queries + targets
        assert T.levenshtein_cross_with_opts_many(both, both, k, costs, upper=True) == \
            [(q, t, d) for q, t, d in T.levenshtein_cross_with_opts_many(both, both, k, costs) if q < t]
    # more hits than the first call's room: one more call with room for the count
    many = [b"ACGT" * 20] * 40
    assert T.levenshtein_cross_with_opts_many(many, many, 0) == [(q, t, 0) for q in range(40) for t in range(40)]
    assert T.levenshtein_cross_with_opts_many([], many, 1) == [] and T.levenshtein_nearest_with_opts_many([b"AC" * 50], [], 1) == [None]
