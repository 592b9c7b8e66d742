"""gpu: every query of 32-bit tokens against every target within k (ta_levenshtein_cross_tokens) against the join over EVERY pair, answered
by the C oracle on byte codes of the same pairs (cross_tokens_cases.dists): the sorted hit list, the count, the nearest words and the
per-query counts.  Target counts on both sides of the wavefront and workgroup edges, query counts on both sides of the query-tile
edges (and the tile forced to 1 and to 16), query lengths 0 .. 64 so that both kernels launch, targets of 0 .. 100 tokens, k = 0, 1, 3
and 2^32 - 1, both cost families and a multiple at an odd k; the upper triangle; cap cutting and counting only; empty sides; the
vocabularies and the hash-collision queries of the CPU suite through the real kernel; byte-valued tokens against the byte entry; the
limits; graph capture; the Python helpers.

One pool of 33 queries and 257 targets serves every shape: a shape takes a prefix of each side, and the oracle runs once per (k, costs)."""
import ctypes as C
import functools

import numpy as np
import pytest

import cross_tokens_cases as X
import datagen as Dg
import oracle_lib as O

pytestmark = pytest.mark.gpu

NONE, ALL_ONES, KMAX = X.NONE, X.ALL_ONES, X.KMAX
NTS = (1, 63, 64, 65, 255, 256, 257)
NQS = (1, 15, 16, 17, 33)
KS = (0, 1, 3, KMAX)
DOUBLE = (2, 2, 0, None)


def _mods():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    return torch, T, B


def _kernel():
    import triple_accel_amd as T
    return T._n.lib().ta_last_kernel_name().decode()


def _name(nw, costs):
    return "lev_cross_tok_kernel<%d, %s>" % (nw, "true" if costs[3] is not None else "false")


@functools.lru_cache(maxsize=None)
def _pool(longest):
    """33 queries of 0 .. `longest` tokens (the first one `longest`: every prefix takes the same kernel) and 257 targets of 0 .. 100: a
    third random, the others a query after 0 .. 5 edits.  200 distinct values from all over the 32 bits."""
    g = Dg.rng(12000 + longest)
    voc = X.vocab("32k")[::160][:200]
    qlens = [longest, 0, 1, longest - 1] + [int(x) for x in g.integers(0, longest + 1, size=29)]
    queries = [X.rand_seq(g, voc[:24], n) for n in qlens]
    targets = []
    for i in range(257):
        if i % 3 == 0:
            targets.append(X.rand_seq(g, voc, int(g.integers(0, 101))))
        else:
            targets.append(X.edited(g, queries[int(g.integers(len(queries)))], int(g.integers(0, 6)), voc[:24]))
    targets[5], targets[6], targets[7] = (), X.rand_seq(g, voc, 100), X.rand_seq(g, voc, 99)
    return queries, targets


def _join(d, upper=False):
    """(nq, nt) distances -> (sorted hits [(q, t, d)], nearest words, per-query counts)"""
    hits, nearest, per_query = [], [], []
    for q in range(d.shape[0]):
        row = [(q, int(t), int(d[q, t])) for t in np.flatnonzero(d[q] != NONE) if not upper or t > q]
        hits += row
        nearest.append(min((x << 32 | t) for _, t, x in row) if row else ALL_ONES)
        per_query.append(len(row))
    return hits, nearest, per_query


def _got(B, torch, hits, count, nearest, per_query, cut=False):
    torch.cuda.synchronize()
    q, t, d = B.cross_to_arrays(hits, count, allow_cut=cut)
    words = None if nearest is None else [int(w) for w in nearest.cpu().numpy().view(np.uint64)]
    counts = None if per_query is None else [int(c) for c in per_query.cpu().numpy().view(np.uint32)]
    return list(zip(q.tolist(), t.tolist(), d.tolist())), int(count.item()), words, counts


def _check(B, torch, qs, ts, d, k, costs, upper=False):
    want = _join(d, upper)
    out = B.levenshtein_cross_tokens(qs, ts, k, costs, cap=max(d.size, 1), nearest=True, per_query=True, upper=upper)
    got, n, near, counts = _got(B, torch, *out)
    where = (d.shape, k, costs, upper)
    assert n == len(want[0]) and got == want[0], where
    assert near == want[1], where
    assert counts == want[2], where
    return want[0]


def test_the_pool_shows_something():
    queries, targets = _pool(64)
    assert {len(q) for q in queries} >= {0, 1, 63, 64} and max(map(len, queries)) == 64
    assert {len(t) for t in targets} >= {0, 99, 100}
    for k in (0, 1, 3):
        d = X.dists(queries, targets, k, O.LEVENSHTEIN_COSTS)
        inside = np.array([[abs(len(q) - len(t)) <= k for t in targets] for q in queries])
        assert int((d == k).sum()) >= 8 and int(((d == NONE) & inside).sum()) >= 16, k
    assert (X.dists(queries, targets, 3, O.RDAMERAU_COSTS) != X.dists(queries, targets, 3, O.LEVENSHTEIN_COSTS)).any()   # a transposition counts


@pytest.mark.parametrize("nt", NTS)
def test_every_pair_equals_the_oracle(nt):
    torch, T, B = _mods()
    queries, targets = _pool(64)
    ts = B.Tokens.from_list(targets[:nt])
    for nq in NQS:
        qs = B.Tokens.from_list(queries[:nq])
        for k in KS:
            for costs in X.COSTS:
                _check(B, torch, qs, ts, X.dists(queries, targets, k, costs)[:nq, :nt], k, costs)
                assert _kernel() == _name(2, costs), (nq, nt, k)
        _check(B, torch, qs, ts, X.dists(queries, targets, 7, DOUBLE)[:nq, :nt], 7, DOUBLE)     # runs with k / g = 3, reports 2 d


def test_multiples_of_the_unit_costs_report_g_times_d():
    torch, T, B = _mods()
    queries, targets = _pool(64)
    qs, ts = B.Tokens.from_list(queries), B.Tokens.from_list(targets)
    for k in (6, 7):
        want = _check(B, torch, qs, ts, X.dists(queries, targets, k, DOUBLE), k, DOUBLE)
        assert len(want) >= 16 and all(d % 2 == 0 for _, _, d in want) and any(d == 6 for _, _, d in want)
        assert [(q, t, d // 2) for q, t, d in want] == _join(X.dists(queries, targets, 3, O.LEVENSHTEIN_COSTS))[0]
    want = _check(B, torch, qs, ts, X.dists(queries, targets, 9, (3, 3, 0, 3)), 9, (3, 3, 0, 3))
    assert _kernel() == "lev_cross_tok_kernel<2, true>" and any(d == 9 for _, _, d in want)


@pytest.mark.parametrize("shape", [(17, 65), (33, 257)])
def test_queries_of_up_to_32_tokens_take_the_one_word_kernel(shape):
    torch, T, B = _mods()
    nq, nt = shape
    queries, targets = _pool(32)
    qs, ts = B.Tokens.from_list(queries[:nq]), B.Tokens.from_list(targets[:nt])
    for k in KS:
        for costs in X.COSTS:
            _check(B, torch, qs, ts, X.dists(queries, targets, k, costs)[:nq, :nt], k, costs)
            assert _kernel() == _name(1, costs), (k, costs)
    _check(B, torch, qs, ts, X.dists(queries, targets, 3, O.RDAMERAU_COSTS)[:nq, :nt], 3, O.RDAMERAU_COSTS, upper=True)


@pytest.mark.parametrize("tile", [1, 16])
def test_a_forced_query_tile(tile, monkeypatch):
    torch, T, B = _mods()
    queries, targets = _pool(64)
    monkeypatch.setenv("TA_CROSS_QTILE", str(tile))                 # (read at every call under TA_TUNING)
    for nq, nt in ((33, 257), (17, 65), (16, 64)):
        qs, ts = B.Tokens.from_list(queries[:nq]), B.Tokens.from_list(targets[:nt])
        for k, costs in ((1, O.LEVENSHTEIN_COSTS), (3, O.RDAMERAU_COSTS)):
            _check(B, torch, qs, ts, X.dists(queries, targets, k, costs)[:nq, :nt], k, costs)
            _check(B, torch, qs, ts, X.dists(queries, targets, k, costs)[:nq, :nt], k, costs, upper=True)


def test_upper_on_a_set_against_itself():
    torch, T, B = _mods()
    g = Dg.rng(12200)
    voc = X.vocab("32k")[:12]
    base = [X.rand_seq(g, voc, int(g.integers(20, 65))) for _ in range(20)]
    reads = [X.edited(g, base[int(g.integers(20))], int(g.integers(0, 5)), voc)[:64] for _ in range(130)]
    s = B.Tokens.from_list(reads)
    for k, costs in ((3, O.LEVENSHTEIN_COSTS), (4, O.RDAMERAU_COSTS)):
        d = X.dists(reads, reads, k, costs)
        full = _check(B, torch, s, s, d, k, costs)
        upper = _check(B, torch, s, s, d, k, costs, upper=True)      # (all four outputs against the filtered join)
        assert upper == [(q, t, x) for q, t, x in full if q < t] and len(upper) >= 16
        diagonal = sum(1 for q, t, _ in full if q == t)
        assert diagonal == 130 and len(upper) == (len(full) - diagonal) // 2


def test_cap_cuts_the_records_not_the_count():
    torch, T, B = _mods()
    queries, targets = _pool(64)
    qs, ts = B.Tokens.from_list(queries), B.Tokens.from_list(targets)
    want, want_near, want_counts = _join(X.dists(queries, targets, 3, O.RDAMERAU_COSTS))
    assert len(want) >= 16
    cap = len(want) // 2
    out = B.levenshtein_cross_tokens(qs, ts, 3, O.RDAMERAU_COSTS, cap=cap, nearest=True, per_query=True)
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
    cc = T._n.EditCostsC(1, 1, 0, 1, 1)
    fn = T._n.lib().ta_levenshtein_cross_tokens
    rc = fn(qs._ref(), qs.n, ts._ref(), ts.n, 3, C.byref(cc), 0, None, count0.data_ptr(), 0, nearest0.data_ptr(), per_query0.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(count0.item()) == len(want)
    assert [int(w) for w in nearest0.cpu().numpy().view(np.uint64)] == want_near
    assert per_query0.cpu().tolist() == want_counts
    rc = fn(qs._ref(), qs.n, ts._ref(), ts.n, 3, C.byref(cc), 0, None, count0.data_ptr(), 0, None, None, None)   # without either per-query output
    torch.cuda.synchronize()
    assert rc == 0 and int(count0.item()) == len(want)
    hits, count, nearest, per_query = B.levenshtein_cross_tokens(qs, ts, 3, O.RDAMERAU_COSTS, cap=0, hits=None)
    torch.cuda.synchronize()
    assert int(count.item()) == len(want) and nearest is None and per_query is None


def test_empty_sides():
    torch, T, B = _mods()
    some = B.Tokens.from_list([(1, 2, 3) * 10, (7, 8), (9,)])
    none = B.Tokens.from_list([])
    for qs, ts in ((some, none), (none, some), (none, none)):
        for upper in (False, True):
            count = torch.full((1,), 9, dtype=torch.int64, device="cuda")
            nearest = torch.full((max(qs.n, 1),), 9, dtype=torch.int64, device="cuda")
            per_query = torch.full((max(qs.n, 1),), 9, dtype=torch.int32, device="cuda")
            B.levenshtein_cross_tokens(qs, ts, 3, cap=4, count=count, nearest=nearest, per_query=per_query, upper=upper)
            torch.cuda.synchronize()
            assert int(count.item()) == 0
            assert (nearest[:qs.n] == -1).all() and (per_query[:qs.n] == 0).all()


@pytest.mark.parametrize("name", X.VOCABS)
def test_the_vocabularies_of_the_cpu_suite(name):
    torch, T, B = _mods()
    g = Dg.rng(12300 + len(name))
    voc = X.vocab(name)
    queries = [X.rand_seq(g, voc, n) for n in (64, 33, 32, 1, 0, 17, 40, 63)]
    targets = [X.edited(g, queries[i % 8], i % 5, voc) for i in range(50)] + [X.rand_seq(g, voc, int(g.integers(0, 101))) for _ in range(20)]
    qs, ts = B.Tokens.from_list(queries), B.Tokens.from_list(targets)
    for k, costs in ((0, O.LEVENSHTEIN_COSTS), (2, O.RDAMERAU_COSTS), (KMAX, O.LEVENSHTEIN_COSTS)):
        want = _check(B, torch, qs, ts, X.dists(queries, targets, k, costs), k, costs)
        assert len(want) >= 8


def test_queries_that_collide_in_the_table():
    """the four collision cases of tests/test_cross_tokens_cpu.py, built with the body's own home-slot function, through the real kernel:
    each query against its own targets, then all of them against all targets in one call"""
    torch, T, B = _mods()
    a, b, d4 = X.case_longest_chain(), X.case_two_on_one_slot(), X.case_duplicates_in_the_second_word()
    cq, ct, planted = X.case_absent_items_on_taken_slots()
    assert len(set(int(h) for h in X.homes(a[0]))) == 1 and len(set(a[0])) == 64
    assert all(X.homes([t[i]])[0] == X.homes([cq[i]])[0] and t[i] not in cq for t in ct for i in range(len(cq)) if t[i] != cq[i])
    for query, targets in (a, b, (cq, ct), d4):
        qs, ts = B.Tokens.from_list([query]), B.Tokens.from_list(targets)
        for k in (0, 1, 3, 64):
            for costs in X.COSTS:
                _check(B, torch, qs, ts, X.dists([query], targets, k, costs), k, costs)
    hits, count, _, _ = B.levenshtein_cross_tokens(B.Tokens.from_list([cq]), B.Tokens.from_list(ct), len(cq))
    assert [x for _, _, x in _got(B, torch, hits, count, None, None)[0]] == planted    # (without the key compare: 0 everywhere)
    queries = [a[0], b[0], cq, d4[0]]
    targets = a[1] + b[1] + ct + d4[1]
    qs, ts = B.Tokens.from_list(queries), B.Tokens.from_list(targets)
    for k, costs in ((2, O.LEVENSHTEIN_COSTS), (5, O.RDAMERAU_COSTS)):
        _check(B, torch, qs, ts, X.dists(queries, targets, k, costs), k, costs)


def test_byte_valued_tokens_give_the_byte_entrys_hit_set():
    torch, T, B = _mods()
    g = Dg.rng(12400)
    voc = list(range(256))
    queries = [X.rand_seq(g, voc[:8], int(g.integers(0, 65))) for _ in range(33)]
    targets = [X.edited(g, queries[int(g.integers(33))], int(g.integers(0, 5)), voc[:8]) for _ in range(100)] + \
              [X.rand_seq(g, voc, int(g.integers(0, 101))) for _ in range(30)]
    qt, tt = B.Tokens.from_list(queries), B.Tokens.from_list(targets)
    qb, tb = B.Strings.from_list([bytes(q) for q in queries]), B.Strings.from_list([bytes(t) for t in targets])
    for k, costs in ((2, O.LEVENSHTEIN_COSTS), (3, O.RDAMERAU_COSTS), (5, (2, 2, 0, 2))):
        for upper in (False, True):
            new = B.levenshtein_cross_tokens(qt, tt, k, costs, cap=33 * 130, nearest=True, per_query=True, upper=upper)
            old = B.levenshtein_cross_with_opts(qb, tb, k, costs, cap=33 * 130, nearest=True, per_query=True, upper=upper)
            a, b = _got(B, torch, *new), _got(B, torch, *old)
            assert a == b and (a[1] >= 16 or upper), (k, costs, upper)


def test_the_limits():
    torch, T, B = _mods()
    one = B.Tokens.from_list([(1, 2, 3)])
    ok = B.Tokens.from_fixed(np.arange(2 * 64, dtype=np.int64).reshape(2, 64))        # 64 tokens work ...
    hits, count, _, _ = B.levenshtein_cross_tokens(ok, B.Tokens.from_list([tuple(range(64, 127))]), 2)
    assert _got(B, torch, hits, count, None, None)[0] == [(1, 0, 1)] and _kernel() == "lev_cross_tok_kernel<2, false>"
    with pytest.raises(NotImplementedError, match="64 tokens"):                      # ... 65 do not: strided,
        B.levenshtein_cross_tokens(B.Tokens.from_fixed(np.zeros((2, 65), dtype=np.int64)), one, 2)
    with pytest.raises(NotImplementedError, match="64 tokens"):                      # CSR with the bound given,
        B.levenshtein_cross_tokens(B.Tokens.from_list([(5,) * 10, (6,) * 65]), one, 2)
    measured = B.Tokens.from_list([(5,) * 10, (6,) * 65])
    measured.max_len = 0
    count = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    with pytest.raises(NotImplementedError, match="64 tokens"):                      # and CSR measured by the library -- before any output
        B.levenshtein_cross_tokens(measured, one, 2, count=count)
    torch.cuda.synchronize()
    assert int(count.item()) == 9
    fine = B.Tokens.from_list([(5,) * 10, (6,) * 64])
    fine.max_len = 0                                               # measured: one synchronisation, then the two-word kernel
    hits, count, _, _ = B.levenshtein_cross_tokens(fine, B.Tokens.from_list([(6,) * 63]), 2)
    assert _got(B, torch, hits, count, None, None)[0] == [(1, 0, 1)] and _kernel() == "lev_cross_tok_kernel<2, false>"
    for costs in ((2, 1, 0, None), (1, 1, 1, None), (2, 2, 0, 3)):                   # weighted costs raise
        with pytest.raises(NotImplementedError, match="unit-cost"):
            B.levenshtein_cross_tokens(one, one, 2, costs)
    with pytest.raises(AssertionError):                                              # invalid costs: EditCosts::new's panic
        B.levenshtein_cross_tokens(one, one, 2, (1, 0, 0, None))


def test_graph_capture_with_every_bound_given():
    torch, T, B = _mods()
    queries, targets = _pool(64)
    nq, nt, k, costs = 33, 130, 3, O.RDAMERAU_COSTS
    qs = B.Tokens.from_list(queries[:nq])                          # (from_list gives max_len: no synchronisation in the call)
    ts = B.Tokens.from_list(targets[:nt])
    d = X.dists(queries, targets, k, costs)[:nq, :nt]
    want = (lambda j: (j[0], len(j[0]), j[1], j[2]))(_join(d))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = B.levenshtein_cross_tokens(qs, ts, k, costs, cap=nq * nt, nearest=True, per_query=True)   # eager (and the warm-up)
        s.synchronize()
        assert _got(B, torch, *out) == want
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):                    # one call, one branch
            B.levenshtein_cross_tokens(qs, ts, k, costs, cap=nq * nt, hits=out[0], count=out[1], nearest=out[2], per_query=out[3])
        for _ in range(2):
            for t in out:
                t.fill_(-3)
            graph.replay()
            s.synchronize()
            assert _got(B, torch, *out) == want


def test_python_helpers_equal_the_join():
    torch, T, B = _mods()
    queries, targets = _pool(64)
    queries, targets = [list(q) for q in queries[:12]], [list(t) for t in targets[:40]]
    for k, costs, tup in ((3, T.LEVENSHTEIN_COSTS, O.LEVENSHTEIN_COSTS), (4, T.RDAMERAU_COSTS, O.RDAMERAU_COSTS)):
        hits, nearest, per_query = _join(X.dists(queries, targets, k, tup))
        assert T.levenshtein_cross_tokens_many(queries, targets, k, costs) == hits and len(hits) > 0
        want = [None if w == ALL_ONES else (w & 0xFFFFFFFF, w >> 32, c) for w, c in zip(nearest, per_query)]
        assert T.levenshtein_nearest_tokens_many(queries, targets, k, costs) == want
        both = queries + [t for t in targets if len(t) <= 64]        # (a set against itself: every sequence is a query too)
        assert len(both) >= 30
        assert T.levenshtein_cross_tokens_many(both, both, k, costs, upper=True) == \
            [(q, t, d) for q, t, d in T.levenshtein_cross_tokens_many(both, both, k, costs) if q < t]
    # int32 tensors carry the u32 bit pattern; int64 tensors the values
    as32 = lambda s: torch.tensor(np.array(s, dtype=np.uint32).view(np.int32))     # noqa: E731
    as64 = lambda s: torch.tensor(np.array(s, dtype=np.int64))                     # noqa: E731
    hits = _join(X.dists(queries, targets, 3, O.LEVENSHTEIN_COSTS))[0]
    assert T.levenshtein_cross_tokens_many([as32(q) for q in queries], [as64(t) for t in targets], 3) == hits
    # more hits than the first call's room: one more call with room for the count
    many = [[7, 8, 9, 10] * 5] * 40
    assert T.levenshtein_cross_tokens_many(many, many, 0) == [(q, t, 0) for q in range(40) for t in range(40)]
    assert T.levenshtein_cross_tokens_many([], many, 1) == [] and T.levenshtein_nearest_tokens_many([[1, 2] * 20], [], 1) == [None]
