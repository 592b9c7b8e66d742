"""gpu: every query against every target within k (ta_levenshtein_cross) against the oracle's levenshtein_simd_k_with_opts on EVERY pair
of every batch: the sorted hit list, the count and the nearest words; batch shapes on both sides of the wavefront and of the query tile,
strided and CSR sides, every alphabet, both cost families and their multiples, cap cutting, counting only, all pairs hitting, the exact
join, streams, repeated calls, graph capture, and the Python helpers."""
import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ALL_ONES = 0xFFFFFFFFFFFFFFFF
TILE = 16                                                          # CROSS_MIN_QTILE: the query tile of a small batch
SHAPES = ((1, 1), (1, 65), (63, 64), (65, 130), (2 * TILE + 1, 200))
QUERY_LENS = (0, 1, 2, 31, 32, 33, 63, 64)
TARGET_LENS = (0, 1, 31, 32, 33, 63, 64, 65, 100)
ALPHABETS = {
    "acgt": np.frombuffer(b"ACGT", np.uint8),
    "1..255": np.arange(1, 256, dtype=np.uint8),
    "nul": np.array([0], np.uint8),
    "nul+0c": np.array([0x00, 0x0C], np.uint8),
    "0..255": np.arange(0, 256, dtype=np.uint8),
}
LEV, RDAM = O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS


def _mods():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    return torch, T, B


def _kernel():
    import triple_accel_amd as T
    return T._n.lib().ta_last_kernel_name().decode()


def _rand(g, alphabet, n):
    return bytes(g.choice(alphabet, n)) if n else b""


def _lens(g, must, count, hi):
    out = [x for x in must if x <= hi][:count]
    out += [int(x) for x in g.integers(0, hi + 1, size=count - len(out))]
    g.shuffle(out)
    return out


def _batch(seed, nq, nt, alphabet, qmax=64):
    """queries of the lengths that matter (up to qmax); half of the targets random, half a query with 0-4 edits (swaps included)"""
    g = Dg.rng(seed)
    queries = [_rand(g, alphabet, n) for n in _lens(g, QUERY_LENS, nq, qmax)]
    targets = [_rand(g, alphabet, n) for n in _lens(g, TARGET_LENS, nt, 100)]
    for i in range(0, nt, 2):
        targets[i] = Dg.mutate(g, queries[int(g.integers(nq))], int(g.integers(0, 5)), swaps=True)
    return queries, targets


_oracle_memo = {}


def _oracle(queries, targets, k, costs):
    """the oracle over EVERY pair -> (sorted hits [(q, t, d)], nearest words); computed once per distinct batch and left unchanged"""
    key = (tuple(queries), tuple(targets), k, tuple(costs))
    if key not in _oracle_memo:
        nq, nt = len(queries), len(targets)
        a = O.csr_from_list([q for q in queries for _ in range(nt)])
        b = O.csr_from_list([t for _ in range(nq) for t in targets])
        d = O.levenshtein_k_batch(a, b, k, costs).reshape(nq, nt) if nq * nt else np.zeros((nq, nt), np.uint32)
        hits = [(q, t, int(d[q, t])) for q in range(nq) for t in range(nt) if d[q, t] != NONE]
        nearest = []
        for q in range(nq):
            row = [(int(d[q, t]), t) for t in range(nt) if d[q, t] != NONE]
            nearest.append((min(row)[0] << 32 | min(row)[1]) if row else ALL_ONES)
        _oracle_memo[key] = (hits, nearest)
    return _oracle_memo[key]


def _got(B, torch, hits, count, nearest, cut=False):
    torch.cuda.synchronize()
    q, t, d = B.cross_to_arrays(hits, count, allow_cut=cut)
    words = None if nearest is None else [int(w) for w in nearest.cpu().numpy().view(np.uint64)]
    return list(zip(q.tolist(), t.tolist(), d.tolist())), int(count.item()), words


def _check(B, torch, qs, ts, queries, targets, k, costs):
    want, want_near = _oracle(queries, targets, k, costs)
    hits, count, nearest = B.levenshtein_cross(qs, ts, k, costs, cap=len(queries) * len(targets), nearest=True)
    got, n, near = _got(B, torch, hits, count, nearest)
    assert n == len(want) and got == want, (len(queries), len(targets), k, costs)
    assert near == want_near, (len(queries), len(targets), k, costs)
    return want


@pytest.mark.parametrize("costs", [LEV, RDAM, (3, 3, 0, None), (2, 2, 0, 2)])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_pair_equals_the_oracle(shape, costs):
    torch, T, B = _mods()
    nq, nt = shape
    g = costs[0]
    total = 0
    for qmax in (32, 64):                                          # one and two table words per row
        queries, targets = _batch(7000 + nq + qmax, nq, nt, ALPHABETS["acgt"], qmax)
        qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
        for k in (0, g, 3 * g + 1, 40 * g):
            total += len(_check(B, torch, qs, ts, queries, targets, k, costs))
            longest = max(len(q) for q in queries)
            assert _kernel() == "lev_cross_kernel<%d, %s>" % (1 if longest <= 32 else 2, "true" if costs[3] is not None else "false")
    assert total > 0 or nq * nt == 1


@pytest.mark.parametrize("name", list(ALPHABETS))
def test_every_alphabet(name):
    torch, T, B = _mods()
    queries, targets = _batch(7100 + len(name), 65, 130, ALPHABETS[name])
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    for costs in (LEV, RDAM):
        for k in (1, 4, 33):
            _check(B, torch, qs, ts, queries, targets, k, costs)


@pytest.mark.parametrize("qform", ["strided", "csr", "csr_unmeasured"])
@pytest.mark.parametrize("tform", ["strided", "csr", "csr_unmeasured"])
def test_strided_and_csr_sides(qform, tform):
    torch, T, B = _mods()
    g = Dg.rng(7200)
    nq, nt, ql, tl = 63, 64, 21, 22
    queries = [_rand(g, ALPHABETS["acgt"], ql) for _ in range(nq)]
    # target i: query i % nq with at most one edit (20..22 bytes), padded to tl = 22: within 3 of that query
    targets = [(Dg.mutate(g, queries[i % nq], 1, swaps=True) + _rand(g, ALPHABETS["acgt"], tl))[:tl] for i in range(nt)]

    def side(strings, form):
        if form == "strided":
            return B.Strings.from_fixed(np.frombuffer(b"".join(strings), np.uint8).reshape(len(strings), -1))
        s = B.Strings.from_list(strings)
        if form == "csr_unmeasured":
            s.max_len = 0                                          # "let the library measure it": one synchronisation
        return s

    qs, ts = side(queries, qform), side(targets, tform)
    for costs in (LEV, RDAM):
        want = _check(B, torch, qs, ts, queries, targets, 4, costs)
        assert len(want) >= nt


def test_nearest_with_ties_and_queries_without_a_hit():
    torch, T, B = _mods()
    queries = [b"ACGTACGTACGT", b"TTTTTTTTTTTT", b"GGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGG", b"", b"ACGTACGTACGA"]
    targets = [b"CCCCCCCCCCCC", b"ACGTACGTACGA", b"ACGTACGTACGC", b"ACGTACGTACGT", b"ACGTACGTACGA", b"ACGTACGTACGT", b"A", b"C"] * 9
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    want, near = _oracle(queries, targets, 1, LEV)
    assert near[0] == (0 << 32 | 3) and near[1] == ALL_ONES and near[2] == ALL_ONES and near[3] == (1 << 32 | 6) and near[4] == (0 << 32 | 1)
    _check(B, torch, qs, ts, queries, targets, 1, LEV)
    _check(B, torch, qs, ts, queries, targets, 1, RDAM)
    _check(B, torch, qs, ts, queries, targets, 0, LEV)


def test_cap_cuts_the_records_not_the_count():
    torch, T, B = _mods()
    queries, targets = _batch(7300, 65, 130, ALPHABETS["acgt"])
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    want, want_near = _oracle(queries, targets, 12, LEV)
    assert len(want) >= 64
    cap = len(want) // 2
    hits, count, nearest = B.levenshtein_cross(qs, ts, 12, LEV, cap=cap, nearest=True)
    got, n, near = _got(B, torch, hits, count, nearest, cut=True)
    assert n == len(want)                                          # the count is unchanged
    assert len(got) == cap and len(set((q, t) for q, t, _ in got)) == cap   # no record twice
    assert set(got) <= set(want)                                   # every record is an oracle hit
    assert near == want_near                                       # nearest does not depend on cap
    with pytest.raises(ValueError, match="larger cap"):
        B.cross_to_arrays(hits, count)
    # cap = 0 with a NULL hits buffer: the count and the nearest words alone
    nearest0 = torch.full((len(queries),), 5, dtype=torch.int64, device="cuda")
    count0 = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    rc = T._n.lib().ta_levenshtein_cross(qs._ref(), qs.n, ts._ref(), ts.n, 12, T._n.EditCostsC(1, 1, 0, 0, 0), None, count0.data_ptr(), 0,
                                         nearest0.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(count0.item()) == len(want)
    assert [int(w) for w in nearest0.cpu().numpy().view(np.uint64)] == want_near


def test_every_pair_hits_and_the_exact_join():
    torch, T, B = _mods()
    queries, targets = _batch(7400, 65, 130, ALPHABETS["1..255"])
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    for k in (164, NONE):                                          # 64 + 100: no pair is further apart
        want = _check(B, torch, qs, ts, queries, targets, k, RDAM)
        assert len(want) == 65 * 130
    # k = 0: the exact-match join, duplicates on both sides
    g = Dg.rng(7401)
    words = [_rand(g, ALPHABETS["acgt"], int(g.integers(0, 9))) for _ in range(12)] + [b"", b""]
    queries = [words[int(g.integers(len(words)))] for _ in range(70)]
    targets = [words[int(g.integers(len(words)))] for _ in range(150)]
    want = _check(B, torch, B.Strings.from_list(queries), B.Strings.from_list(targets), queries, targets, 0, LEV)
    assert want == [(q, t, 0) for q in range(70) for t in range(150) if queries[q] == targets[t]] and len(want) > 150


def test_empty_sides():
    torch, T, B = _mods()
    some = B.Strings.from_list([b"ACGT", b"AC", b"TTT"])
    none = B.Strings.from_list([])
    for qs, ts in ((some, none), (none, some), (none, none)):
        count = torch.full((1,), 9, dtype=torch.int64, device="cuda")
        nearest = torch.full((max(qs.n, 1),), 9, dtype=torch.int64, device="cuda")
        B.levenshtein_cross(qs, ts, 3, LEV, cap=4, count=count, nearest=nearest)
        torch.cuda.synchronize()
        assert int(count.item()) == 0
        assert (nearest[:qs.n] == -1).all()


def test_a_measured_query_longer_than_64_bytes_is_unsupported():
    torch, T, B = _mods()
    qs = B.Strings.from_list([b"A" * 10, b"C" * 65])
    qs.max_len = 0
    with pytest.raises(NotImplementedError, match="64 bytes"):
        B.levenshtein_cross(qs, B.Strings.from_list([b"ACGT"]), 2)


def test_streams_repeated_calls_and_graph_replay():
    torch, T, B = _mods()
    variants = [_batch(7500 + v, 65, 130, ALPHABETS["acgt"], 32) for v in range(3)]
    nq, nt, ql, tl = 65, 130, 32, 100
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
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        put(0)
        hits, count, nearest = B.levenshtein_cross(qs, ts, 5, RDAM, cap=cap, nearest=True)    # a stream of its own
        s.synchronize()
        want, want_near = _oracle(*variants[0], 5, RDAM)
        assert _got(B, torch, hits, count, nearest) == (want, len(want), want_near)
        for _ in range(2):                                         # back to back into the same buffers
            B.levenshtein_cross(qs, ts, 5, RDAM, cap=cap, hits=hits, count=count, nearest=nearest)
        s.synchronize()
        assert _got(B, torch, hits, count, nearest) == (want, len(want), want_near)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            B.levenshtein_cross(qs, ts, 5, RDAM, cap=cap, hits=hits, count=count, nearest=nearest)
        for v in (1, 2):
            put(v)
            graph.replay()
            s.synchronize()
            want, want_near = _oracle(*variants[v], 5, RDAM)
            assert _got(B, torch, hits, count, nearest) == (want, len(want), want_near), v     # the counter read after each replay


def test_python_helpers_equal_a_double_loop_of_single_calls():
    torch, T, B = _mods()
    queries, targets = _batch(7600, 20, 30, ALPHABETS["acgt"])
    for costs, tcosts in ((LEV, T.LEVENSHTEIN_COSTS), (RDAM, T.RDAMERAU_COSTS)):
        for k in (2, 30):
            want, nearest = [], []
            for q, a in enumerate(queries):
                row = []
                for t, b in enumerate(targets):
                    d = T.levenshtein_simd_k_with_opts(a, b, k, False, tcosts)
                    d = d[0] if isinstance(d, tuple) else d
                    if d is not None:
                        want.append((q, t, d))
                        row.append((d, t))
                nearest.append((min(row)[1], min(row)[0]) if row else None)
            assert T.levenshtein_cross_many(queries, targets, k, tcosts) == want
            assert T.levenshtein_nearest_many(queries, targets, k, tcosts) == nearest
    # more hits than the first call's room: one more call with room for the count
    many = [b"ACGT"] * 40
    assert T.levenshtein_cross_many(many, many, 0) == [(q, t, 0) for q in range(40) for t in range(40)]
    assert T.levenshtein_cross_many([], many, 1) == [] and T.levenshtein_nearest_many([b"AC"], [], 1) == [None]
