"""gpu: every query against every target within k mismatches (ta_hamming_cross) against a numpy join over EVERY pair of every batch
(equal length, count the differing bytes): the sorted hit list, the count, the nearest words and the per-query counts; batch shapes on
both sides of the lane, wavefront, workgroup, staging-chunk and query-tile edges at every register width, strided and CSR sides, six
alphabets, duplicates and ties, cap cutting, counting only, all pairs hitting, the upper triangle of a set against itself, empty sides,
streams, repeated calls, graph capture, and the Python helpers."""
import numpy as np
import pytest

import datagen as Dg

pytestmark = pytest.mark.gpu

ALL_ONES = 0xFFFFFFFFFFFFFFFF
ALPHABETS = {
    "acgt": np.frombuffer(b"ACGT", np.uint8),
    "lower": np.arange(97, 123, dtype=np.uint8),
    "0..255": np.arange(0, 256, dtype=np.uint8),
    "nul": np.array([0x00], np.uint8),
    "nul+0c": np.array([0x00, 0x0C], np.uint8),
    "0c+0d": np.array([0x0C, 0x0D], np.uint8),
}
LENS = {4: (0, 1, 3, 4, 5, 15, 16), 8: (0, 1, 3, 4, 5, 15, 16, 17, 31, 32), 16: (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64)}
NTS = (1, 63, 64, 65, 257)                                         # the lane, wavefront and workgroup edges


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


def _substitute(g, s, e, alphabet):
    s = bytearray(s)
    for p in (g.choice(len(s), min(e, len(s)), replace=False) if s else []):
        others = [int(c) for c in alphabet if int(c) != s[p]] or [s[p] ^ 0x0C, s[p] ^ 0xFF]
        s[p] = others[int(g.integers(len(others)))]
    return bytes(s)


def _batch(seed, nq, nt, alphabet, lens):
    """queries of the lengths that matter; a third of the targets random (lengths of the set, plus 65 and 100: never hits), the others a
    query with 0-3 substitutions -- most pairs differ in length"""
    g = Dg.rng(seed)
    qlens = [int(n) for n in g.permutation(lens)[:nq]] + [int(lens[int(i)]) for i in g.integers(len(lens), size=max(nq - len(lens), 0))]
    g.shuffle(qlens)
    queries = [_rand(g, alphabet, n) for n in qlens]
    tlens = tuple(lens) + (65, 100)
    targets = []
    for i in range(nt):
        if i % 3 == 0:
            targets.append(_rand(g, alphabet, tlens[int(g.integers(len(tlens)))]))
        else:
            targets.append(_substitute(g, queries[int(g.integers(nq))], int(g.integers(0, 4)), alphabet))
    return queries, targets


_join_memo = {}


def _join(queries, targets, k, upper=False):
    """the numpy join over EVERY pair -> (sorted hits [(q, t, d)], nearest words, per-query counts); computed once per distinct batch"""
    key = (tuple(queries), tuple(targets), k, upper)
    if key not in _join_memo:
        by_len = {}
        for t, s in enumerate(targets):
            by_len.setdefault(len(s), []).append(t)
        groups = {n: (np.array(idx), np.frombuffer(b"".join(targets[t] for t in idx), np.uint8).reshape(len(idx), n))
                  for n, idx in by_len.items()}
        hits, nearest, per_query = [], [], []
        for q, s in enumerate(queries):
            row = []
            if len(s) in groups:
                idx, rows = groups[len(s)]
                d = (rows != np.frombuffer(s, np.uint8)[None, :]).sum(axis=1)
                row = [(q, int(t), int(x)) for t, x in zip(idx, d) if x <= k and (not upper or t > q)]
            hits += row
            nearest.append(min((x << 32 | t) for _, t, x in row) if row else ALL_ONES)
            per_query.append(len(row))
        _join_memo[key] = (hits, nearest, per_query)
    return _join_memo[key]


def _got(B, torch, hits, count, nearest, per_query, cut=False):
    torch.cuda.synchronize()
    q, t, d = B.cross_to_arrays(hits, count, allow_cut=cut)
    words = None if nearest is None else [int(w) for w in nearest.cpu().numpy().view(np.uint64)]
    counts = None if per_query is None else [int(c) for c in per_query.cpu().numpy().view(np.uint32)]
    return list(zip(q.tolist(), t.tolist(), d.tolist())), int(count.item()), words, counts


def _check(B, torch, qs, ts, queries, targets, k, upper=False):
    want = _join(queries, targets, k, upper)
    hits, count, nearest, per_query = B.hamming_cross(qs, ts, k, cap=len(queries) * len(targets), nearest=True, per_query=True, upper=upper)
    got, n, near, counts = _got(B, torch, hits, count, nearest, per_query)
    where = (len(queries), len(targets), k, upper)
    assert n == len(want[0]) and got == want[0], where
    assert near == want[1], where
    assert counts == want[2], where
    return want[0]


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("nw", [4, 8, 16])
def test_every_pair_equals_the_join(nw, nt):
    """mixed lengths up to 4 nw bytes; nq on both sides of the staging chunk (256 / nw queries) and over two query tiles"""
    torch, T, B = _mods()
    chunk = 256 // nw                                              # = the query tile of a small batch
    total = 0
    for nq in (1, chunk - 1, chunk, chunk + 1, 2 * chunk + 3):
        queries, targets = _batch(9000 + 10 * nw + nq, nq, nt, ALPHABETS["acgt"], LENS[nw])
        qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
        for k in (0, 1, 2, 3):
            total += len(_check(B, torch, qs, ts, queries, targets, k))
            longest = max(len(q) for q in queries)
            assert _kernel() == "ham_cross_kernel<%d>" % (4 if longest <= 16 else 8 if longest <= 32 else 16)
    assert total > 0 or nt == 1


@pytest.mark.parametrize("nt", NTS)
def test_fixed_16_byte_tags(nt):
    torch, T, B = _mods()
    g = Dg.rng(9100 + nt)
    acgt = ALPHABETS["acgt"]
    total = 0
    for nq in (1, 63, 64, 65, 131):
        targets = [_rand(g, acgt, 16) for _ in range(nt)]
        queries = [_substitute(g, targets[int(g.integers(nt))], int(g.integers(0, 4)), acgt) for _ in range(nq)]
        arr = lambda s: np.frombuffer(b"".join(s), np.uint8).reshape(len(s), 16)   # noqa: E731
        qs, ts = B.Strings.from_fixed(arr(queries)), B.Strings.from_fixed(arr(targets))
        for k in (0, 1, 2):
            total += len(_check(B, torch, qs, ts, queries, targets, k))
            assert _kernel() == "ham_cross_kernel<4>"
    assert total >= 5


def test_a_small_query_tile_makes_many_tiles(monkeypatch):
    torch, T, B = _mods()
    monkeypatch.setenv("TA_HCROSS_QTILE", "5")                     # (read at every call under TA_TUNING: tiles of 5, a partial chunk each)
    for nw, nq in ((4, 2 * 5 + 3), (16, 70)):
        queries, targets = _batch(9200 + nw, nq, 257, ALPHABETS["lower"], LENS[nw])
        qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
        for k in (1, 3):
            _check(B, torch, qs, ts, queries, targets, k)
            _check(B, torch, qs, ts, queries, targets, k, upper=True)


@pytest.mark.parametrize("name", list(ALPHABETS))
def test_every_alphabet(name):
    torch, T, B = _mods()
    queries, targets = _batch(9300 + len(name), 35, 130, ALPHABETS[name], LENS[16])
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    for k in (0, 1, 2, 33):
        _check(B, torch, qs, ts, queries, targets, k)
    g = Dg.rng(9301)
    targets = [_rand(g, ALPHABETS[name], 16) for _ in range(130)]
    queries = [_substitute(g, targets[i], i % 4, ALPHABETS[name]) for i in range(65)]
    arr = lambda s: np.frombuffer(b"".join(s), np.uint8).reshape(len(s), 16)       # noqa: E731
    for k in (1, 2):
        _check(B, torch, B.Strings.from_fixed(arr(queries)), B.Strings.from_fixed(arr(targets)), queries, targets, k)


@pytest.mark.parametrize("qform", ["strided", "csr", "csr_unmeasured"])
@pytest.mark.parametrize("tform", ["strided", "csr", "csr_unmeasured"])
def test_strided_and_csr_sides(qform, tform):
    torch, T, B = _mods()
    g = Dg.rng(9400)
    nq, nt, n = 63, 65, 21                                         # 21 bytes: every string starts at another alignment
    acgt = ALPHABETS["acgt"]
    queries = [_rand(g, acgt, n) for _ in range(nq)]
    targets = [_substitute(g, queries[i % nq], i % 3, acgt) for i in range(nt)]

    def side(strings, form):
        if form == "strided":
            return B.Strings.from_fixed(np.frombuffer(b"".join(strings), np.uint8).reshape(len(strings), -1))
        s = B.Strings.from_list(strings)
        if form == "csr_unmeasured":
            s.max_len = 0                                          # "let the library measure it": one synchronisation
        return s

    qs, ts = side(queries, qform), side(targets, tform)
    for k in (1, 2):
        want = _check(B, torch, qs, ts, queries, targets, k)
        assert len(want) >= nt * 2 // 3 and _kernel() == "ham_cross_kernel<8>"


def test_duplicate_targets_ties_and_a_query_without_a_hit():
    torch, T, B = _mods()
    queries = [b"ACGTACGTACGT", b"TTTTTTTTTTTT", b"GGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGGG", b"", b"ACGTACGTACGA", b"ACGTACGTACG"]
    targets = [b"CCCCCCCCCCCC", b"ACGTACGTACGA", b"ACGTACGTACGC", b"ACGTACGTACGT", b"ACGTACGTACGA", b"ACGTACGTACGT", b"A", b""] * 9
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    hits, near, counts = _join(queries, targets, 1)
    # nearest takes the lowest index among equal targets, per-query counts every duplicate; a shifted tag (one byte shorter) never hits
    assert near[0] == (0 << 32 | 3) and counts[0] == 5 * 9 and near[4] == (0 << 32 | 1) and counts[4] == 5 * 9
    assert near[1] == ALL_ONES and counts[1] == 0 and near[2] == ALL_ONES and near[5] == ALL_ONES and counts[5] == 0
    assert near[3] == (0 << 32 | 7) and counts[3] == 9             # two empty strings: a hit with d = 0
    for k in (0, 1, 2):
        _check(B, torch, qs, ts, queries, targets, k)


def test_cap_cuts_the_records_not_the_count():
    torch, T, B = _mods()
    queries, targets = _batch(9500, 65, 130, ALPHABETS["acgt"], LENS[4])
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    want, want_near, want_counts = _join(queries, targets, 3)
    assert len(want) >= 64
    cap = len(want) // 2
    hits, count, nearest, per_query = B.hamming_cross(qs, ts, 3, cap=cap, nearest=True, per_query=True)
    got, n, near, counts = _got(B, torch, hits, count, nearest, per_query, cut=True)
    assert n == len(want)                                          # the count is unchanged
    assert len(got) == cap and len(set((q, t) for q, t, _ in got)) == cap   # no record twice
    assert set(got) <= set(want)                                   # every record is a true hit
    assert near == want_near and counts == want_counts             # neither depends on cap
    with pytest.raises(ValueError, match="larger cap"):
        B.cross_to_arrays(hits, count)
    # cap = 0 with a NULL hits buffer: the count, the nearest words and the per-query counts alone
    nearest0 = torch.full((len(queries),), 5, dtype=torch.int64, device="cuda")
    per_query0 = torch.full((len(queries),), 5, dtype=torch.int32, device="cuda")
    count0 = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    rc = T._n.lib().ta_hamming_cross(qs._ref(), qs.n, ts._ref(), ts.n, 3, 0, None, count0.data_ptr(), 0, nearest0.data_ptr(),
                                     per_query0.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(count0.item()) == len(want)
    assert [int(w) for w in nearest0.cpu().numpy().view(np.uint64)] == want_near
    assert per_query0.cpu().tolist() == want_counts
    # and without either per-query output
    rc = T._n.lib().ta_hamming_cross(qs._ref(), qs.n, ts._ref(), ts.n, 3, 0, None, count0.data_ptr(), 0, None, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and int(count0.item()) == len(want)


def test_k_of_64_and_more_hits_every_pair_of_equal_length():
    torch, T, B = _mods()
    g = Dg.rng(9600)
    for n in (16, 64):
        queries = [_rand(g, ALPHABETS["0..255"], n) for _ in range(40)]
        targets = [_rand(g, ALPHABETS["0..255"], n) for _ in range(70)]
        qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
        for k in (64, 65, 0xFFFFFFFF):                             # (2^32 - 1 must not overflow the kernel's 8 k + 7)
            want = _check(B, torch, qs, ts, queries, targets, k)
            assert len(want) == 40 * 70


def test_upper_on_a_set_against_itself():
    torch, T, B = _mods()
    g = Dg.rng(9700)
    acgt = ALPHABETS["acgt"]
    base = [_rand(g, acgt, 12) for _ in range(20)]
    umis = [_substitute(g, base[int(g.integers(20))], int(g.integers(0, 3)), acgt) for _ in range(130)]
    s = B.Strings.from_fixed(np.frombuffer(b"".join(umis), np.uint8).reshape(130, 12))
    for k in (1, 2):
        full = _check(B, torch, s, s, umis, umis, k)
        upper = _check(B, torch, s, s, umis, umis, k, upper=True)
        assert upper == [(q, t, d) for q, t, d in full if q < t]   # exactly the pairs i < j of the full join
        assert not any(q == t for q, t, _ in upper)
        diagonal = sum(1 for q, t, _ in full if q == t)
        assert diagonal == 130 and len(upper) == (len(full) - diagonal) // 2 and len(upper) > 30
    # the same with mixed lengths (CSR), where a wavefront's last targets decide where its tile stops
    queries, _ = _batch(9701, 130, 1, acgt, LENS[16])
    s = B.Strings.from_list(queries)
    full = _check(B, torch, s, s, queries, queries, 64)
    upper = _check(B, torch, s, s, queries, queries, 64, upper=True)
    assert upper == [(q, t, d) for q, t, d in full if q < t] and len(upper) > 130


def test_empty_sides():
    torch, T, B = _mods()
    some = B.Strings.from_list([b"ACGT", b"AC", b"TTT"])
    none = B.Strings.from_list([])
    for qs, ts in ((some, none), (none, some), (none, none)):
        for upper in (False, True):
            count = torch.full((1,), 9, dtype=torch.int64, device="cuda")
            nearest = torch.full((max(qs.n, 1),), 9, dtype=torch.int64, device="cuda")
            per_query = torch.full((max(qs.n, 1),), 9, dtype=torch.int32, device="cuda")
            B.hamming_cross(qs, ts, 3, cap=4, count=count, nearest=nearest, per_query=per_query, upper=upper)
            torch.cuda.synchronize()
            assert int(count.item()) == 0
            assert (nearest[:qs.n] == -1).all() and (per_query[:qs.n] == 0).all()


def test_a_measured_query_longer_than_64_bytes_is_unsupported():
    torch, T, B = _mods()
    qs = B.Strings.from_list([b"A" * 10, b"C" * 65])
    qs.max_len = 0
    with pytest.raises(NotImplementedError, match="64 bytes"):
        B.hamming_cross(qs, B.Strings.from_list([b"ACGT"]), 2)


def test_streams_repeated_calls_and_graph_replay():
    torch, T, B = _mods()
    variants = [_batch(9800 + v, 65, 130, ALPHABETS["acgt"], LENS[8]) for v in range(3)]
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
    want = lambda v: (lambda j: (j[0], len(j[0]), j[1], j[2]))(_join(*variants[v], 2))   # noqa: E731
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        put(0)
        out = B.hamming_cross(qs, ts, 2, cap=cap, nearest=True, per_query=True)          # a stream of its own
        s.synchronize()
        assert _got(B, torch, *out) == want(0)
        with torch.cuda.stream(s2):                                # a second stream, buffers of its own, while the first goes on
            out2 = B.hamming_cross(qs, ts, 2, cap=cap, nearest=True, per_query=True)
        for _ in range(2):                                         # back to back into the same buffers
            B.hamming_cross(qs, ts, 2, cap=cap, hits=out[0], count=out[1], nearest=out[2], per_query=out[3])
        s.synchronize()
        s2.synchronize()
        assert _got(B, torch, *out) == want(0) and _got(B, torch, *out2) == want(0)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            B.hamming_cross(qs, ts, 2, cap=cap, hits=out[0], count=out[1], nearest=out[2], per_query=out[3])
        for v in (1, 2):
            put(v)
            graph.replay()
            s.synchronize()
            assert _got(B, torch, *out) == want(v), v              # the counter read after each replay


def test_python_helpers_equal_a_double_loop_of_single_calls():
    torch, T, B = _mods()
    queries, targets = _batch(9900, 20, 30, ALPHABETS["acgt"], LENS[4])
    for k in (1, 3):
        want, nearest = [], []
        for q, a in enumerate(queries):
            row = []
            for t, b in enumerate(targets):
                if len(a) != len(b):
                    with pytest.raises(T.PanicError):              # the reference panics: never a hit
                        T.hamming(a, b)
                    continue
                d = T.hamming(a, b)
                if d <= k:
                    want.append((q, t, d))
                    row.append((d, t))
            nearest.append((min(row)[1], min(row)[0], len(row)) if row else None)
        assert T.hamming_cross_many(queries, targets, k) == want and len(want) > 0
        assert T.hamming_nearest_many(queries, targets, k) == nearest
        assert T.hamming_cross_many(queries, queries, k, upper=True) == \
            [(q, t, T.hamming(a, b)) for q, a in enumerate(queries) for t, b in enumerate(queries)
             if q < t and len(a) == len(b) and T.hamming(a, b) <= k]
    # more hits than the first call's room: one more call with room for the count
    many = [b"ACGT"] * 40
    assert T.hamming_cross_many(many, many, 0) == [(q, t, 0) for q in range(40) for t in range(40)]
    assert T.hamming_cross_many([], many, 1) == [] and T.hamming_nearest_many([b"AC"], [], 1) == [None]
