"""gpu: edit distance over 32-bit token sequences (ta_*_tokens): k, exp and trace batches, CSR and strided, against the int-item oracle
(tokens_ref.py) and the byte oracle on an equality-preserving coding; overflow pairs (more than 254 distinct common items) mixed in."""
import numpy as np
import pytest

import oracle_lib as O
import tokens_ref as R

pytestmark = pytest.mark.gpu

COSTS = [(1, 1, 0, None), (1, 1, 0, 1), (2, 3, 1, None), (2, 2, 1, 3)]
KS = [0, 8, 32, 100, 0xFFFFFFFF]
NONE = 0xFFFFFFFF


def _pairs(seed, n, vocab, max_len, overflow=0):
    rng = np.random.default_rng(seed)
    a, b = [], []
    for i in range(n):
        la = int(rng.integers(0, max_len + 1))
        x = rng.integers(0, vocab, la).tolist()
        if i % 2:                                               # mutated copy
            y = list(x)
            for _ in range(int(rng.integers(0, 12))):
                op, p = int(rng.integers(0, 3)), int(rng.integers(0, len(y) + 1))
                if op == 0 or not y:
                    y.insert(p, int(rng.integers(0, vocab)))
                elif op == 1:
                    del y[min(p, len(y) - 1)]
                else:
                    y[min(p, len(y) - 1)] = int(rng.integers(0, vocab))
        else:
            y = rng.integers(0, vocab, int(rng.integers(0, max_len + 1))).tolist()
        a.append(x); b.append(y)
    for t in range(overflow):                                   # permutations of 300-500 distinct tokens: no byte coding exists
        m = int(rng.integers(300, 501))
        base = (rng.permutation(60000)[:m] + (0xFFFFFF00 if t % 2 else 0)).astype(np.int64) % (1 << 32)
        x = base.tolist()
        y = list(x)
        for _ in range(6):
            p, q = int(rng.integers(0, m)), int(rng.integers(0, m))
            y[p], y[q] = y[q], y[p]
        if t % 3 == 2:
            y = y[: m - 40]
        pos = int(rng.integers(0, len(a) + 1))
        a.insert(pos, x); b.insert(pos, y)
    return a, b


_ref_cache = {}


def _dist(x, y, costs):
    """the unbounded distance (byte oracle on a coding where one exists, else the int-item oracle)"""
    key = (tuple(x), tuple(y), costs)
    if key not in _ref_cache:
        c = R.codes(x, y)
        if c is not None:
            r = O.levenshtein_naive_with_opts(c[0], c[1], False, costs)
            _ref_cache[key] = r[0]
        else:
            _ref_cache[key] = R.levenshtein(x, y, None, False, costs)[0]
    return _ref_cache[key]


def _want(a, b, k, costs):
    return np.array([(lambda d: d if d <= k else NONE)(_dist(x, y, costs)) for x, y in zip(a, b)], dtype=np.uint32)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("costs", COSTS)
@pytest.mark.parametrize("vocab", [50, 50000])
def test_k_batch_csr(costs, vocab):
    from triple_accel_amd import batch as B
    a, b = _pairs(11 + vocab, 120, vocab, 600 if vocab == 50 else 250, overflow=3)
    ta, tb = B.Tokens.from_list(a), B.Tokens.from_list(b)
    for k in KS:
        got = _u32(B.levenshtein_k_batch_tokens(ta, tb, k, costs))
        assert np.array_equal(got, _want(a, b, k, costs)), (k, costs)
    got = _u32(B.levenshtein_exp_batch_tokens(ta, tb, costs))
    assert np.array_equal(got, _want(a, b, NONE, costs))


@pytest.mark.parametrize("costs", COSTS)
def test_k_batch_strided(costs):
    import torch
    from triple_accel_amd import batch as B
    rng = np.random.default_rng(5)
    for L, vocab in ((64, 50), (64, 40000), (300, 30)):
        x = rng.integers(0, vocab, (70, L))
        y = x.copy()
        y[:, ::7] = rng.integers(0, vocab, y[:, ::7].shape)
        if L == 300:                                            # overflow rows: permutations of 300 distinct tokens
            for r in (3, 40):
                x[r] = rng.permutation(1 << 20)[:L]
                y[r] = x[r]
                y[r, 10], y[r, 200] = y[r, 200], y[r, 10]
        ta = B.Tokens.from_fixed(torch.from_numpy(x.astype(np.int64)))
        tb = B.Tokens.from_fixed(torch.from_numpy(y.astype(np.int32)))
        a, b = x.tolist(), y.tolist()
        for k in (0, 8, 32, NONE):
            assert np.array_equal(_u32(B.levenshtein_k_batch_tokens(ta, tb, k, costs)), _want(a, b, k, costs)), (L, k)


def _ref_script(x, y, k, costs):
    c = R.codes(x, y)
    if c is not None:
        d, tr = O.levenshtein_simd_k_with_opts(c[0], c[1], k, True, costs)
        return None if d is None else (d, tr)
    return R.levenshtein(x, y, k, True, costs)


def _norm(edits):
    return [(str(e[0]), int(e[1])) for e in edits]


@pytest.mark.parametrize("costs", COSTS)
def test_trace_batch(costs):
    from triple_accel_amd import batch as B
    a, b = _pairs(21, 60, 50000, 200, overflow=2)
    a2, b2 = _pairs(22, 40, 30, 120)
    a, b = a + a2, b + b2
    ta, tb = B.Tokens.from_list(a), B.Tokens.from_list(b)
    for k in (8, 100):
        out, edits, ne = B.levenshtein_trace_batch_tokens(ta, tb, k, costs, cap=2 * 1000 + 1)
        lists = B.edits_to_lists(edits, ne)
        d = _u32(out)
        for i, (x, y) in enumerate(zip(a, b)):
            r = _ref_script(x, y, k, costs)
            if r is None:
                assert d[i] == NONE, i
                continue
            assert d[i] == r[0], (i, k)
            assert _norm(lists[i]) == _norm(r[1]), (i, k)
    # cap cuts: n_edits says how long the script is, the first cap runs are kept
    out, edits, ne = B.levenshtein_trace_batch_tokens(ta, tb, 100, costs, cap=3)
    lists = B.edits_to_lists(edits, ne, allow_cut=True)
    nn = ne.cpu().numpy()
    for i, (x, y) in enumerate(zip(a, b)):
        r = _ref_script(x, y, 100, costs)
        if r is None:
            continue
        assert nn[i] == len(r[1]), i
        assert _norm(lists[i]) == _norm(r[1])[:3], i


@pytest.mark.parametrize("costs", COSTS)
def test_small_values_bit_identical_to_bytes(costs):
    import torch
    from triple_accel_amd import batch as B
    rng = np.random.default_rng(3)
    a = [bytes(rng.integers(0, 256, int(rng.integers(0, 90))).astype(np.uint8)) for _ in range(300)]
    b = [bytes(rng.integers(0, 256, int(rng.integers(0, 90))).astype(np.uint8)) for _ in range(300)]
    sa, sb = B.Strings.from_list(a), B.Strings.from_list(b)
    ta, tb = B.Tokens.from_list([list(s) for s in a]), B.Tokens.from_list([list(s) for s in b])
    for k in (0, 8, 32, NONE):
        assert torch.equal(B.levenshtein_k_batch(sa, sb, k, costs), B.levenshtein_k_batch_tokens(ta, tb, k, costs)), k
    o1, e1, n1 = B.levenshtein_trace_batch(sa, sb, 32, costs)
    o2, e2, n2 = B.levenshtein_trace_batch_tokens(ta, tb, 32, costs)
    assert torch.equal(o1, o2) and torch.equal(n1, n2)
    assert B.edits_to_lists(e1, n1, allow_cut=True) == B.edits_to_lists(e2, n2, allow_cut=True)


def test_graph_capture_with_overflow_pairs():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    a, b = _pairs(31, 200, 1000, 300, overflow=3)
    ta, tb = B.Tokens.from_list(a), B.Tokens.from_list(b)
    want = _want(a, b, 32, COSTS[0])
    T.thread_release()
    side = torch.cuda.Stream()
    out = torch.empty(len(a), dtype=torch.int32, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(NotImplementedError):                      # no scratch held: the capture would have to grow it
        with torch.cuda.graph(graph, stream=side):
            B.levenshtein_k_batch_tokens(ta, tb, 32, out=out)
    torch.cuda.synchronize()
    B.levenshtein_k_batch_tokens(ta, tb, 32, out=out)             # warm-up outside the capture sizes the scratch
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2, stream=side):
        B.levenshtein_k_batch_tokens(ta, tb, 32, out=out)
    out.fill_(7)
    graph2.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_u32(out), want)


def test_single_pair_api_agrees_with_batch():
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    a, b = _pairs(41, 16, 70000, 300, overflow=2)
    a.append([0, 254, 255, 0xFFFFFFFF, 7]); b.append([0xFFFFFFFF, 255, 0, 254])
    ta, tb = B.Tokens.from_list(a), B.Tokens.from_list(b)
    for costs in COSTS:
        got = _u32(B.levenshtein_k_batch_tokens(ta, tb, 100, costs))
        out, edits, ne = B.levenshtein_trace_batch_tokens(ta, tb, 100, costs, cap=1001)
        lists = B.edits_to_lists(edits, ne)
        for i, (x, y) in enumerate(zip(a, b)):
            r = T.levenshtein_tokens(x, y, 100, False, costs)
            assert (NONE if r is None else r[0]) == got[i], i
            r = T.levenshtein_tokens(np.array(x, dtype=np.int64), y, 100, True, costs)
            if r is None:
                assert got[i] == NONE
            else:
                assert r[0] == got[i] and _norm(r[1]) == _norm(lists[i]), i
    assert T.levenshtein_tokens([1, 2, 3], [1, 3]) == (1, None)
    assert T.levenshtein_tokens([], []) == (0, None)


def test_u8_wide_route_unchanged(monkeypatch):
    from triple_accel_amd import batch as B
    import datagen as Dg
    am, bm = Dg.pairs_mutated_fixed(4, 300, 200, 16)
    want = O.levenshtein_k_batch(O.csr_from_fixed(am), O.csr_from_fixed(bm), 40, (2, 2, 1, 3))
    monkeypatch.setenv("TA_FORCE_WIDE", "1")
    got = B.levenshtein_k_batch(B.Strings.from_fixed(am), B.Strings.from_fixed(bm), 40, (2, 2, 1, 3))
    assert np.array_equal(_u32(got), want)
