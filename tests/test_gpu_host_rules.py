"""gpu: the host helpers the batch entry points share (ta_internal.h: order_pairs with its caller's slots and flag), where a ragged batch
first takes the length-order path -- 4,096 pairs -- eagerly, inside a captured graph replayed on changed strings, and with its two
callers (ta_levenshtein_search_batch, ta_levenshtein_k_batch) enqueued back to back on one stream."""
import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
K = 4


def _lengths(seed, n):
    """lengths 0..40 of both sides, fixed over the versions of a batch: two thirds of the pairs within 3 of each other"""
    g = Dg.rng(seed)
    la = g.integers(0, 41, n)
    lb = np.where(g.integers(0, 3, n) > 0, np.clip(la + g.integers(-3, 4, n), 0, 40), g.integers(0, 41, n))
    la[:2], lb[:2] = (0, 40), (40, 0)                                    # both extremes on both sides
    return la, lb


def _strings(seed, la, lb):
    """strings of the given lengths over ACGT: b_i = a_i cut or padded to its own length, with up to three substitutions"""
    g = Dg.rng(seed)
    a, b = [], []
    for x, y in zip(la, lb):
        s = g.choice(ACGT, int(x))
        t = np.concatenate([s[:y], g.choice(ACGT, max(0, int(y) - int(x)))])
        for _ in range(int(g.integers(0, 4))):
            if len(t):
                t[int(g.integers(len(t)))] = g.choice(ACGT)
        a.append(s.tobytes()); b.append(t.tobytes())
    return a, b


def _side(B, strings):
    """a CSR side with max_len given (no measuring: the call is capturable) whose bytes can be rewritten in place"""
    s = B.Strings.from_list(strings)
    assert s.max_len == 40
    return s


def _rewrite(torch, side, strings):
    data = b"".join(strings)
    side.blob[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))


@pytest.mark.parametrize("n", [4096, 4095])
def test_k_batch_length_order_eager_and_replayed_on_changed_strings(n):
    """4,096 pairs: the smallest ragged batch whose pairs are taken in length order (the histogram zeroed by a kernel, as everything a
    captured call fills); 4,095: the unordered control.  Eager, then one captured graph replayed twice, the strings changed in between."""
    import torch
    from triple_accel_amd import batch as B
    la, lb = _lengths(0x4096, n)
    versions = [_strings(0x5000 + v, la, lb) for v in range(3)]
    want = [O.levenshtein_k_batch(O.csr_from_list(a), O.csr_from_list(b), K) for a, b in versions]
    assert all(((w != 0xFFFFFFFF).sum() > n // 8) and ((w == 0xFFFFFFFF).sum() > n // 8) for w in want)
    sa, sb = _side(B, versions[0][0]), _side(B, versions[0][1])
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        B.levenshtein_k_batch(sa, sb, K, out=out)                        # eager (and the scratch sized outside the capture)
        s.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want[0])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            B.levenshtein_k_batch(sa, sb, K, out=out)
        for v in (1, 2):
            _rewrite(torch, sa, versions[v][0]); _rewrite(torch, sb, versions[v][1])
            out.fill_(-7)
            graph.replay()
            s.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, want[v]), (n, v, np.flatnonzero(got != want[v])[:8])


def test_search_batch_then_k_batch_on_one_stream_keep_their_own_order():
    """Both callers of order_pairs, each over its own ragged batch of 4,096 pairs, enqueued on one stream with no synchronisation in
    between: each keeps its own order list, histogram and flag."""
    import torch
    from triple_accel_amd import batch as B
    n = 4096
    g = Dg.rng(0x5B01)
    needles = g.choice(ACGT, (n, 6)).astype(np.uint8)
    hays = []
    for i in range(n):
        h = bytearray(g.choice(ACGT, int(g.integers(0, 41))))
        if i % 2 and len(h) >= 6:
            p = int(g.integers(0, len(h) - 5))
            h[p:p + 6] = needles[i].tobytes()
        hays.append(bytes(h))
    hays[0], hays[1] = b"", bytes(g.choice(ACGT, 40))
    la, lb = _lengths(0x5B02, n)
    a, b = _strings(0x5B03, la, lb)
    nd, hs = B.Strings.from_fixed(needles), B.Strings.from_list(hays)
    sa, sb = B.Strings.from_list(a), B.Strings.from_list(b)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        m, c = B.levenshtein_search_batch(nd, hs, 1, O.BEST, (1, 1, 0, None), False, cap=42)
        out = B.levenshtein_k_batch(sa, sb, K)
        s.synchronize()
    got = [[tuple(x) for x in r] for r in B.matches_to_lists(m, c)]
    assert got == [O.levenshtein_search_naive_with_opts(needles[i].tobytes(), hays[i], 1, O.BEST, (1, 1, 0, None), False) for i in range(n)]
    assert np.array_equal(out.cpu().numpy().view(np.uint32), O.levenshtein_k_batch(O.csr_from_list(a), O.csr_from_list(b), K))
