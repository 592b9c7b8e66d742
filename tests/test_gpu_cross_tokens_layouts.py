"""gpu: ta_levenshtein_cross_tokens under hostile memory layouts (tests/layout_arena.py): the strided form with stride > len and with
stride < len (overlapping windows), CSR sides whose offsets start above 0 and point into the middle of a larger batch, both behind a
values pointer that is not 16-byte aligned, and every item that belongs to no sequence of the batch -- the gaps, the decoy rows, what
lies in front of the first and behind the last item -- holding a hostile value: 0, all ones, or a token of the queries.  The entry
promises to read nothing outside a sequence's items, so the answers depend on the sequences alone; outputs are written inside guard
bands that must stay intact."""
import numpy as np
import pytest

import cross_tokens_cases as X
import datagen as Dg
import layout_arena as A
import oracle_lib as O

pytestmark = pytest.mark.gpu

MARGIN = 64


def _mods():
    import torch
    from triple_accel_amd import batch as B
    return torch, B


def _data(seed, nq=17, nt=130, fixed=None):
    """fixed = (query length, target length) for the strided form; else ragged sides.  Few distinct values: hits abound."""
    g = Dg.rng(seed)
    voc = X.vocab("32k")[:6] + [0, 0xFFFFFFFF]
    qlens = [fixed[0]] * nq if fixed else [64, 0, 33] + [int(x) for x in g.integers(0, 65, size=nq - 3)]
    queries = [X.rand_seq(g, voc, n) for n in qlens]
    targets = []
    for i in range(nt):
        t = X.edited(g, queries[int(g.integers(nq))], int(g.integers(0, 4)), voc)
        if fixed:                                                  # one length: cut or fill up
            t = (t + X.rand_seq(g, voc, fixed[1]))[:fixed[1]]
        targets.append(t)
    return queries, targets


def _hostile(queries):
    """what the items outside the sequences hold, one value per run of the test: 0, all ones, the queries' commonest token"""
    flat = [x for q in queries for x in q]
    return (0, 0xFFFFFFFF, max(set(flat), key=flat.count))


def _strided_host(seqs, stride, fill, shift):
    n, length = len(seqs), len(seqs[0])
    extent = (n - 1) * stride + length
    base = MARGIN + shift
    vals = np.full(base + extent + MARGIN, fill, dtype=np.int64)
    for i, s in enumerate(seqs):
        vals[base + i * stride:base + i * stride + length] = s
    seen = [tuple(int(x) for x in vals[base + i * stride:base + i * stride + length]) for i in range(n)]
    return vals, base, seen


def _strided(B, torch, seqs, stride, fill, shift=3):
    """the sequences (one length) `stride` items apart behind MARGIN + shift items of fill; stride < len: overlapping windows, the
    sequences the test then expects are read back from the arena"""
    n, length = len(seqs), len(seqs[0])
    vals, base, seen = _strided_host(seqs, stride, fill, shift)
    t = torch.from_numpy(vals.astype(np.uint32).view(np.int32)).cuda()
    tok = B.Tokens(t[base:], None, length=length, n=n, stride=stride)
    tok._arena = t
    return tok, seen


def _csr_view(B, torch, seqs, fill, seed):
    """the sequences as rows 3 .. 3 + n of a larger CSR batch whose first offset is 5 (layout_arena.host_tokens): decoy rows of hostile
    items in front and behind, the values pointer 3 items off alignment"""
    g = Dg.rng(seed)
    decoy = lambda: tuple([fill] * int(g.integers(1, 9)))           # noqa: E731
    rows = [decoy() for _ in range(3)] + list(seqs) + [decoy() for _ in range(2)]
    vals, base, off = A.host_tokens(rows, shift_items=3, lead=5, sentinel=fill, margin=MARGIN)
    whole = A.to_tokens(vals, base, off)
    tok = B.Tokens(whole.values, whole.off[3:3 + len(seqs) + 1], max_len=max(map(len, seqs)))
    tok._arena = whole
    assert int(tok.off[0].item()) > 0
    return tok


def _run(B, torch, qs, ts, queries, targets, k, costs, upper):
    want_hits, want_near, want_counts = X.join(queries, targets, k, costs, upper)
    nq, cap = len(queries), len(queries) * len(targets)
    hits, count = A.guarded((cap, 4), torch.int32), A.guarded(1, torch.int64)
    nearest, per_query = A.guarded(nq, torch.int64), A.guarded(nq, torch.int32)
    B.levenshtein_cross_tokens(qs, ts, k, costs, cap=cap, hits=hits.view, count=count.view, nearest=nearest.view, per_query=per_query.view,
                               upper=upper)
    for gd in (hits, count, nearest, per_query):
        gd.check()                                                 # (synchronises) the canaries around every output
    q, t, d = B.cross_to_arrays(hits.view, count.view)
    assert list(zip(q.tolist(), t.tolist(), d.tolist())) == want_hits and len(want_hits) >= 16
    assert [int(w) for w in nearest.numpy().view(np.uint64)] == want_near
    assert [int(c) for c in per_query.numpy().view(np.uint32)] == want_counts
    assert hits.unwritten()[len(want_hits):].all()                 # no record behind the count


@pytest.mark.parametrize("pad", [1, 5])
def test_strided_sides_with_stride_above_len(pad):
    torch, B = _mods()
    queries, targets = _data(13000 + pad, fixed=(33, 34))
    for fill in _hostile(queries):
        qs, seen_q = _strided(B, torch, queries, 33 + pad, fill)
        ts, seen_t = _strided(B, torch, targets, 34 + pad, fill, shift=1)
        assert seen_q == queries and seen_t == targets
        for k, costs, upper in ((3, O.LEVENSHTEIN_COSTS, False), (4, O.RDAMERAU_COSTS, True)):
            _run(B, torch, qs, ts, queries, targets, k, costs, upper)


@pytest.mark.parametrize("step", [1, 7])
def test_strided_sides_with_stride_below_len(step):
    torch, B = _mods()
    queries, targets = _data(13100 + step, fixed=(20, 21))
    for fill in _hostile(queries):
        qs, seen_q = _strided(B, torch, queries, step, fill)       # overlapping windows: the sequences are what the arena holds
        ts, seen_t = _strided(B, torch, targets, step, fill, shift=2)
        assert len(seen_q[0]) == 20 and seen_q[1][:20 - step] == seen_q[0][step:]
        for k, costs, upper in ((13, O.LEVENSHTEIN_COSTS, False), (15, O.RDAMERAU_COSTS, True)):
            _run(B, torch, qs, ts, seen_q, seen_t, k, costs, upper)


def test_csr_sides_inside_a_larger_batch():
    torch, B = _mods()
    queries, targets = _data(13200)
    for fill in _hostile(queries):
        qs, ts = _csr_view(B, torch, queries, fill, 1), _csr_view(B, torch, targets, fill, 2)
        for k, costs, upper in ((2, O.LEVENSHTEIN_COSTS, False), (3, O.RDAMERAU_COSTS, True), (5, (2, 2, 0, None), False)):
            _run(B, torch, qs, ts, queries, targets, k, costs, upper)
        qs.max_len = ts.max_len = 0                                # the bounds measured by the library: off[0] > 0 there too
        _run(B, torch, qs, ts, queries, targets, 2, O.LEVENSHTEIN_COSTS, False)


def test_mixed_forms_and_an_allocation_that_ends_with_the_last_item():
    torch, B = _mods()
    queries, targets = _data(13300, fixed=(31, 32))
    fill = _hostile(queries)[2]
    qs, _ = _strided(B, torch, queries, 40, fill)
    ts = B.Tokens.from_list(targets)                               # CSR, the values tensor exactly the items: nothing behind the last one
    assert ts.values.numel() == sum(map(len, targets))
    _run(B, torch, qs, ts, queries, targets, 3, O.RDAMERAU_COSTS, False)
    _run(B, torch, B.Tokens.from_list(queries), _strided(B, torch, targets, 33, fill)[0], queries, targets, 3, O.LEVENSHTEIN_COSTS, True)
