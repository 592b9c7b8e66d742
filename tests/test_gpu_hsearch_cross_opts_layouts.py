"""gpu: ta_hamming_search_cross_with_opts' two-word route under hostile memory layouts (tests/layout_arena.py), with the plans of
test_gpu_hsearch_cross_layouts.py: both sides re-hosted with odd blob alignments, stride != len, off[0] > 0, CSR views between decoy
rows, and bytes around the strings that echo the other side, continue a needle behind the last haystack or hold NULs (0x00, 0x0C,
0xFF) -- every output inside guard bands.  The plain layout is checked against the oracle over every pair; every hostile layout must give the plain layout's answers and leave the guards
untouched: NUL bytes AROUND the strings mark no haystack (only the reads that hold one are marked), and a needle that continues behind
a haystack's last byte creates no hit."""
import numpy as np
import pytest

import datagen as Dg
import hsearch_cross_cases as X
import hsearch_cross_opts_cases as Y
import layout_arena as A
from layout_arena import Layout

pytestmark = pytest.mark.gpu


def _mods():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    return torch, T, B


def _shift_pairs():
    s = A.SHIFTS
    return [(s[i], s[(i + 4) % len(s)]) for i in range(len(s))]       # both sides see every shift, never the same one together


def _plans(ragged):
    if ragged:
        plans = [("view", Layout("csr_view", 15, fill="echo"), Layout("csr_view", 63, fill="echo")),
                 ("lead5", Layout("csr", 1, lead=5), Layout("csr", 65, lead=5, fill="0c")),
                 ("continue", Layout("csr", 3, lead=5, fill="nul"), Layout("csr", 17, lead=0, fill="continue")),
                 ("nul", Layout("csr", 7, lead=5, fill="nul"), Layout("csr", 9, lead=5, fill="nul"))]
        plans += [("shift%d" % sa, Layout("csr", sa, lead=5, fill="00"), Layout("csr", sb, lead=0, fill="ff")) for sa, sb in _shift_pairs()]
    else:
        plans = [("pad%d" % p, Layout("strided", 3, pad=p, fill="echo"), Layout("strided", 17, pad=A.PADS[(i + 2) % 5], fill="echo")) for i, p in enumerate(A.PADS)]
        plans += [("continue", Layout("strided", 5, pad=3, fill="nul"), Layout("strided", 1, pad=16, fill="continue")),
                  ("nul", Layout("strided", 1, pad=5, fill="nul"), Layout("strided", 3, pad=7, fill="nul"))]
        plans += [("shift%d" % sa, Layout("strided", sa, pad=1, fill="0c"), Layout("strided", sb, pad=3, fill="00")) for sa, sb in _shift_pairs()]
    return plans


def _sides(needles, hays, ln, lh):
    hn = A.host_side(needles, ln, partner=hays)
    hh = A.host_side(hays, lh, partner=needles, needles=max(needles, key=len), seed=1)
    assert hn.oracle == needles and hh.oracle == hays
    return A.to_strings(hn), A.to_strings(hh)


def _plain(B, needles, hays, ragged):
    if ragged:
        return B.Strings.from_list(needles), B.Strings.from_list(hays)
    arr = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)      # noqa: E731
    return B.Strings.from_fixed(arr(needles)), B.Strings.from_fixed(arr(hays))


def _run(nd, hs, k, cap):
    """every output guarded -> (sorted records, count, nearest words, best rows, per-haystack counts, kernel name)"""
    torch, T, B = _mods()
    gh, gc = A.guarded((cap, 6), torch.int32), A.guarded(1, torch.int64)
    gn, gb, gp = A.guarded(hs.n, torch.int64), A.guarded((hs.n, 3), torch.int64), A.guarded(hs.n, torch.int32)
    B.hamming_search_cross_with_opts(nd, hs, k, cap=cap, hits=gh.view, count=gc.view, nearest=gn.view, best=gb.view, per_haystack=gp.view)
    for g in (gh, gc, gn, gb, gp):
        g.check()
    cols = B.search_cross_to_arrays(gh.view, gc.view)
    recs = [tuple(int(x) for x in r) for r in zip(*cols)]
    best = [(int(r[0]), int(r[1]), int(r[2])) for r in gb.numpy().view(np.uint64).reshape(-1, 3)]      # (pad_ = 0: the whole word is k)
    assert not gn.unwritten().any() and not gb.unwritten().any() and not gp.unwritten().any()
    return (recs, int(gc.numpy()[0]), gn.numpy().view(np.uint64).tolist(), best, gp.numpy().view(np.uint32).tolist(), T.last_kernel_name())


def _batches(seed):
    """-> ragged (needles of every length of the panel up to 64 bytes, reads of every length class, NUL reads) and fixed (41-byte
    needles, 121-byte reads: every string of the strided form starts at another alignment)"""
    g = Dg.rng(seed)
    rn = Y.panel(seed, 33)
    rh = X.reads(seed + 1, 130, rn)
    fn = [bytes(g.choice(X.ACGT, 41)) for _ in range(20)]
    fh = [h[:121] for h in X.reads(seed + 2, 80, fn, lo=121, hi=250) if len(h) >= 121]
    return (rn, rh), (fn, fh)


@pytest.mark.parametrize("k", [2, 9])
def test_hamming_search_cross_with_opts_under_hostile_layouts(k):
    _, _, B = _mods()
    for ragged, (needles, hays) in zip((True, False), _batches(0x7D00)):
        want = X.join(needles, hays, k)
        cap = len(needles) * len(hays)
        plain = _run(*_plain(B, needles, hays, ragged), k, cap)
        print("route:", plain[5])
        assert max(map(len, needles)) > 32
        assert plain[5] == "ham_search_cross_w2_kernel<%d>" % Y.planes(k, needles), plain[5]
        assert plain[:5] == (want[0], len(want[0]), want[1], want[2], want[3]), "plain layout against the oracle"
        assert len(want[0]) > 30
        marked = [i for i, c in enumerate(plain[4]) if c == X.NONE]
        assert marked == [i for i, h in enumerate(hays) if 0 in h and len(h) >= min(len(nd) for nd in needles if nd)] and marked
        for tag, ln, lh in _plans(ragged):
            got = _run(*_sides(needles, hays, ln, lh), k, cap)
            assert got == plain, tag                               # ("nul": no other haystack marked; "continue": no other hit)
