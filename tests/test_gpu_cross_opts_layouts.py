"""gpu: ta_levenshtein_cross_with_opts under hostile memory layouts (tests/layout_arena.py), with the plans test_gpu_layouts.py applies to
the two older cross entries, on both of its kernels (queries of up to 64 bytes: lev_cross_kernel; of 65 .. 256: lev_cross_win_kernel):
both sides re-hosted with odd blob alignments, stride != len, off[0] > 0, CSR views between decoy rows and bytes around the strings
that echo the other side or hold 0x00 / 0x0C / 0xFF -- every output inside guard bands.  The plain layout is checked against the oracle
over every pair; every hostile layout must give the plain layout's answers and leave the guards untouched."""
import numpy as np
import pytest

import datagen as Dg
import layout_arena as A
import oracle_lib as O
from layout_arena import Layout

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
FOREIGN = ord("N")
NONE = 0xFFFFFFFF
ALL_ONES = 0xFFFFFFFFFFFFFFFF
LEV, RDAM = O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS


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
        plans = [("view", Layout("csr_view", 15, fill="echo"), Layout("csr_view", 63, fill="echo")), ("lead5", Layout("csr", 1, lead=5), Layout("csr", 65, lead=5, fill="0c"))]
        plans += [("shift%d" % sa, Layout("csr", sa, lead=5, fill="00"), Layout("csr", sb, lead=0, fill="ff")) for sa, sb in _shift_pairs()]
    else:
        plans = [("pad%d" % p, Layout("strided", 3, pad=p, fill="echo"), Layout("strided", 17, pad=A.PADS[(i + 2) % 5], fill="echo")) for i, p in enumerate(A.PADS)]
        plans += [("shift%d" % sa, Layout("strided", sa, pad=1, fill="0c"), Layout("strided", sb, pad=3, fill="00")) for sa, sb in _shift_pairs()]
    return plans


def _sides(a, b, la, lb):
    ha, hb = A.host_side(a, la, partner=b), A.host_side(b, lb, partner=a, seed=1)
    assert ha.oracle == a and hb.oracle == b
    return A.to_strings(ha), A.to_strings(hb)


def _plain(B, a, b, ragged):
    if ragged:
        return B.Strings.from_list(a), B.Strings.from_list(b)
    arr = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)      # noqa: E731
    return B.Strings.from_fixed(arr(a)), B.Strings.from_fixed(arr(b))


def _edit(g, s, edits):
    """`edits` random edits; substitutions write FOREIGN (never a match by accident)"""
    s = bytearray(s)
    for _ in range(edits):
        t = int(g.integers(0, 4))
        if t == 0 and s:
            s[int(g.integers(len(s)))] = FOREIGN
        elif t == 1:
            s.insert(int(g.integers(len(s) + 1)), int(g.choice(ACGT)))
        elif t == 2 and s:
            del s[int(g.integers(len(s)))]
        elif t == 3 and len(s) > 1:
            p = int(g.integers(len(s) - 1))
            s[p], s[p + 1] = s[p + 1], s[p]
    return bytes(s)


def _batches(seed, nq, nt, lo, hi, fixed):
    """-> ragged (queries of lo .. hi bytes, the last one hi; targets: half of them a query with 0 .. 5 edits, the others random within
    6 bytes of a query's length) and fixed (queries and targets of `fixed` bytes, an odd length: every string of the strided form starts
    at another alignment)"""
    g = Dg.rng(seed)
    rq = [bytes(g.choice(ACGT, int(g.integers(lo, hi + 1)))) for _ in range(nq)]
    rq[0], rq[-1] = bytes(g.choice(ACGT, lo)), bytes(g.choice(ACGT, hi))
    rt = [(_edit(g, rq[int(g.integers(nq))], int(g.integers(0, 6))) if i % 2
           else bytes(g.choice(ACGT, max(0, len(rq[int(g.integers(nq))]) + int(g.integers(-6, 7)))))) for i in range(nt)]
    fq = [bytes(g.choice(ACGT, fixed)) for _ in range(nq)]
    ft = [bytes(np.where(g.random(fixed) < 5.0 / fixed, FOREIGN, np.frombuffer(fq[int(g.integers(nq))], np.uint8)).astype(np.uint8)) if i % 3
          else bytes(g.choice(ACGT, fixed)) for i in range(nt)]
    return (rq, rt), (fq, ft)


def _run(call, qs, ts, cap):
    """call(qs, ts, cap, hits, count, nearest, per_query) with every output guarded -> (sorted hits, count, nearest words, per-query
    counts, kernel name)"""
    torch, T, B = _mods()
    gh, gc = A.guarded((cap, 4), torch.int32), A.guarded(1, torch.int64)
    gn, gp = A.guarded(qs.n, torch.int64), A.guarded(qs.n, torch.int32)
    call(qs, ts, cap, gh.view, gc.view, gn.view, gp.view)
    for g in (gh, gc, gn, gp):
        g.check()
    assert not gn.unwritten().any() and not gp.unwritten().any()
    q, t, d = B.cross_to_arrays(gh.view, gc.view)
    return (list(zip(q.tolist(), t.tolist(), d.tolist())), int(gc.numpy()[0]), gn.numpy().view(np.uint64).tolist(),
            gp.numpy().view(np.uint32).tolist(), T.last_kernel_name())


@pytest.mark.parametrize("shape", [(63, 65), (130, 515)])
@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("kernel", ["lev_cross_kernel<", "lev_cross_win_kernel<"])
@pytest.mark.parametrize("upper", [False, True])
def test_levenshtein_cross_with_opts_under_hostile_layouts(upper, kernel, costs, shape):
    """nq x nt on both sides of the wavefront and of the query tile; CSR views with decoys, off[0] = 5, every shift; strided strings of
    an odd length with every pad"""
    _, _, B = _mods()
    k = 5
    nq, nt = shape
    lo, hi, fixed = (0, 64, 21) if kernel == "lev_cross_kernel<" else (65, 256, 151)
    for ragged, (queries, targets) in zip((True, False), _batches(0x7E00 + nq + hi, nq, nt, lo, hi, fixed)):
        d = O.levenshtein_k_batch(O.csr_from_list([q for q in queries for _ in range(nt)]), O.csr_from_list([t for _ in range(nq) for t in targets]),
                                  k, costs).reshape(nq, nt)
        keep = lambda q, t: d[q, t] != NONE and (not upper or t > q)                           # noqa: E731
        hits = [(q, t, int(d[q, t])) for q in range(nq) for t in range(nt) if keep(q, t)]
        near = [min(((int(d[q, t]) << 32 | t) for t in range(nt) if keep(q, t)), default=ALL_ONES) for q in range(nq)]
        counts = [sum(1 for t in range(nt) if keep(q, t)) for q in range(nq)]
        assert (4 if upper else 16) <= len(hits) < nq * nt // 2                                  # (upper keeps about half)
        call = lambda qs, ts, cap, h, c, n, p: B.levenshtein_cross_with_opts(qs, ts, k, costs, cap=cap, hits=h, count=c, nearest=n,   # noqa: E731
                                                                             per_query=p, upper=upper)
        cap = nq * nt
        plain = _run(call, *_plain(B, queries, targets, ragged), cap)
        print("route:", plain[4])
        assert plain[4].startswith(kernel), plain[4]
        assert plain[:4] == (hits, len(hits), near, counts), "plain layout against the oracle"
        for tag, lq, lt in _plans(ragged):
            got = _run(call, *_sides(queries, targets, lq, lt), cap)
            assert got == plain, tag
