"""Batches and the oracle join for levenshtein_search_cross (tests/test_search_cross_cpu.py, tests/test_gpu_search_cross*.py).

panel() mixes the needle lengths that matter (0, 1, the register forms' edges 8 | 9, 16 | 17, 24 | 25, 31, 32) in one panel, so that
needles the scan takes (kf < n) and needles it does not (n == 0, kf >= n) share a group, and repeats some needles (the nearest tie goes
to the lower index).  reads() mixes the haystack lengths that matter (0, 1, 3, 4, 5, shorter than a needle, 100-250) and plants needles
with 0-2 edits: once, twice apart (n_matches = 2) and twice overlapping (the Best fold).  join() is the oracle over EVERY (needle,
haystack) pair, computed once per distinct batch."""
import numpy as np

import datagen as Dg
import oracle_lib as O

COSTS = [(1, 1, 0, None), (1, 1, 0, 1), (3, 1, 0, None), (1, 1, 2, None), (2, 1, 2, None), (2, 2, 1, 3), (1, 2, 0, 1), (2, 3, 1, None)]
NEEDLE_LENS = (0, 1, 8, 9, 16, 17, 24, 25, 31, 32)
PANELS = (1, 2, 3, 5, 16, 31, 32, 33, 63, 64, 65, 96, 130)
ACGT = np.frombuffer(b"ACGT", np.uint8)
BYTES = np.arange(0, 256, dtype=np.uint8)
ALL_ONES = 0xFFFFFFFFFFFFFFFF
NONE = 0xFFFFFFFF


def _rand(g, alphabet, n):
    return bytes(g.choice(alphabet, n)) if n else b""


def mutate(g, s, edits, alphabet):
    s = bytearray(s)
    for _ in range(edits):
        op, p = int(g.integers(3)), int(g.integers(len(s) + 1))
        if op == 0 or not s:
            s.insert(p, int(g.choice(alphabet)))
        elif op == 1:
            del s[min(p, len(s) - 1)]
        else:
            s[min(p, len(s) - 1)] = int(g.choice(alphabet))
    return bytes(s)


def panel(seed, nn, alphabet=ACGT, lens=NEEDLE_LENS):
    """nn needles: the lengths of `lens` in a shuffled round-robin (a panel of one takes the longest), every seventh needle a copy of an
    earlier one"""
    g = Dg.rng(seed)
    order = [int(x) for x in g.permutation(len(lens))]
    out = []
    for p in range(nn):
        if p % 7 == 6:
            out.append(out[int(g.integers(p))])
        else:
            out.append(_rand(g, alphabet, lens[order[p % len(lens)]] if nn > 1 else max(lens)))
    return out


def reads(seed, nh, needles, alphabet=ACGT, lo=100, hi=250):
    """nh haystacks; by i mod 8: 0-2 one needle planted with 0-2 edits, 3 one needle twice apart, 4 one needle twice overlapping, 5 a
    short haystack (0, 1, 3, 4, 5 bytes, or one byte less than a needle), 6 nothing planted, 7 two different needles"""
    g = Dg.rng(seed)
    real = [nd for nd in needles if len(nd) >= 8] or [nd for nd in needles if nd] or [b"ACGTACGT"]
    short = [0, 1, 3, 4, 5] + [len(nd) - 1 for nd in real[:3]]
    out = []
    for i in range(nh):
        kind = i % 8
        if kind == 5:
            n = short[(i // 8) % len(short)]
            nd = real[int(g.integers(len(real)))]
            out.append(nd[:n] if (i // 8) % 2 and n <= len(nd) else _rand(g, alphabet, n))
            continue
        h = bytearray(_rand(g, alphabet, int(g.integers(lo, hi + 1))))
        nd = real[int(g.integers(len(real)))]

        def plant(s, at):
            at = max(0, min(at, len(h) - len(s)))
            h[at:at + len(s)] = s

        if kind <= 2:
            plant(mutate(g, nd, kind, alphabet), int(g.integers(0, len(h))))
        elif kind == 3:
            plant(nd, 5)
            plant(nd, 5 + len(nd) + 20)
        elif kind == 4:
            plant(nd, 30)
            plant(nd, 30 + max(len(nd) // 2, 1))
        elif kind == 7:
            plant(mutate(g, nd, 1, alphabet), 3)
            plant(real[int(g.integers(len(real)))], len(h) - 40)
        out.append(bytes(h))
    return out


_memo = {}


def join(needles, hays, k, costs, anchored):
    """the oracle over EVERY pair -> (records [(i, p, start, end, k, n_matches)] sorted by (i, p), nearest words, best [(start, end, k)],
    per-haystack counts); memoised per batch"""
    key = (tuple(needles), tuple(hays), k, costs, bool(anchored))
    if key not in _memo:
        recs, nearest, best, per = [], [], [], []
        cache = {}
        for i, h in enumerate(hays):
            row = []
            for p, nd in enumerate(needles):
                if (nd, h) not in cache:                           # (duplicate needles)
                    cache[(nd, h)] = O.levenshtein_search_naive_with_opts(nd, h, k, O.BEST, costs, anchored)
                r = cache[(nd, h)]
                if r:
                    row.append((i, p, r[0][0], r[0][1], r[0][2], len(r)))
            cache.clear()
            recs += row
            per.append(len(row))
            if row:
                w = min((x[4] << 32 | x[1]) for x in row)
                nearest.append(w)
                best.append(next((x[2], x[3], x[4]) for x in row if x[1] == (w & 0xFFFFFFFF)))
            else:
                nearest.append(ALL_ONES)
                best.append((0, 0, NONE))
        _memo[key] = (recs, nearest, best, per)
    return _memo[key]
