"""Batches and the oracle join for hamming_search_cross (tests/test_hsearch_cross_cpu.py, tests/test_gpu_hsearch_cross*.py).

panel() mixes the needle lengths that matter (0, 1, the register forms' edges 8 | 9, 16 | 17, 24 | 25, 31, 32) in one panel, repeats some
needles (the nearest tie goes to the lower index) and makes some periodic (two overlapping windows at the same count: there is no fold).
reads() mixes the haystack lengths that matter (0, 1, 3, 4, 5, one byte shorter than a needle, 100-250) and plants needles with 0-2
SUBSTITUTIONS: once, twice apart (n_matches = 2), twice overlapping, two different ones, one at offset 0 and one ending at the last byte;
every eleventh read holds one 0x00 byte (first, middle, last byte in turn).  join() is the oracle hamming_search_simd_with_opts(.., Best)
over EVERY (needle, haystack) pair, ValueError standing for the NUL verdict, computed once per distinct batch.

STD_LENS leaves the 1-byte needle out: in the standard batch a NUL read of 1-5 bytes is then shorter than every non-empty needle (not an
error, not marked), which a panel with a 1-byte needle cannot show."""
import numpy as np

import datagen as Dg
import oracle_lib as O

NEEDLE_LENS = (0, 1, 8, 9, 16, 17, 24, 25, 31, 32)
STD_LENS = (0, 8, 9, 16, 17, 24, 25, 31, 32)
PANELS = (1, 2, 3, 5, 16, 31, 32, 33, 63, 64, 65, 96, 130)
KS = (0, 1, 2, 3, 4, 8, 16, 31, 32, 40)
ACGT = np.frombuffer(b"ACGT", np.uint8)
BYTES = np.arange(1, 256, dtype=np.uint8)
ALL_ONES = 0xFFFFFFFFFFFFFFFF
NONE = 0xFFFFFFFF


def planes(k, needles):
    """the plane count the call takes: the smallest B with 2^B - 1 >= min(k, longest needle)"""
    kc = min(k, max((len(nd) for nd in needles), default=0))
    return next(b for b in range(1, 7) if (1 << b) - 1 >= kc)


def _rand(g, alphabet, n):
    return bytes(g.choice(alphabet, n)) if n else b""


def substitute(g, s, edits, alphabet):
    """`edits` distinct positions of s replaced by another symbol"""
    s = bytearray(s)
    for p in g.permutation(len(s))[:edits]:
        s[p] = int(g.choice([c for c in alphabet[:8] if c != s[p]]))
    return bytes(s)


def _period(nd):
    return next((q for q in (2, 3) if len(nd) > q and nd == (nd[:q] * len(nd))[:len(nd)]), None)


def panel(seed, nn, alphabet=ACGT, lens=NEEDLE_LENS):
    """nn needles: the lengths of `lens` in a shuffled round-robin (a panel of one takes the longest), every seventh needle a copy of an
    earlier one, every fifth periodic (period 2 or 3)"""
    g = Dg.rng(seed)
    order = [int(x) for x in g.permutation(len(lens))]
    out = []
    for p in range(nn):
        n = lens[order[p % len(lens)]] if nn > 1 else max(lens)
        if p % 7 == 6:
            out.append(out[int(g.integers(p))])
        elif p % 5 == 4 and n > 3:
            q = 2 + p % 2
            unit = bytes(g.permutation(alphabet)[:q])
            out.append((unit * n)[:n])
        else:
            out.append(_rand(g, alphabet, n))
    return out


def reads(seed, nh, needles, alphabet=ACGT, lo=100, hi=250):
    """nh haystacks; by i mod 9: 0-2 one needle planted with 0-2 substitutions, 3 one needle twice apart, 4 one needle twice overlapping
    (a periodic needle one period apart: two windows at the same count), 5 a short haystack (0, 1, 3, 4, 5 bytes, or one byte less than a
    needle), 6 nothing planted, 7 two different needles, 8 one needle at offset 0 and one ending at the last byte.  i mod 11 == 10: one
    byte of the read becomes 0x00 -- read 32 is a 4-byte one"""
    g = Dg.rng(seed)
    real = [nd for nd in needles if len(nd) >= 8] or [nd for nd in needles if nd] or [b"ACGTACGT"]
    periodic = [nd for nd in real if _period(nd)]
    short = [0, 1, 3, 4, 5] + [len(nd) - 1 for nd in real[:3]]
    out = []
    for i in range(nh):
        kind = i % 9
        if kind == 5:
            n = short[(i // 9) % len(short)]
            nd = real[int(g.integers(len(real)))]
            h = bytearray(nd[:n] if (i // 9) % 2 and n <= len(nd) else _rand(g, alphabet, n))
        else:
            h = bytearray(_rand(g, alphabet, int(g.integers(lo, hi + 1))))
            nd = real[int(g.integers(len(real)))]

            def plant(s, at):
                at = max(0, min(at, len(h) - len(s)))
                h[at:at + len(s)] = s

            if kind <= 2:
                plant(substitute(g, nd, kind, alphabet), int(g.integers(0, len(h))))
            elif kind == 3:
                plant(nd, 5)
                plant(nd, 5 + len(nd) + 20)
            elif kind == 4:
                if periodic:
                    nd = periodic[int(g.integers(len(periodic)))]
                plant(nd, 30)
                plant(nd, 30 + (_period(nd) or max(len(nd) // 2, 1)))
            elif kind == 7:
                plant(substitute(g, nd, 1, alphabet), 3)
                plant(real[int(g.integers(len(real)))], len(h) - 40)
            elif kind == 8:
                plant(nd, 0)
                other = real[int(g.integers(len(real)))]
                plant(other, len(h) - len(other))
        if i % 11 == 10 and h:
            h[(0, len(h) // 2, len(h) - 1)[(i // 11) % 3]] = 0
        out.append(bytes(h))
    return out


_memo = {}


def join(needles, hays, k):
    """the oracle over EVERY pair -> (records [(i, p, start, end, k, n_matches)] sorted by (i, p), nearest words, best [(start, end, k)],
    per-haystack counts with NONE where a pair of the haystack is the NUL verdict); memoised per batch"""
    key = (tuple(needles), tuple(hays), k)
    if key not in _memo:
        recs, nearest, best, per = [], [], [], []
        for i, h in enumerate(hays):
            row, nul, cache = [], False, {}
            for p, nd in enumerate(needles):
                if nd not in cache:                                # (duplicate needles)
                    try:
                        cache[nd] = O.hamming_search_simd_with_opts(nd, h, k, O.BEST)
                    except ValueError:
                        cache[nd] = None
                r = cache[nd]
                if r is None:
                    nul = True
                elif r:
                    assert r[0][1] == r[0][0] + len(nd)
                    row.append((i, p, r[0][0], r[0][1], r[0][2], len(r)))
            assert not (nul and row)                               # (a NUL haystack has no hit at all)
            recs += row
            per.append(NONE if nul else len(row))
            if row:
                w = min((x[4] << 32 | x[1]) for x in row)
                nearest.append(w)
                best.append(next((x[2], x[3], x[4]) for x in row if x[1] == (w & 0xFFFFFFFF)))
            else:
                nearest.append(ALL_ONES)
                best.append((0, 0, NONE))
        _memo[key] = (recs, nearest, best, per)
    return _memo[key]
