"""Batches for hamming_search_cross_with_opts (tests/test_hsearch_cross_opts_cpu.py, tests/test_gpu_hsearch_cross_opts*.py) on top of
tests/hsearch_cross_cases.py (its panel / reads / join): the needle lengths of the two-word route, the standard batch with a hit at every
distance 0..3 for a long needle, and hand-made pairs for the places where two words can go wrong.

LONG_LENS: 32 | 33 is where a needle starts to span both words (33 bytes: one position in the low word), 63 | 64 the top of the second
word; the lengths up to 32 sit wholly in the high word under an all-zero low word.  STD_LENS leaves the 1-byte needle out, as
hsearch_cross_cases.STD_LENS does: a NUL read of 1-5 bytes is then shorter than every non-empty needle (not marked)."""
import datagen as Dg
import hsearch_cross_cases as X

LONG_LENS = (0, 1, 31, 32, 33, 34, 40, 47, 48, 63, 64)
STD_LENS = (0, 31, 32, 33, 34, 40, 47, 48, 63, 64)
PANELS = (1, 5, 31, 32, 33, 65, 96)                               # G = 1, 8, 32; the 32-needle group boundary from both sides; three groups
KS = (0, 1, 3, 8, 31, 32, 33, 63, 64, 70)
PLANES_AT_64 = {0: 1, 1: 1, 3: 2, 8: 4, 31: 5, 32: 6, 33: 6, 63: 6, 64: 7, 70: 7}     # a panel whose longest needle is 64 bytes
ACGT, BYTES, ALL_ONES, NONE = X.ACGT, X.BYTES, X.ALL_ONES, X.NONE
join, reads, substitute = X.join, X.reads, X.substitute


def planes(k, needles):
    """the plane count the two-word route takes: the smallest B with 2^B - 1 >= min(k, longest needle)"""
    kc = min(k, max((len(nd) for nd in needles), default=0))
    return next(b for b in range(1, 8) if (1 << b) - 1 >= kc)


def panel(seed, nn, alphabet=ACGT, lens=LONG_LENS):
    return X.panel(seed, nn, alphabet, lens)


def std():
    """the batch most tests share: 33 needles of every length of STD_LENS (two groups: 32 and 1), 257 reads of
    hsearch_cross_cases.reads and four more that hold the first needle beyond 32 bytes with 0, 1, 2 and 3 substitutions"""
    needles = panel(900, 33, lens=STD_LENS)
    hays = reads(901, 257, needles)
    g = Dg.rng(902)
    long_one = next(nd for nd in needles if len(nd) > 32 and not X._period(nd))
    for d in range(4):
        hays.append(bytes(g.choice(ACGT, 40 + d)) + substitute(g, long_one, d, ACGT) + bytes(g.choice(ACGT, 50)))
    return needles, hays


def _mutate(nd, positions):
    s = bytearray(nd)
    for j in positions:
        s[j] = ord("ACGT"[("ACGT".index(chr(s[j])) + 1) % 4])
    return bytes(s)


def hand_made():
    """-> a list of (tag, needle, haystack, k, want) with want = None (no hit) or (start, end, d, n_matches), for a 64-byte and a 33-byte
    needle; position j of a needle of n bytes is bit 64 - n + j of the 64: j < n - 32 is the LOW word.
    lo_over / lo_hit: m mismatches, all within the first n - 32 positions (m = 4 of 32, and 1 of 1): no hit at k = m - 1, d = m at k = m
    boundary: mismatches at exactly j = n - 33 and j = n - 32, the two sides of the word boundary
    hi_only: mismatches only in the last 32 positions
    ends: one window at offset 0 and one ending on the haystack's last byte"""
    g = Dg.rng(0x4D2)
    fill = lambda n: bytes(g.choice(ACGT, n))                      # noqa: E731
    out = []
    for n, lo in ((64, (0, 9, 20, 31)), (33, (0,))):
        nd = fill(n)
        m = len(lo)
        assert all(j < n - 32 for j in lo)
        hay = fill(57) + _mutate(nd, lo) + fill(41)
        out.append(("lo_over%d" % n, nd, hay, m - 1, None))
        out.append(("lo_hit%d" % n, nd, hay, m, (57, 57 + n, m, 1)))
        hay = fill(23) + _mutate(nd, (n - 33, n - 32)) + fill(70)
        out.append(("boundary_over%d" % n, nd, hay, 1, None))
        out.append(("boundary%d" % n, nd, hay, 2, (23, 23 + n, 2, 1)))
        hi = (n - 32, n - 17, n - 1)
        hay = fill(5) + _mutate(nd, hi) + fill(90)
        out.append(("hi_only_over%d" % n, nd, hay, 2, None))
        out.append(("hi_only%d" % n, nd, hay, 3, (5, 5 + n, 3, 1)))
        hay = nd + fill(77) + nd
        out.append(("ends%d" % n, nd, hay, 2, (0, n, 0, 2)))
    return out
