"""Batches for levenshtein_search_cross_with_opts (tests/test_search_cross_opts_cpu.py, tests/test_gpu_search_cross_opts*.py) on top of
tests/search_cross_cases.py: the needle lengths of the two-word route and four hand-made pairs for the places where two words can go wrong.

LONG_LENS: 32 | 33 is where a needle starts to span both words (33 bytes: one row in word 0), 63 | 64 the top of the second word; the
lengths up to 32 sit wholly in word 1 under an all-wildcard word 0."""
import numpy as np

import datagen as Dg
import search_cross_cases as X

LONG_LENS = (0, 1, 8, 31, 32, 33, 34, 47, 48, 63, 64)
PANELS = (1, 2, 3, 5, 16, 31, 32, 33, 63, 64, 65, 96)          # every G from 1 to 32, the 32-needle group boundary from both sides
RDAMERAU = (1, 1, 0, 1)
LEVENSHTEIN = (1, 1, 0, None)
ZERO = np.array([0x00], np.uint8)
ZERO_0C = np.array([0x00, 0x0C], np.uint8)


def panel(seed, nn, alphabet=X.ACGT):
    return X.panel(seed, nn, alphabet, lens=LONG_LENS)


def hand_made():
    """-> (needles, haystacks): needle p belongs to haystack p, and every needle meets every haystack
    0: 64 bytes of one byte in a haystack of the same byte -- the add's carry runs through all 64 rows and across the word boundary
    1: 34 bytes planted with bytes 0 and 1 transposed (restricted Damerau) -- rows 0 and 1 are word 0's two rows
    2: the same needle planted with bytes 1 and 2 transposed -- row 1 is word 0's top bit, row 2 word 1's lowest
    3: 33 bytes whose only mismatch is the first byte -- the one row in word 0
    4: a needle one byte longer than its haystack"""
    g = Dg.rng(0x5C2)
    fill = lambda n: bytes(g.choice(X.ACGT, n))                    # noqa: E731
    t = bytearray(fill(34))
    t[0:3] = b"ACG"                                                # three different bytes: each transposition is a real one
    t = bytes(t)
    f = bytearray(fill(33))
    f[0] = ord("A")
    f = bytes(f)
    lng = fill(40)
    needles = [b"A" * 64, t, t, f, lng]
    hays = [b"A" * 200,
            fill(80) + t[1:2] + t[0:1] + t[2:] + fill(80),
            fill(70) + t[0:1] + t[2:3] + t[1:2] + t[3:] + fill(90),
            fill(60) + b"C" + f[1:] + fill(60),
            lng[:39]]
    return needles, hays
