"""The batches of the table form's tests (tests/test_emu_lev_bits_tab.py, tests/test_gpu_lev_bits_tab.py): the 209 pairs of
test_gpu_lev_bits_core.pairs() cut to the two lengths, and 209 more over the alphabets that attack two nibble tables."""
import functools

import numpy as np

import datagen as Dg
import oracle_lib as O
import test_gpu_lev_bits_core as Core

LEV, LEV2 = (1, 1, 0, None), (2, 2, 0, None)
NONE = 0xFFFFFFFF
# (len_a, len_b, k, costs)
SHAPES = [(129, 129, 32, LEV), (160, 160, 32, LEV), (256, 256, 32, LEV), (257, 257, 32, LEV), (288, 256, 32, LEV), (256, 288, 32, LEV),
          (250, 256, 32, LEV), (256, 250, 32, LEV), (256, 224, 32, LEV),
          (256, 256, 24, LEV), (256, 256, 25, LEV), (256, 256, 31, LEV), (256, 256, 64, LEV2)]
PAIR_COUNTS = [1, 63, 64, 65, 209]
# {0x00}; {0x0C, 0x0D}; nibbles that alias across rows; all-ones and all-zero nibbles; every byte value
ALPHABETS = [np.array([0x00]), np.array([0x0C, 0x0D]), np.array([0x11, 0x12, 0x21, 0x22]), np.array([0x0F, 0xF0, 0xFF, 0x00]), np.arange(256)]


@functools.lru_cache(maxsize=None)
def core_pairs(la, lb, ku):
    """pairs() at the longer length and unit threshold ku, each side cut to its own length (read only)"""
    a, b = Core.pairs(max(la, lb), ku)
    a, b = np.ascontiguousarray(a[:, :la]), np.ascontiguousarray(b[:, :lb])
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def alphabet_pairs(la, lb, ku):
    """209 pairs over the five alphabets in turn: 0 .. ku + 1 edits inside the alphabet, every seventh pair unrelated"""
    g = Dg.rng(0x7AB1E + 1000 * la + 10 * lb + ku)
    L = max(la, lb)
    a, b = np.zeros((Core.N, L), np.uint8), np.zeros((Core.N, L), np.uint8)
    for i in range(Core.N):
        al = ALPHABETS[i % len(ALPHABETS)]
        a[i] = al[g.integers(0, len(al), size=L)]
        b[i] = al[g.integers(0, len(al), size=L)] if i % 7 == 6 else Core._edit_within(g, a[i], int(g.integers(0, ku + 2)), al)
    a, b = np.ascontiguousarray(a[:, :la]), np.ascontiguousarray(b[:, :lb])
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def want(kind, la, lb, k, costs):
    a, b = (core_pairs if kind == "core" else alphabet_pairs)(la, lb, k // costs[0])
    return O.levenshtein_k_batch(O.csr_from_fixed(np.array(a)), O.csr_from_fixed(np.array(b)), k, costs)
