"""The batches of the table form's depth tests (tests/test_emu_lev_bits_tab_depth.py, tests/test_gpu_lev_bits_tab_depth.py): the smallest
shapes at which the order of the LDS stream inside a span can go wrong.  101 pairs (a ragged second wavefront); column counts whose last
span is a tail of 1, 2, 3, 15 or 16 columns ending in phase 0 and in phase 1, and counts of whole spans only; `a` as long as `b`, 6 bytes
shorter and 5 longer, where it stays above 128 bytes (the window starts at a piece's edge and inside one: nlo & 15 zero and not); 24 and
32 errors.  Mutated pairs 10..20 edits apart, every fifth `b` random."""
import functools

import numpy as np

import datagen as Dg
import oracle_lib as O

LEV = (1, 1, 0, None)
NONE = 0xFFFFFFFF
N = 101
B_LENS = [129, 130, 131, 143, 144, 145, 146, 160, 161, 175, 176, 177, 255, 256]
# (len_a, len_b, k)
SHAPES = [(lb + d, lb, k) for lb in B_LENS for d in (0, -6, 5) if lb + d > 128 for k in (24, 32)]


@functools.lru_cache(maxsize=None)
def pairs(la, lb):
    """N pairs made at the longer length, each side cut to its own (read only)"""
    L = max(la, lb)
    a, b = Dg.pairs_mutated_fixed(0xDE97 + 1000 * la + lb, N, L, 20)
    b[4::5] = Dg.random_bytes(Dg.rng(0xDE98 + 1000 * la + lb), len(b[4::5]) * L).reshape(-1, L)
    a, b = np.ascontiguousarray(a[:, :la]), np.ascontiguousarray(b[:, :lb])
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def want(la, lb, k):
    a, b = pairs(la, lb)
    w = O.levenshtein_k_batch(O.csr_from_fixed(np.array(a)), O.csr_from_fixed(np.array(b)), k, LEV)
    w.setflags(write=False)
    return w


def check_shares(w):
    """more than half of a shape's answers are numbers and at least a tenth None (checked with the oracle alone when the seeds were chosen)"""
    assert (w != NONE).sum() > N // 2 and (w == NONE).sum() * 10 >= N, ((w != NONE).sum(), (w == NONE).sum())
