"""The batches of tests/test_emu_lev_bits_tab_regs.py and tests/test_gpu_lev_bits_tab_regs.py: the table form of the band kernel takes its
strings out of the parked registers, `b` piece by piece and `a` through a window that starts nlo & 15 bytes into a piece
(nlo = (k - |len_b - len_a|) / 2, + len_a - len_b where `a` is the longer string).  The geometries make nlo take every residue 0..15 mod 16
-- so every dword offset and every byte shift of the window -- with both signs of len_a - len_b, nlo = 0 (the whole warm-up in front of the
string) and nlo = 32 (none of it), and strings that end in the first, a middle and the last piece of a line and need a second and a third
burst (129, 143, 144, 255, 256, 257, 272, 385 bytes)."""
import functools

import numpy as np

import datagen as Dg
import oracle_lib as O

LEV = (1, 1, 0, None)
NONE = 0xFFFFFFFF
ALPHABETS = [np.array([0x00]), np.array([0x0C, 0x0D]), np.arange(256)]
# (len_a, len_b, k)
GEOMETRIES = [
    # len_b >= len_a: nlo = (k - diff) / 2 = 16 .. 0
    (129, 129, 32), (143, 145, 32), (140, 144, 32), (249, 255, 32), (248, 256, 32), (247, 257, 32), (260, 272, 32), (371, 385, 32),
    (128, 144, 32), (126, 144, 32), (236, 256, 32), (233, 255, 32), (233, 257, 32), (246, 272, 32), (357, 385, 32), (114, 144, 32),
    (97, 129, 32),
    # len_a > len_b: nlo = (k - diff) / 2 + diff = 17 .. 32
    (131, 129, 32), (385, 381, 32), (143, 137, 32), (272, 264, 32), (144, 134, 32), (256, 244, 32), (255, 241, 32), (144, 128, 32),
    (256, 238, 32), (257, 237, 32), (257, 235, 32), (255, 231, 32), (272, 246, 32), (385, 357, 32), (385, 355, 32), (288, 256, 32),
    # narrower bands, odd differences
    (256, 256, 25), (256, 256, 31), (256, 255, 24), (385, 385, 27), (256, 259, 31), (143, 144, 29), (272, 257, 30),
]


def nlo(la, lb, k):
    diff = abs(la - lb)
    return (k - diff) // 2 + (diff if la > lb else 0)


@functools.lru_cache(maxsize=None)
def pairs(la, lb, k, n):
    """n pairs over the three alphabets in turn; the even ones are copies of `a` brought to len_b by insertions or deletions and then given
    up to k - diff substitutions (within k by construction), the odd ones unrelated.  Read only."""
    g = Dg.rng(0x4E65 + 100000 * la + 100 * lb + k)
    diff = abs(la - lb)
    a, b = np.zeros((n, la), np.uint8), np.zeros((n, lb), np.uint8)
    for i in range(n):
        al = ALPHABETS[i % len(ALPHABETS)].astype(np.uint8)
        a[i] = al[g.integers(0, len(al), size=la)]
        if i % 2:
            b[i] = al[g.integers(0, len(al), size=lb)]
            continue
        s = bytearray(a[i].tobytes())
        for _ in range(diff):
            if la > lb:
                del s[int(g.integers(0, len(s)))]
            else:
                s.insert(int(g.integers(0, len(s) + 1)), int(al[int(g.integers(0, len(al)))]))
        for _ in range(int(g.integers(0, k - diff + 1))):
            s[int(g.integers(0, len(s)))] = int(al[int(g.integers(0, len(al)))])
        b[i] = np.frombuffer(bytes(s), np.uint8)
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def want(la, lb, k, n):
    a, b = pairs(la, lb, k, n)
    return O.levenshtein_k_batch(O.csr_from_fixed(np.array(a)), O.csr_from_fixed(np.array(b)), k, LEV)
