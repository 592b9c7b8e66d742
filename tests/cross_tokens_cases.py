"""What tests/test_cross_tokens_cpu.py and the gpu tests of ta_levenshtein_cross_tokens share (TEST INFRASTRUCTURE ONLY): the emulation
library of the token cross body with its home-slot function, the vocabularies, the hash-collision cases, token edits, and the reference.

The reference is never the code under test: a batch whose vocabulary holds at most 256 distinct values is mapped injectively to bytes,
any other batch pair by pair with tokens_ref.codes, and the C oracle's levenshtein_k_batch answers every pair."""
import ctypes as C
import os
import subprocess

import numpy as np

import datagen as Dg
import oracle_lib as O
import tokens_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_cross_tokens")
NONE = 0xFFFFFFFF
ALL_ONES = 0xFFFFFFFFFFFFFFFF
KMAX = 0xFFFFFFFF
COSTS = (O.LEVENSHTEIN_COSTS, O.RDAMERAU_COSTS)

_lib = None


def emu_lib():
    global _lib
    if _lib is None:
        path = os.path.join(EMU_DIR, "libta_emu_cross_tokens.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        _lib.emu_cross_tok_query.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                             C.c_void_p, C.c_void_p]
        _lib.emu_cross_tok_query.restype = C.c_int
        _lib.emu_cross_tok_table_clean.argtypes = [C.c_int]
        _lib.emu_cross_tok_table_clean.restype = C.c_int
        _lib.emu_cross_tok_home.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        _lib.emu_cross_tok_home.restype = None
        _lib.emu_cross_tok_slots.restype = C.c_uint32
    return _lib


def homes(values):
    """the slot at which the body's probe of each token starts (the body's own function, exported by the emulation library)"""
    x = np.ascontiguousarray(np.asarray(values, dtype=np.uint32))
    out = np.zeros(len(x), np.uint32)
    emu_lib().emu_cross_tok_home(x.ctypes.data, len(x), out.ctypes.data)
    return out


def slots():
    return int(emu_lib().emu_cross_tok_slots())


# ---------------------------------------------------------------- vocabularies
def vocab(name):
    """-> a list of distinct token values"""
    if name == "one":
        return [0x00C0FFEE]
    if name == "0+ff":
        return [0, 0xFFFFFFFF]
    if name == "low16":                                            # equal in the low 16 bits
        return [(i << 16) | 0x1234 for i in range(48)]
    if name == "high16":                                           # equal in the high 16 bits
        return [0xABCD0000 | (i * 257) for i in range(48)]
    if name == "32k":
        g = Dg.rng(77001)
        return sorted({int(x) for x in g.integers(0, 1 << 32, size=40000, dtype=np.uint64)})[:32768]
    if name == "bytes":
        return list(range(256))
    raise KeyError(name)


VOCABS = ("one", "0+ff", "low16", "high16", "32k", "bytes")


def rand_seq(g, voc, n):
    return tuple(int(voc[int(i)]) for i in g.integers(0, len(voc), size=n)) if n else ()


def edited(g, s, e, voc, swaps=True):
    """s after e random substitutions, insertions, deletions and (swaps) adjacent transpositions, with items of voc"""
    s = list(s)
    for _ in range(e):
        kind = int(g.integers(0, 4 if swaps else 3))
        if kind == 0 and s:
            s[int(g.integers(len(s)))] = int(voc[int(g.integers(len(voc)))])
        elif kind == 1:
            s.insert(int(g.integers(len(s) + 1)), int(voc[int(g.integers(len(voc)))]))
        elif kind == 2 and s:
            del s[int(g.integers(len(s)))]
        elif kind == 3 and len(s) > 1:
            p = int(g.integers(len(s) - 1))
            s[p], s[p + 1] = s[p + 1], s[p]
    return tuple(s)


# ---------------------------------------------------------------- tokens that collide in the body's table
_pool = None


def colliding(count, slot=None, exclude=()):
    """`count` distinct tokens whose probes all start at one slot (`slot`, or the one the token 1 starts at), none of them in `exclude`"""
    global _pool
    if _pool is None:
        xs = np.unique(Dg.rng(77100).integers(1, 1 << 32, size=200000, dtype=np.uint64).astype(np.uint32))
        _pool = (xs, homes(xs))
    xs, hs = _pool
    slot = int(homes([1])[0]) if slot is None else int(slot)
    ex = set(int(x) for x in exclude)
    got = [int(x) for x in xs[hs == slot] if int(x) not in ex][:count]
    assert len(got) == count, (slot, count, len(got))
    assert len(set(got)) == count and (homes(got) == slot).all()   # the precondition, by the body's own function
    return got


def case_longest_chain():
    """(a) a query of 64 distinct tokens that all start at one slot -> (query, targets)"""
    q = tuple(colliding(64))
    g = Dg.rng(77101)
    others = colliding(16, exclude=q)                              # absent from the query, same home slot: the whole chain is walked
    targets = [q, q[::-1], q[1:], q[:-1], q[:32], q[32:], q[:31] + (others[0],) + q[32:], tuple(others), q + tuple(others[:4]),
               (q[1], q[0]) + q[2:]]
    targets += [edited(g, q, e, list(q) + others) for e in (1, 2, 3, 5) for _ in range(4)]
    return q, targets


def case_two_on_one_slot(m=20):
    """(b) a query whose first two distinct tokens share a home slot, the rest spread by the hash"""
    a, b = colliding(2, slot=5)
    g = Dg.rng(77102)
    pool = vocab("32k")[:200]
    rest = [x for x, h in zip(pool, homes(pool)) if int(h) != 5][:m - 2]
    q = (a, b) + tuple(rest)
    assert len(set(q)) == m and int(homes([a])[0]) == int(homes([b])[0]) == 5
    voc = list(q)
    targets = [q, (b, a) + q[2:], (a,) + q[2:], (b,) + q[2:], (a, a) + q[2:], (b, b) + q[2:], (b, a), (a, b)]
    targets += [edited(g, q, e, voc) for e in (1, 2, 3) for _ in range(4)]
    return q, targets


def case_absent_items_on_taken_slots(m=24):
    """(c) targets that hold, where the query holds a token, an item ABSENT from the query whose probe starts at that token's slot: a
    lookup that trusts the slot without comparing the key takes it for a match and answers one less per such item.
    -> (query, targets, planted): planted[i] = the exact distance of target i (substitutions by items foreign to the query)"""
    pool = vocab("32k")[1000:1400]
    first = {}
    for x, h in zip(pool, homes(pool)):                            # query tokens with distinct home slots: each is found at its own
        first.setdefault(int(h), int(x))
    q = tuple(first.values())[:m]
    hq = homes(q)
    assert len(q) == m and len(set(int(h) for h in hq)) == m
    twin = [colliding(1, slot=int(h), exclude=q)[0] for h in hq]   # twin[i]: not in q, starts at q[i]'s slot
    assert not set(twin) & set(q) and (homes(twin) == hq).all()
    targets, planted = [], []
    for positions in ([0], [m - 1], [m // 2], [1, 2], [3, 9, 17], list(range(0, m, 2)), list(range(m))):
        t = list(q)
        for p in positions:
            t[p] = twin[p]
        targets.append(tuple(t))
        planted.append(len(positions))
    return q, targets, planted


def case_duplicates_in_the_second_word():
    """(d) a query of 64 tokens, distinct but for two: z sits at rows 5, 40 and 50 (its mask has bits in both words, two of its three
    lanes are at or above 32) and y at rows 45 and 60 (every lane that holds it is at or above 32: its mask lives in the second word)"""
    base = [int(x) for x in vocab("32k")[2000:2064]]
    z, y = base[5], base[45]
    base[40] = base[50] = z
    base[60] = y
    q = tuple(base)
    assert len(set(q)) == 61 and [i for i, x in enumerate(q) if x == z] == [5, 40, 50] and [i for i, x in enumerate(q) if x == y] == [45, 60]
    g = Dg.rng(77104)
    cut = lambda *rows: tuple(x for i, x in enumerate(q) if i not in rows)   # noqa: E731
    targets = [q, cut(5), cut(40), cut(50), cut(40, 50), cut(5, 40, 50), cut(45), cut(60), cut(45, 60), q[32:], q[:32], q[36:64], (z,) * 3,
               (z,) * 64, (y,) * 2, q[:45] + (q[60],) + q[46:60] + (q[45],),
               q[:40] + (q[41], q[40]) + q[42:]]
    targets += [edited(g, q, e, list(q)) for e in (1, 2, 4) for _ in range(4)]
    return q, targets


# ---------------------------------------------------------------- the reference
def _as_bytes(queries, targets):
    """the sequences of a batch with at most 256 distinct values as byte strings under one injective map, else None"""
    vals = {}
    for s in list(queries) + list(targets):
        for v in s:
            vals.setdefault(v, len(vals))
            if len(vals) > 256:
                return None
    return [bytes(vals[v] for v in s) for s in queries], [bytes(vals[v] for v in s) for s in targets]


_memo = {}


def dists(queries, targets, k, costs):
    """the C oracle over EVERY pair -> (nq, nt) uint32, NONE where it answers None; computed once per distinct batch"""
    queries, targets = [tuple(q) for q in queries], [tuple(t) for t in targets]
    key = (tuple(queries), tuple(targets), k, tuple(costs))
    if key in _memo:
        return _memo[key]
    nq, nt = len(queries), len(targets)
    if nq == 0 or nt == 0:
        out = np.zeros((nq, nt), np.uint32)
    else:
        mapped = _as_bytes(queries, targets)
        if mapped is not None:
            a = [q for q in mapped[0] for _ in targets]
            b = list(mapped[1]) * nq
        else:
            a, b = [], []
            for q in queries:
                for t in targets:
                    ca, cb = R.codes(q, t)
                    a.append(ca)
                    b.append(cb)
        out = O.levenshtein_k_batch(O.csr_from_list(a), O.csr_from_list(b), k, costs).reshape(nq, nt)
    _memo[key] = out
    return out


def join(queries, targets, k, costs, upper=False):
    """-> (sorted hits [(q, t, d)], nearest words, per-query counts)"""
    d = dists(queries, targets, k, costs)
    hits, nearest, per_query = [], [], []
    for q in range(len(queries)):
        row = [(q, t, int(d[q, t])) for t in range(len(targets)) if d[q, t] != NONE and (not upper or t > q)]
        hits += row
        nearest.append(min((x << 32 | t) for _, t, x in row) if row else ALL_ONES)
        per_query.append(len(row))
    return hits, nearest, per_query
