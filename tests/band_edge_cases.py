"""Pairs whose cheapest script runs along the band's outermost diagonals (pure numpy; tests/test_band_edge_cpu.py, tests/test_gpu_band_edge.py).

Every k-bounded route keeps the diagonals [min(0, d) - t, max(0, d) + t], t = (unit_k - |d|) / 2, d = len(b) - len(a) (lev_plan.h), half
of the reference's band, and each kernel restates that rule in its own geometry.  A pair notices a lost diagonal only when its cheapest
script HOLDS that diagonal, so the pairs here are staircases: a = M0 P M1 M2, b = M0 M1' Q M2 over random text.  Deleting P takes the
path |P| diagonals down, it stays there for all of M1 and comes back up over Q; with the sides exchanged it goes up first.  |P| + |Q| is
the largest number of gap items k pays for (an edge pair, distance = the constructed cost) and that plus 2 (None at k).  M1' is M1 with
an optional foreign byte and an optional adjacent swap: a substitution and a transposition ON the edge diagonal."""
import collections
import functools

import numpy as np

import datagen as Dg

LEV, RDAM = (1, 1, 0, None), (1, 1, 0, 1)
PRINT = np.arange(33, 127, dtype=np.uint8)
ACGT = np.frombuffer(b"ACGT", np.uint8)
FOREIGN = 0x20                                                     # a byte outside both alphabets
_ADVANCE = {"Match": (1, 1), "Mismatch": (1, 1), "Transpose": (2, 2), "AGap": (0, 1), "BGap": (1, 0)}     # edit -> (rows i, columns j)

# cls: "edge" | "plus2" | "unrelated" | "identical"; side: "low" (the deletion first) | "high"; cost: the constructed script's (None: no claim)
Row = collections.namedtuple("Row", "cls side m0 m2 p q sub swap cost")
Family = collections.namedtuple("Family", "a b rows la lb k costs")


def excursion(script):
    """(lowest, highest) diagonal j - i that an oracle script [(name, count)] visits, the start (0) included"""
    i = j = lo = hi = 0
    for name, count in script:
        di, dj = _ADVANCE[name]
        i += di * count
        j += dj * count
        lo, hi = min(lo, j - i), max(hi, j - i)
    return lo, hi


def edge_diagonals(script):
    """the diagonal j - i each edit of a script STARTS on: [(name, count, diagonal)]"""
    i = j = 0
    out = []
    for name, count in script:
        out.append((name, count, j - i))
        di, dj = _ADVANCE[name]
        i += di * count
        j += dj * count
    return out


def _text(g, n, alphabet):
    return g.choice(alphabet, n).astype(np.uint8) if n else np.zeros(0, np.uint8)


def stair(g, la, lb, p, q, m0, m2, delete_first, alphabet, sub=0, swap=False):
    """a = M0 P M1 M2, b = M0 M1' Q M2 (delete_first), or the sides exchanged: a = M0 M1' Q M2, b = M0 P M1 M2 -- len(a) = la and
    len(b) = lb either way.  M1' = M1 with `sub` foreign bytes (a third of the way in) and, for `swap`, one adjacent swap of unequal
    neighbours in its middle.  -> (a, b) bytes, or None when the lengths do not work out or |M1| < 8"""
    lx, ly = (la, lb) if delete_first else (lb, la)                # x = M0 P M1 M2, y = M0 M1' Q M2
    m1 = lx - m0 - p - m2
    if p < 0 or q < 0 or m1 < 8 or m0 + m1 + q + m2 != ly:
        return None
    M0, P, M1, Q, M2 = (_text(g, n, alphabet) for n in (m0, p, m1, q, m2))
    M1e = M1.copy()
    for s in range(sub):
        M1e[m1 // 3 + 2 * s] = FOREIGN
    if swap:
        at = m1 // 2
        while at + 1 < m1 and M1e[at] == M1e[at + 1]:
            at += 1
        if at + 1 >= m1:
            return None
        M1e[at], M1e[at + 1] = M1e[at + 1], M1e[at]
    x, y = np.concatenate([M0, P, M1, M2]).tobytes(), np.concatenate([M0, M1e, Q, M2]).tobytes()
    return (x, y) if delete_first else (y, x)


def afforded_gaps(k, costs, diff, sub=0, swap=False):
    """the most gap items p + q that k pays for in two runs beside `sub` substitutions and the swap, of the parity of diff = |len
    difference|: 2 sg + (p + q) gc + sub mc + swap tc <= k.  None: not even the length difference"""
    mc, gc, sg, tc = costs
    rest = k - 2 * sg - sub * mc - (tc if swap else 0)
    if rest < 0:
        return None
    gaps = rest // gc
    gaps -= (gaps - diff) & 1
    return gaps if gaps >= diff else None


def edge_t(k, costs, diff):
    """t': the largest excursion beyond [min(0, d), max(0, d)] that k affords -- 2 sg + (2 t' + |d|) gc <= k"""
    gaps = afforded_gaps(k, costs, diff)
    return None if gaps is None else (gaps - diff) // 2


def script_cost(p, q, sub, swap, costs):
    mc, gc, sg, tc = costs
    return ((sg + p * gc) if p else 0) + ((sg + q * gc) if q else 0) + sub * mc + (tc if swap else 0)


def placements(la, lb):
    """(m0, m2): the excursion from row 0, into the last column, across the 64- and 128-byte fetch boundaries, and in mid-string"""
    quarter = min(la, lb) // 4
    return [(0, 0), (1, 0), (0, 1), (quarter, 0), (0, quarter), (quarter, quarter), (63, 0), (64, 1)]


@functools.lru_cache(maxsize=None)
def family(la, lb, k, costs, alphabet="print", seed=0, m0s=None):
    """the staircase pairs of lengths la / lb for threshold k under `costs`: every placement, both sides, p + q = the most k pays for and
    that plus 2, (sub, swap) in {(0, F), (1, F), (0, T)} (the swap only with a transposition cost), then 20 unrelated and 20 identical
    pairs.  m0s: further values of m0 (with m2 = 0 and m2 = a quarter).  -> Family(a, b, rows, ...): lists of bytes and one Row per pair"""
    alpha = PRINT if alphabet == "print" else ACGT
    g = Dg.rng(0xED6E0000 + seed)
    d = lb - la
    a, b, rows = [], [], []
    places = placements(la, lb) + [(m, m2) for m in (m0s or ()) for m2 in (0, min(la, lb) // 4)]
    for m0, m2 in places:
        for low in (True, False):
            for sub, swap in ((0, False), (1, False)) + (((0, True),) if costs[3] is not None else ()):
                gaps = afforded_gaps(k, costs, abs(d), sub, swap)
                if gaps is None:
                    continue
                for extra in (0, 1):
                    t = (gaps - abs(d)) // 2 + extra
                    p = t + (max(0, -d) if low else max(0, d))     # the first run: down to min(0, d) - t, or up to max(0, d) + t
                    q = p + d if low else p - d
                    pair = stair(g, la, lb, p, q, m0, m2, low, alpha, sub, swap)
                    if pair is None:
                        continue
                    a.append(pair[0]); b.append(pair[1])
                    rows.append(Row("plus2" if extra else "edge", "low" if low else "high", m0, m2, p, q, sub, swap, script_cost(p, q, sub, swap, costs)))
    for i in range(40):
        x = _text(g, la, alpha).tobytes()
        same = i >= 20 and la == lb
        a.append(x); b.append(x if same else _text(g, lb, alpha).tobytes())
        rows.append(Row("identical" if same else "unrelated", "", 0, 0, 0, 0, 0, False, 0 if same else None))
    return Family(a, b, rows, la, lb, k, costs)


def plain_cost(fam):
    """the constructed cost of the family's edge pairs without a planted byte or swap"""
    return max(r.cost for r in fam.rows if r.cls == "edge" and not r.sub and not r.swap)


def ks(fam):
    """the k the family was built for, k - 1 and k + 1, and (weighted costs: k - 1 may still pay for the staircase) one below its cost"""
    return sorted({fam.k - 1, fam.k, fam.k + 1, plain_cost(fam) - 1})


def tiled(fam, n):
    """the family repeated to n pairs (np.tile and a remainder) -> ((n, la), (n, lb)) uint8 arrays and, per pair, its row in the family"""
    m = len(fam.a)
    idx = np.resize(np.arange(m), n) if n >= m else np.arange(n) * m // n      # (fewer than the family: evenly spread over its classes)
    arr = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)      # noqa: E731
    return np.ascontiguousarray(arr(fam.a)[idx]), np.ascontiguousarray(arr(fam.b)[idx]), idx


def arrays(fam):
    arr = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)      # noqa: E731
    return arr(fam.a).copy(), arr(fam.b).copy()


# ---- the families of the GPU cases (tests/test_gpu_band_edge.py), by name: (la, lb, k, costs, alphabet, seed, m0s); the CPU file checks
# every one of them on the oracle alone
W1, W2, W3, U3, LEV2 = (2, 3, 1, None), (2, 2, 1, 3), (100, 90, 3, 150), (3, 3, 0, 3), (2, 2, 0, None)
TAB_SHAPES = [(129, 129, 32, LEV), (160, 160, 32, LEV), (256, 256, 32, LEV), (257, 257, 32, LEV), (288, 256, 32, LEV), (256, 288, 32, LEV),
              (250, 256, 32, LEV), (256, 250, 32, LEV), (256, 224, 32, LEV),
              (256, 256, 24, LEV), (256, 256, 25, LEV), (256, 256, 31, LEV), (256, 256, 64, LEV2)]       # = tab_cases.SHAPES (asserted by the CPU file)
DP_LAYOUTS = [(2, 0), (4, 0), (6, 0), (8, 3), (10, 2), (12, 0), (16, 4), (18, 1), (22, 3), (24, 0), (34, 2), (66, 1), (8, 9), (2, 40), (56, 0)]


def dp_layout_k(force_D, force_L):
    return min(32, max(0, (force_D * (force_L if force_L else 64) - 2) // 2))


def _families():
    reg = {}

    def add(la, lb, k, costs, alphabet="print", m0s=None):
        name = "%d_%d-k%d-%s%s" % (la, lb, k, "_".join(str(c) for c in costs), "" if alphabet == "print" else "-acgt")
        name += "-m0s" if m0s else ""
        if name in reg:
            return name
        # (the seed: the family's number, except where the oracle's script of a mid-string pair over ACGT leaves the staircase -- 56 bytes
        # of M1 against 40 gap items -- and the conditions of tests/test_band_edge_cpu.py asked for another)
        reg[name] = (la, lb, k, costs, alphabet, 106 if (alphabet, la, k) in (("acgt", 150, 40), ("acgt", 150, 41)) else len(reg), m0s)
        return name
    for la, lb, k, costs in TAB_SHAPES:
        add(la, lb, k, costs)
    for la, lb in ((256, 256), (300, 291)):
        add(la, lb, 30, RDAM)
    for la, lb in ((100, 97), (300, 291)):
        for k in (12, 20, 40):
            add(la, lb, k, LEV)
            add(la, lb, k, RDAM)
        add(la, lb, 32, RDAM)
    add(300, 291, 32, LEV)
    add(256, 256, 40, LEV)
    add(256, 256, 32, RDAM)
    for costs in (LEV, RDAM):
        add(24, 23, 6, costs)
        add(150, 150, 16, costs, "acgt")
        add(2600, 2500, 300, costs)
        add(256, 256, 30 if costs[3] else 32, costs, m0s=(15, 16, 17))
    add(150, 147, 20, W1)
    add(150, 147, 12, W2)
    add(150, 143, 700, W3)
    add(300, 291, 40, W1)
    add(256, 256, 40, W1)
    add(256, 256, 90, U3)
    add(256, 256, 92, U3)
    for D, L in DP_LAYOUTS:
        k = dp_layout_k(D, L)
        for costs in (LEV, RDAM, W2):
            if afforded_gaps(k, costs, 2) is not None:
                add(90, 88, k, costs)
    for lq in (150, 256):
        for k in (8, 16, 24, 32, 40, 41):
            for costs in (LEV, RDAM):
                add(lq, lq, k, costs, "acgt")
    return reg


FAMILIES = _families()


def named(name):
    return family(*FAMILIES[name])


def name_of(la, lb, k, costs, alphabet="print", m0s=False):
    name = "%d_%d-k%d-%s%s%s" % (la, lb, k, "_".join(str(c) for c in costs), "" if alphabet == "print" else "-acgt", "-m0s" if m0s else "")
    assert name in FAMILIES, name
    return name
