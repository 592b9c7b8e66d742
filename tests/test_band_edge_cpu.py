"""not-gpu: the band-edge families of tests/band_edge_cases.py.

a. Conditions, from the oracle alone, for every family a GPU case of tests/test_gpu_band_edge.py uses: the oracle's own scripts have
   the constructed cost and reach exactly min(0, d) - t' and max(0, d) + t' (t' the largest excursion k affords), from row 0, into the
   last column and in mid-string; the "plus 2" pairs are None at k and Some beyond; the planted transposition and the planted mismatch
   sit where they were put.  These are conditions, not measurements: a family that stops reaching either edge fails here.
b. The same families through the host emulation of the kernel bodies (tests/emu_lib.py, and the table form's emulation of
   tests/test_emu_lev_bits_tab.py), at the k each was built for and at k - 1 and k + 1, against the oracle."""
import functools

import numpy as np
import pytest

import band_edge_cases as C
import emu_lib as E
import oracle_lib as O

LEV, RDAM = C.LEV, C.RDAM
NONE = 0xFFFFFFFF


# ================================================================ the convention
def test_excursion_convention():
    """Match / Mismatch advance both indices, Transpose both by two, AGap advances j (up), BGap advances i (down)"""
    assert C.excursion([("Match", 3), ("BGap", 2), ("Mismatch", 1), ("AGap", 5), ("Transpose", 1)]) == (-2, 3)
    assert C.excursion([("AGap", 4), ("Match", 9), ("BGap", 6)]) == (-2, 4) and C.excursion([]) == (0, 0)
    assert C.edge_diagonals([("BGap", 2), ("Transpose", 1), ("AGap", 3), ("Mismatch", 1)]) == \
        [("BGap", 2, 0), ("Transpose", 1, -2), ("AGap", 3, -2), ("Mismatch", 1, 1)]


def test_stair_builds_what_it_says():
    g = C.Dg.rng(5)
    a, b = C.stair(g, 40, 38, 5, 3, 2, 4, True, C.PRINT, sub=1, swap=True)
    assert len(a) == 40 and len(b) == 38 and a[:2] == b[:2] and a[-4:] == b[-4:]
    m1, m1e = a[7:36], b[2:31]
    assert sum(x != y for x, y in zip(m1, m1e)) == 3 and m1e[len(m1) // 3] == C.FOREIGN
    a2, b2 = C.stair(g, 38, 40, 5, 3, 0, 0, False, C.ACGT)
    assert len(a2) == 38 and len(b2) == 40 and a2[:30] == b2[5:35]
    assert C.stair(g, 40, 38, 5, 4, 0, 0, True, C.PRINT) is None and C.stair(g, 20, 20, 7, 7, 3, 3, True, C.PRINT) is None
    assert C.TAB_SHAPES == __import__("tab_cases").SHAPES


# ================================================================ a. conditions
@functools.lru_cache(maxsize=None)
def scripts(name, k=None):
    """the oracle's (distance, script) of every pair of a family at its k (or another)"""
    fam = C.named(name)
    return [O.levenshtein_simd_k_with_opts(x, y, fam.k if k is None else k, True, fam.costs) for x, y in zip(fam.a, fam.b)]


def check_conditions(fam, at_k, beyond):
    """at_k / beyond: the oracle's (distance, script) per pair at the family's k and at the dearest plus-2 script's cost"""
    d = fam.lb - fam.la
    t = C.edge_t(fam.k, fam.costs, abs(d))
    assert t is not None, "k does not pay for the length difference"
    lo_edge, hi_edge = min(0, d) - t, max(0, d) + t
    exact = [i for i, r in enumerate(fam.rows) if r.cls == "edge" and at_k[i][0] == r.cost]
    low = [i for i in exact if fam.rows[i].side == "low" and C.excursion(at_k[i][1])[0] == lo_edge]
    high = [i for i in exact if fam.rows[i].side == "high" and C.excursion(at_k[i][1])[1] == hi_edge]
    assert len(low) >= 4 and len(high) >= 4, (len(low), len(high), lo_edge, hi_edge)
    for side in (low, high):
        assert any(fam.rows[i].m0 == 0 for i in side), "no edge pair starts at row 0"
        assert any(fam.rows[i].m2 == 0 for i in side), "no edge pair ends in the last column"
        assert any(fam.rows[i].m0 >= 2 and fam.rows[i].m2 >= 2 for i in side), "no edge pair in mid-string"
    plus2 = [i for i, r in enumerate(fam.rows) if r.cls == "plus2" and at_k[i][0] is None and beyond[i][0] is not None]
    assert len(plus2) >= 4, len(plus2)
    if any(r.swap and r.cls == "edge" for r in fam.rows):         # the family has them: k pays for the swap beside the length difference
        assert sum(1 for i in exact if any(n == "Transpose" for n, _ in at_k[i][1])) >= 2
    on_edge = [i for i in low + high if fam.rows[i].sub and
               any(n == "Mismatch" and dg == (lo_edge if fam.rows[i].side == "low" else hi_edge) for n, _, dg in C.edge_diagonals(at_k[i][1]))]
    if C.afforded_gaps(fam.k, fam.costs, abs(d), 1) == C.afforded_gaps(fam.k, fam.costs, abs(d)):    # the family has them: the byte is free
        assert len(on_edge) >= 2, len(on_edge)
    assert sum(1 for i, r in enumerate(fam.rows) if r.cls == "unrelated" and at_k[i][0] is None) >= 10
    if fam.la == fam.lb:
        assert sum(1 for i, r in enumerate(fam.rows) if r.cls == "identical" and at_k[i][0] == 0) == 20
    assert len(fam.a) <= 400
    return len(low), len(high), len(plus2), len(on_edge)


@pytest.mark.parametrize("name", sorted(C.FAMILIES))
def test_family_reaches_both_edges(name):
    """150 / 143 under (100, 90, 3, 150) at k = 700: unit_k = 7 = |d|, t' = t = 0 -- the single-run case.  Where sg > 0 a staircase
    pays two gap openings and the planner's bound counts one, so t' can be one below the planner's t: 300 / 291 under (2, 3, 1, None)
    at k = 40 (t = 2, t' = 1) and 90 / 88 under (2, 2, 1, 3) at k = 9 (t = 1, t' = 0) -- there the planner's outermost diagonal holds
    no script of cost <= k at all, and the family's edge is the outermost diagonal that can."""
    fam = C.named(name)
    d, (_, gc, sg, _) = abs(fam.lb - fam.la), fam.costs
    assert ((max(fam.k - sg, 0) // gc - d) // 2 != C.edge_t(fam.k, fam.costs, d)) == (name in ("300_291-k40-2_3_1_None", "90_88-k9-2_2_1_3"))
    big = max(r.cost for r in fam.rows if r.cls == "plus2")
    print(name, check_conditions(fam, scripts(name), scripts(name, big)))


def test_conditions_fail_when_the_staircase_is_halved():
    """the same check on a family built for HALF the k (p + q halved) and judged at the full k: no pair reaches either edge"""
    small = C.family(256, 256, 16, LEV, "print", 77)
    fam = small._replace(k=32)
    at_k = [O.levenshtein_simd_k_with_opts(x, y, 32, True, LEV) for x, y in zip(fam.a, fam.b)]
    with pytest.raises(AssertionError):
        check_conditions(fam, at_k, at_k)


# ================================================================ b. the emulated bodies
def want_of(fam, k):
    d = O.levenshtein_k_batch(O.csr_from_list(fam.a), O.csr_from_list(fam.b), k, fam.costs)
    return [None if int(x) == NONE else int(x) for x in d]


plain_cost, ks = C.plain_cost, C.ks


def _edges_flip(fam):
    """the edge pairs answer None just below their cost and Some at k"""
    lo, hi = want_of(fam, plain_cost(fam) - 1), want_of(fam, fam.k)
    assert sum(1 for i, r in enumerate(fam.rows) if r.cls == "edge" and lo[i] is None and hi[i] is not None) >= 8


def fam_of(la, lb, k, costs, alphabet="print", m0s=False):
    return C.named(C.name_of(la, lb, k, costs, alphabet, m0s))


BITS_CSR = [(100, 97, 12, 1, 0), (100, 97, 20, 1, 0), (300, 291, 12, 1, 0), (300, 291, 20, 1, 0), (100, 97, 40, 1, 0), (300, 291, 40, 1, 0),
            (100, 97, 20, 2, 8), (256, 256, 24, 2, 8), (300, 291, 20, 2, 9), (100, 97, 40, 2, 12), (300, 291, 40, 2, 12), (300, 291, 40, 2, 16),
            (100, 97, 40, 2, 0), (300, 291, 40, 2, 0)]


@pytest.mark.parametrize("la,lb,k,static,na,costs", [c + (costs,) for c in BITS_CSR for costs in (LEV, RDAM) if (c[0], c[2], costs) != (256, 24, RDAM)])
def test_emu_bits_sliding_and_static_windows(la, lb, k, static, na, costs):
    """lev_bits (CSR form) and lev_bits_fixed: the sliding window (static=1) and the static one (static=2) at NA 8, 9, 12, 16 and the
    planner's"""
    fam = fam_of(la, lb, k, costs)
    trans = costs[3] is not None
    for kk in ks(fam):
        if static == 2 and na and kk + 1 + (2 if trans else 0) > 4 * na - 3:
            continue
        got, plan = E.lev_bits(fam.a, fam.b, kk, trans, force_NA=na, static=static)
        assert plan["static"] == (static == 2) and not plan["s8"] and (not na or plan["NA"] == na), plan
        assert got == want_of(fam, kk), (kk, plan)
        got, plan = E.lev_bits_fixed(*C.arrays(fam), kk, trans, force_NA=na, static=static)
        assert got == want_of(fam, kk), ("fixed", kk, plan)
    _edges_flip(fam)


S8 = [s for s in C.TAB_SHAPES if s[3] == LEV] + [(256, 256, 30, RDAM), (300, 291, 30, RDAM), (300, 291, 32, LEV)]


@pytest.mark.parametrize("la,lb,k,costs", S8)
def test_emu_bits_stride8_window(la, lb, k, costs):
    """lev_bits static=3 (33 diagonals in 8 registers, the 33rd as match | carry), CSR form and the fixed-length LINE form"""
    fam = fam_of(la, lb, k, costs)
    trans = costs[3] is not None
    for kk in ks(fam):
        if kk + 1 + (2 if trans else 0) > 33:
            continue
        got, plan = E.lev_bits(fam.a, fam.b, kk, trans, static=3)
        assert plan["s8"], plan
        assert got == want_of(fam, kk), (kk, plan)
        got, plan = E.lev_bits_fixed(*C.arrays(fam), kk, trans, static=3)
        assert plan["s8"] and got == want_of(fam, kk), ("fixed", kk, plan)
    _edges_flip(fam)


@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_emu_bits_fixed_chunk_form_and_early_out(costs):
    """fixed-length batches of up to one line (the chunk form with wave-uniform predicates), and the early out on the LINE form"""
    trans = costs[3] is not None
    fam = fam_of(100, 97, 20, costs)
    E.bits_fixed_chunk(True)
    try:
        for kk in ks(fam):
            for static in (1, 2, 3):
                got, plan = E.lev_bits_fixed(*C.arrays(fam), kk, trans, static=static)
                assert got == want_of(fam, kk), (kk, static, plan)
    finally:
        E.bits_fixed_chunk(False)
    fam = fam_of(256, 256, 30 if trans else 32, costs)
    E.bits_set_tune(2)
    try:
        for kk in ks(fam):
            if kk + 1 + (2 if trans else 0) <= 33:
                got, plan = E.lev_bits_fixed(*C.arrays(fam), kk, trans)
                assert plan["s8"] and got == want_of(fam, kk), (kk, plan)
    finally:
        E.bits_set_tune(0)


@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_emu_bits_vline_form(costs):
    """the VLINE fetch form (whole lines per lane) on the CSR view of the stride-8 families"""
    trans = costs[3] is not None
    fam = fam_of(256, 256, 30 if trans else 32, costs)
    E.bits_vline(True)
    try:
        for kk in ks(fam):
            if kk + 1 + (2 if trans else 0) <= 33:
                got, plan = E.lev_bits(fam.a, fam.b, kk, trans, static=3)
                assert plan["s8"] and got == want_of(fam, kk), (kk, plan)
    finally:
        E.bits_vline(False)


@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_emu_two_pairs_per_lane(costs):
    fam = fam_of(24, 23, 6, costs)
    a, b, idx = C.tiled(fam, 2 * len(fam.a) + 65)                   # (an odd remainder: the last lane holds one pair)
    for kk in ks(fam):
        got, plan = E.lev_bits2(a, b, kk, costs[3] is not None)
        assert got is not None, "planner declined"
        want = want_of(fam, kk)
        assert got == [want[i] for i in idx], (kk, plan)
    _edges_flip(fam)


@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_emu_small_alphabet_bodies(costs):
    """lev_bitsq (2-bit codes) and lev_bitsqw (5-bit codes) over ACGT; the pairs with the planted foreign byte go to the caller's list"""
    fam = fam_of(150, 150, 16, costs, "acgt")
    a, b = C.arrays(fam)
    foreign = [i for i, r in enumerate(fam.rows) if r.sub]
    assert len(foreign) >= 8
    for kk in ks(fam):
        want = want_of(fam, kk)
        for body in (E.lev_bitsq, E.lev_bitsqw):
            got, bad = body(a, b, kk, b"ACGT", costs[3] is not None)
            assert got is not None, "declined"
            assert bad == foreign
            assert got == ["untouched" if r.sub else want[i] for i, r in enumerate(fam.rows)], (kk, body.__name__)
    _edges_flip(fam)


@pytest.mark.parametrize("la,lb,k", [(256, 256, 32), (300, 291, 20)])
@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_emu_lone_pair(la, lb, k, costs):
    k = 30 if (k == 32 and costs == RDAM) else k
    fam = fam_of(la, lb, k, costs)
    for kk in ks(fam):
        want = want_of(fam, kk)
        got = [E.lev_one(x, y, kk, costs[3] is not None) for x, y in zip(fam.a, fam.b)]
        assert got == want, (kk, [i for i, (x, y) in enumerate(zip(got, want)) if x != y][:5])


@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_emu_row_blocked(costs):
    fam = fam_of(2600, 2500, 300, costs)
    pick = [i for i, r in enumerate(fam.rows) if r.cls in ("edge", "plus2")][::3] + [len(fam.rows) - 1, len(fam.rows) - 25]
    a, b = [fam.a[i] for i in pick], [fam.b[i] for i in pick]
    for kk in ks(fam):
        want = want_of(fam, kk)
        for nwl in (1, 2):
            assert E.lev_widebits(a, b, kk, costs[3] is not None, nwl=nwl) == [want[i] for i in pick], (kk, nwl)
    _edges_flip(fam)


@pytest.mark.parametrize("force_D,force_L", C.DP_LAYOUTS)
def test_emu_dp_band_lane_layouts(force_D, force_L):
    """lev_band under every (force_D, force_L) of test_dpp_and_layouts: the band's outermost diagonals sit on the lanes where wave_shr /
    wave_shl meet the neighbouring pair, so low-edge and high-edge pairs alternate"""
    k = C.dp_layout_k(force_D, force_L)
    for costs in (LEV, RDAM, C.W2):
        if C.afforded_gaps(k, costs, 2) is None:
            continue
        fam = fam_of(90, 88, k, costs)
        order = alternate(fam)
        a, b = [fam.a[i] for i in order], [fam.b[i] for i in order]
        for kk in ks(fam):
            if kk < 0 or (kk > k and force_D * (force_L or 64) < (max(kk - costs[2], 0) // costs[1]) + 2):
                continue
            want = want_of(fam, kk)
            got, plan = E.lev_band(a, b, kk, costs, force_D=force_D, force_L=force_L)
            assert plan["D"] == force_D
            assert got == [want[i] for i in order], (kk, costs, plan)


def alternate(fam):
    """the family's pairs with low-edge and high-edge pairs alternating (neighbouring pairs of a wavefront sit on each other's lane
    edge), the rest behind them"""
    low = [i for i, r in enumerate(fam.rows) if r.side == "low"]
    high = [i for i, r in enumerate(fam.rows) if r.side == "high"]
    rest = [i for i, r in enumerate(fam.rows) if not r.side]
    order = [i for pair in zip(low, high) for i in pair]
    return order + [i for i in low + high if i not in set(order)] + rest


@pytest.mark.parametrize("la,lb,k,costs", [(150, 147, 20, C.W1), (150, 147, 12, C.W2), (150, 143, 700, C.W3), (300, 291, 40, C.W1)])
def test_emu_dp_band_cost_sets(la, lb, k, costs):
    """the weighted cost sets: score form, cost form, the select form of the transposition, and the LINE form of the fetch"""
    fam = fam_of(la, lb, k, costs)
    for kk in ks(fam):
        want = want_of(fam, kk)
        got, plan = E.lev_band(fam.a, fam.b, kk, costs)
        assert got == want, (kk, plan)
        assert E.lev_band(fam.a, fam.b, kk, costs, score=False)[0] == want, (kk, "cost form")
        if costs[3] is not None:
            assert E.lev_band(fam.a, fam.b, kk, costs, force_trans_select=True)[0] == want, (kk, "select form")
        if E.lev_band_score_applies(costs):
            E.band_line(True)
            try:
                assert E.lev_band(fam.a, fam.b, kk, costs)[0] == want, (kk, "line form")
            finally:
                E.band_line(False)
    _edges_flip(fam)


@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("m0s", [False, True])
def test_emu_checkpoint_traceback(costs, m0s):
    """lev_bits_trace, edit for edit: tiles of 16 columns (excursions that begin at columns 15, 16, 17 under m0s), CSR and fixed, plain
    and packed"""
    trans = costs[3] is not None
    fam = fam_of(256, 256, 30 if trans else 32, costs, m0s=m0s)
    name = C.name_of(256, 256, fam.k, costs, m0s=m0s)
    for kk in (fam.k - 1, fam.k):
        want = scripts(name, kk)
        dists = [w[0] for w in want]
        for fixed in (False, True):
            got = E.lev_bits_trace(fam.a, fam.b, kk, dists, trans, 16, fixed)
            assert got == [w[1] for w in want], (kk, fixed)
        cap = 2 * kk + 1
        got = E.lev_bits_trace(fam.a, fam.b, kk, dists, trans, 16, True, packed=cap)
        for g, w in zip(got, want):
            assert (g is None and w[0] is None) or (g[0] == len(w[1]) and g[1] == w[1][-cap:]), (kk, g, w)


@pytest.mark.parametrize("la,lb,k,costs", C.TAB_SHAPES)
def test_emu_table_form(la, lb, k, costs):
    """the table form (the headline kernel) on a family built FOR each shape of tab_cases.SHAPES, at 65 pairs and at 209"""
    import test_emu_lev_bits_tab as Tab
    fam = fam_of(la, lb, k, costs)
    for n in (65, 209):
        a, b, idx = C.tiled(fam, n)
        for kk in (k - 1, k, k + 1):
            if not 25 <= kk // costs[0] + 1 <= 33:
                continue
            want = np.array([NONE if w is None else w for w in want_of(fam, kk)], np.uint32)[idx]
            got = Tab.emu(a, b, kk, costs)
            assert np.array_equal(got, want), (n, kk, np.flatnonzero(got != want)[:10])
