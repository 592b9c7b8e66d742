"""-m gpu: every k-bounded route on pairs whose cheapest script runs along the band's outermost diagonals (tests/band_edge_cases.py).

Every route computes the diagonals [min(0, d) - t, max(0, d) + t] only (lev_plan.h) and restates that rule in its own geometry; a lost
diagonal shows on the pairs that HOLD it and on no others.  One case per route -- the routes, their switches and their kernel names are
those of tests/test_gpu_layouts.py -- each on a family built for its shape, costs and k (tests/test_band_edge_cpu.py checks on the
oracle alone that every family reaches both edges), at that k, at k - 1 and k + 1 and one below the staircase's cost.  Every case asserts
the route and answers equal to the oracle's, bit for bit; the traceback cases assert the scripts edit for edit.

Where the issue's table and the code disagree the code wins: k + 1 often leaves a route's domain (k = 33 leaves the stride-8 window and
the table form), so the expected kernel name is a function of the k actually run.

Mutation check (done once, by hand, on scratch copies of the library; answers-only edits -- no address, guard, loop bound or launch
dimension changed; 166 cases in this file; each edit reverted afterwards):
  * DP band kernel (lev_band_body.h): for pairs with t >= 1 the cells of the lowest diagonal forced to "unreachable" after every phase.
    (Not through the planner: the band offset o also places the ring reads, so moving it would move addresses.)  27 cases fail: all 15 of
    test_dp_band_every_lane_layout, 5 of test_dp_band_kernel, the cost form's child, 6 of test_trace_record_routes.  The older
    tests/test_gpu_lev_batch.py goes red as well (16 of 48: all_costs_ragged, band_line_form_fixed_length, dpp_and_layouts, ...).
  * bit window (lev_bits_body.h column(): sliding and static windows): for pairs with t >= 1 the match bit of the window's lowest diagonal
    cleared.  66 cases fail: sliding_window 8 of 8, static_window_and_forced_na 9 of 9, and every case whose k + 1 or k - 1 leaves the
    stride-8 window for a static or sliding one (stride8 21, table_form 13, csr 8, small alphabets' fallback 4, two_pairs 2, times_g 1).
    tests/test_gpu_lev_bits.py, test_gpu_lev_bits_core.py and test_gpu_lev_batch.py: 23 of 105 fail too (test_gpu_lev_bits_tab.py not
    run: its kernel does not go through column()).  Neither edit is one the older suite was blind to; what is new is WHERE they
    are seen: per route, per lane layout, on both sides, with the kernel name asserted.
  * cross window (lev_cross_win_body.h), top row of a window that has slid never matches: 8 cases fail, test_cross_window_kernel at
    k = 16 and k = 32 (all 8 of them) and at no other k -- the window's top row 32 lo + 1 is the band's row j0 + 1 - k only when
    k = 0 mod 16 (pieces of 16 columns); at k = 8, 24, 40 the window has 8 spare rows and at 41 it is the whole column.  The issue's
    k list {8, 24, 40, 41} could not see this edit: k = 16 and 32 are the class that was missing, added.  The single-run targets with
    the run at the FRONT are the pairs that catch it.  tests/test_gpu_cross_opts.py: 1 of 24 fails (the helpers' k = 0 call).
  * cross window, a pair whose lengths differ by exactly k answers None: all 24 cases of test_cross_window_kernel fail (the single-run
    targets); tests/test_gpu_cross_opts.py: 5 of 24."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import band_edge_cases as C
import oracle_lib as O

pytestmark = pytest.mark.gpu

LEV, RDAM, W1, W2, W3 = C.LEV, C.RDAM, C.W1, C.W2, C.W3
NONE = 0xFFFFFFFF
TAB = "lev_bits_tab_kernel"


def _mods():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    return torch, T, B


def _route():
    _, T, _ = _mods()
    return T.last_launch_info()["kernel"], T.last_kernel_name()


@functools.lru_cache(maxsize=None)
def want(name, k):
    """the oracle's answers for the distinct rows of a family"""
    fam = C.named(name)
    return O.levenshtein_k_batch(O.csr_from_list(fam.a), O.csr_from_list(fam.b), k, fam.costs)


@functools.lru_cache(maxsize=None)
def scripts(name, k):
    fam = C.named(name)
    return [O.levenshtein_simd_k_with_opts(x, y, k, True, fam.costs) for x, y in zip(fam.a, fam.b)]


def strings(B, fam, idx, csr):
    """the family's rows idx as two Strings: CSR, or fixed-length (strided)"""
    if csr:
        return B.Strings.from_list([fam.a[i] for i in idx]), B.Strings.from_list([fam.b[i] for i in idx])
    a, b = C.arrays(fam)
    return B.Strings.from_fixed(np.ascontiguousarray(a[idx])), B.Strings.from_fixed(np.ascontiguousarray(b[idx]))


def index(fam, n=None, order=None):
    m = len(fam.a)
    base = np.arange(m) if order is None else np.array(order)
    if n is None:
        return base
    return base[np.resize(np.arange(m), n)] if n >= m else base[np.arange(n) * m // n]


def sweep(name, expect, n=None, csr=False, alphabet=None, order=None, only=None):
    """the family at every k of C.ks: answers equal to the oracle's, the route expect(k)(route); -> {k: answers}"""
    _, _, B = _mods()
    fam = C.named(name)
    idx = index(fam, n, order)
    sa, sb = strings(B, fam, idx, csr)
    out = {}
    for k in (C.ks(fam) if only is None else only):
        got = B.levenshtein_k_batch(sa, sb, k, fam.costs, alphabet=alphabet).cpu().numpy().view(np.uint32)
        route = _route()
        w = want(name, k)[idx]
        assert np.array_equal(got, w), (name, k, route, [(int(i), fam.rows[idx[i]], int(got[i]), int(w[i])) for i in np.flatnonzero(got != w)[:6]])
        assert expect(k)(route), (name, k, route)
        out[k] = got
    edge = np.array([fam.rows[i].cls == "edge" for i in idx])
    lo, hi = want(name, C.plain_cost(fam) - 1)[idx], want(name, fam.k)[idx]
    assert ((lo == NONE) & (hi != NONE) & edge).sum() >= 8, "the edge pairs answer None below their cost and Some at k"
    return out


def fam_name(la, lb, k, costs, alphabet="print", m0s=False):
    return C.name_of(la, lb, k, costs, alphabet, m0s)


def is_s8(k, costs):
    return 25 <= k + 1 + (2 if costs[3] else 0) <= 33


def bits_expect(costs, line, early=False):
    """the bit-parallel band kernel's name at unit threshold k: the stride-8 form for bands of 25..33 diagonals, else a window kernel"""
    t = "true" if costs[3] else "false"

    def at(k):
        if is_s8(k, costs):
            return lambda r: r == (3, "lev_bits_s8_kernel<%s, %s, %s>" % (t, "true" if line else "false", "true" if early and line else "false"))
        return lambda r: r[0] == 3 and r[1].startswith("lev_bits_line_kernel<" if line else "lev_bits_kernel<")
    return at


# ================================================================ the stride-8 window: chunk and LINE forms, early out
S8_SHAPES = [(129, 129, 32, LEV), (256, 256, 32, LEV), (288, 256, 32, LEV), (256, 288, 32, LEV), (250, 256, 32, LEV), (256, 250, 32, LEV),
             (256, 256, 30, RDAM), (300, 291, 30, RDAM), (256, 256, 24, LEV), (256, 256, 25, LEV), (256, 256, 31, LEV)]


@pytest.mark.parametrize("mode", ["default", "TA_NO_LATENCY_RULE", "TA_EARLY_OUT"])
@pytest.mark.parametrize("la,lb,k,costs", S8_SHAPES)
def test_stride8_chunk_and_line_forms(la, lb, k, costs, mode, monkeypatch):
    """fixed-length (LINE form: strings longer than one line) and CSR (chunk form).  default: 1,100 pairs (tiled) so that the throughput
    choice holds; TA_NO_LATENCY_RULE=1: the family as it is; TA_EARLY_OUT=1: the early-out instantiation of the LINE form"""
    if mode != "default":
        monkeypatch.setenv(mode, "1")
    if mode == "TA_EARLY_OUT":
        monkeypatch.setenv("TA_NO_LATENCY_RULE", "1")
    n = 1100 if mode == "default" else None
    name = fam_name(la, lb, k, costs)
    sweep(name, bits_expect(costs, True, mode == "TA_EARLY_OUT"), n=n)
    sweep(name, bits_expect(costs, False), n=n, csr=True)


# ================================================================ the table form (the headline kernel)
@pytest.mark.parametrize("n", [65, 209])
@pytest.mark.parametrize("la,lb,k,costs", C.TAB_SHAPES)
def test_table_form(la, lb, k, costs, n, monkeypatch):
    """TA_FORCE_TAB_FORM=1 on a family built FOR each shape of tab_cases.SHAPES (not cut from another); k / g outside 24..32 leaves the
    table form's domain and the answers are still the oracle's"""
    monkeypatch.setenv("TA_NO_LATENCY_RULE", "1")
    monkeypatch.setenv("TA_FORCE_TAB_FORM", "1")
    g = costs[0]
    sweep(fam_name(la, lb, k, costs), lambda kk: (lambda r: r[0] == 3 and (TAB in r[1]) == (25 <= kk // g + 1 <= 33)), n=n)


# ================================================================ sliding and static windows
@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("la,lb", [(100, 97), (300, 291)])
@pytest.mark.parametrize("k", [12, 20])
def test_sliding_window(la, lb, k, costs):
    line = la > 128
    sweep(fam_name(la, lb, k, costs), lambda kk: (lambda r: r[0] == 3 and r[1].startswith("lev_bits_line_kernel<" if line else "lev_bits_kernel<")
                                                  and r[1].endswith(", false>")), n=1100)


@pytest.mark.parametrize("costs,k", [(LEV, 40), (RDAM, 40), (RDAM, 32)])
@pytest.mark.parametrize("env", [{"TA_BITS_STATIC": "1"}, {"TA_BITS_STATIC": "2"}, {"TA_FORCE_NA": "12"}])
def test_static_window_and_forced_na(costs, k, env, monkeypatch):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    tail = ", %s>" % ("false" if env.get("TA_BITS_STATIC") == "1" else "true")
    for la, lb in ((100, 97), (300, 291)):
        kern = "lev_bits_line_kernel<" if la > 128 else "lev_bits_kernel<"
        sweep(fam_name(la, lb, k, costs), lambda kk: (lambda r: r[0] == 3 and r[1].startswith(kern) and r[1].endswith(tail)))


# ================================================================ CSR: one ragged batch of all the stride-8 families
@functools.lru_cache(maxsize=None)
def ragged_mix(costs):
    """the stride-8 families of one cost set as one ragged batch -> (a rows, b rows, the family's name and row per pair)"""
    names = [fam_name(la, lb, k, c) for la, lb, k, c in S8_SHAPES[:8] if c == costs and k == (30 if costs[3] else 32)]
    names += [fam_name(160, 160, 32, LEV), fam_name(257, 257, 32, LEV), fam_name(256, 224, 32, LEV)] if costs == LEV else []
    a, b, src = [], [], []
    for nm in names:
        fam = C.named(nm)
        a += fam.a; b += fam.b; src += [(nm, i) for i in range(len(fam.a))]
    return a, b, src


@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("n,switch", [(1100, None), (4500, None), (4500, "TA_NO_LENGTH_ORDER"), (4500, "TA_BITS_VLINE")])
def test_csr_chunk_form_length_ordered_and_vline(costs, n, switch, monkeypatch):
    """1,100 pairs: batch order; 4,500: a length-ordered subset list, the same in batch order, and the VLINE fetch form"""
    _, _, B = _mods()
    if switch:
        monkeypatch.setenv(switch, "1")
    a, b, src = ragged_mix(costs)
    pick = np.resize(np.random.default_rng(n).permutation(len(a)), n)
    sa, sb = B.Strings.from_list([a[i] for i in pick]), B.Strings.from_list([b[i] for i in pick])
    k0 = 30 if costs[3] else 32
    for k in (k0 - 1, k0, k0 + 1):
        got = B.levenshtein_k_batch(sa, sb, k, costs).cpu().numpy().view(np.uint32)
        route = _route()
        w = np.array([want(src[i][0], k)[src[i][1]] for i in pick], np.uint32)
        assert np.array_equal(got, w), (k, route, [src[pick[i]] for i in np.flatnonzero(got != w)[:6]])
        kern = ("lev_bits_s8v_kernel<" if switch == "TA_BITS_VLINE" else "lev_bits_s8_kernel<") if is_s8(k, costs) else "lev_bits_kernel<"
        assert route[0] == 3 and route[1].startswith(kern), (k, route)


# ================================================================ two pairs per lane, small alphabets, the lone pair, the row-blocked kernel
@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_two_pairs_per_lane(costs, monkeypatch):
    _, T, _ = _mods()
    name = fam_name(24, 23, 6, costs)
    two = sweep(name, lambda k: (lambda r: r[0] == 3 and r[1].startswith("lev_bits2_kernel<") and T.last_launch_info()["pairs_per_wave"] == 128), n=262144 + 65)
    monkeypatch.setenv("TA_NO_BITS2", "1")
    one = sweep(name, lambda k: (lambda r: r[0] == 3 and r[1].startswith("lev_bits_kernel<") and T.last_launch_info()["pairs_per_wave"] == 64), n=262144 + 65)
    assert all(np.array_equal(two[k], one[k]) for k in two)


@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("wide", [False, True])
def test_small_alphabet_kernels(costs, wide, monkeypatch):
    """alphabet=b"ACGT": the 2-bit-code kernel, the 5-bit-code kernel under TA_BITSQ_WIDE=1; the pairs with the planted foreign byte
    (0x20) take the general kernel's list"""
    if wide:
        monkeypatch.setenv("TA_BITSQ_WIDE", "1")
    kern = "lev_bitsqw_kernel<" if wide else "lev_bitsq_kernel<"
    sweep(fam_name(150, 150, 16, costs, "acgt"), lambda k: (lambda r: r[0] == 7 and r[1].startswith(kern)), n=16385, alphabet=b"ACGT")


@pytest.mark.parametrize("la,lb,k,costs", [(256, 256, 32, LEV), (300, 291, 20, LEV), (256, 256, 30, RDAM), (300, 291, 20, RDAM)])
def test_lone_pair(la, lb, k, costs):
    """n = 1, one call per pair (64 pairs of the family, spread over its classes)"""
    _, _, B = _mods()
    name = fam_name(la, lb, k, costs)
    fam = C.named(name)
    for i in index(fam, 64):
        sa, sb = B.Strings.from_list([fam.a[i]]), B.Strings.from_list([fam.b[i]])
        for kk in C.ks(fam):
            got = int(B.levenshtein_k_batch(sa, sb, kk, costs).cpu().numpy().view(np.uint32)[0])
            route = _route()
            assert got == int(want(name, kk)[i]), (i, kk, fam.rows[i], got)
            assert route[0] == 6 and route[1].startswith("lev_one_kernel<"), route


@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("rows", [32, 64])
def test_row_blocked_kernel(costs, rows, monkeypatch):
    _, T, _ = _mods()
    monkeypatch.setenv("TA_FORCE_WIDEBITS", str(rows))
    sweep(fam_name(2600, 2500, 300, costs), lambda k: (lambda r: r[0] == 4 and T.last_launch_info()["diags_per_lane"] == rows), csr=True)


# ================================================================ the DP band kernel
WEIGHTED = ((W1, 20, 147), (W2, 12, 147), (W3, 700, 143))


def alternate(fam):
    """low-edge and high-edge pairs in turn (the 64 / L pairs of a wavefront sit on each other's lane edge), the rest behind them"""
    low = [i for i, r in enumerate(fam.rows) if r.side == "low"]
    high = [i for i, r in enumerate(fam.rows) if r.side == "high"]
    order = [i for pair in zip(low, high) for i in pair]
    return order + [i for i in range(len(fam.rows)) if i not in set(order)]


@pytest.mark.parametrize("costs,k,lb,env", [w + (e,) for w in WEIGHTED for e in ({}, {"TA_BAND_NO_LINE": "1"}, {"TA_FORCE_TRANS_SELECT": "1"})
                                            if w[0][3] is not None or "TA_FORCE_TRANS_SELECT" not in e])
def test_dp_band_kernel(costs, k, lb, env, monkeypatch):
    """score-line, score-chunk (TA_BAND_NO_LINE=1) and select (TA_FORCE_TRANS_SELECT=1: cost form) forms, fixed-length and CSR"""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    name = fam_name(150, lb, k, costs)
    if env.get("TA_FORCE_TRANS_SELECT"):
        fixed = ragged = lambda kk: (lambda r: r[0] == 1 and r[1].startswith("lev_band_kernel<") and ", 2, " in r[1])       # noqa: E731
    else:
        fixed = lambda kk: (lambda r: r[0] == 1 and r[1].startswith("lev_band_score_kernel<" if env else "lev_band_score_line_kernel<"))   # noqa: E731
        ragged = lambda kk: (lambda r: r[0] == 1 and r[1].startswith("lev_band_score_kernel<"))                               # noqa: E731
    order = alternate(C.named(name))
    sweep(name, fixed, n=1100, order=order)
    sweep(name, ragged, n=1100, order=order, csr=True)


def _cost_form_child():
    """runs in a fresh process started with TA_NO_SCORE_FORM=1 (the switch is read once, at the process's first DP band launch)"""
    for costs, k, lb in WEIGHTED:
        name = fam_name(150, lb, k, costs)
        sweep(name, lambda kk: (lambda r: r[0] == 1 and r[1].startswith("lev_band_kernel<")), n=1100, order=alternate(C.named(name)))
    print("cost form ok")


def test_dp_band_cost_form_in_a_child_process():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, TA_NO_SCORE_FORM="1", TA_TUNING="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_band_edge as G; G._cost_form_child()" % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "cost form ok" in r.stdout, r.stderr[-3000:]


@pytest.mark.parametrize("force_D,force_L", C.DP_LAYOUTS)
def test_dp_band_every_lane_layout(force_D, force_L, monkeypatch):
    """every (TA_FORCE_D, TA_FORCE_L) of test_dpp_and_layouts, k = min(32, (cap - 2) / 2) at 90 / 88: the band's outermost diagonals sit on
    the lanes where wave_shr / wave_shl meet the neighbouring pair of the wavefront (a k + 1 the forced layout cannot hold is left out)"""
    _, T, _ = _mods()
    monkeypatch.setenv("TA_FORCE_D", str(force_D))
    monkeypatch.setenv("TA_FORCE_L", str(force_L))
    k = C.dp_layout_k(force_D, force_L)
    cap = force_D * (force_L if force_L else 64)
    for costs in (LEV, RDAM, W2):
        if C.afforded_gaps(k, costs, 2) is None:
            continue
        name = fam_name(90, 88, k, costs)
        fam = C.named(name)
        fits = [kk for kk in C.ks(fam) if kk >= 0 and max(kk - costs[2], 0) // costs[1] + 2 <= cap]
        sweep(name, lambda kk: (lambda r: r[0] == 1 and T.last_launch_info()["diags_per_lane"] == force_D), n=1100, order=alternate(fam), csr=True, only=fits)


def test_wide_dp_kernel(monkeypatch):
    monkeypatch.setenv("TA_FORCE_WIDE", "1")
    sweep(fam_name(300, 291, 40, W1), lambda k: (lambda r: r[0] == 2), csr=True)


@pytest.mark.parametrize("k", [90, 92])
def test_unit_costs_times_g(k):
    """(3, 3, 0, 3): the unit-cost kernels with k / 3 and the answers times 3"""
    sweep(fam_name(256, 256, k, C.U3), lambda kk: bits_expect(RDAM, True)(kk // 3), n=1100)


# ================================================================ tracebacks
CKPT = lambda r: r[0] == 8 and "lev_bits_trace_kernel" in r[1]                                 # noqa: E731
RECORD = lambda r: r[0] == 1 and r[1].startswith("lev_band_trace_kernel<")                     # noqa: E731


def trace_case(name, k, expect, csr, packed):
    torch, _, B = _mods()
    fam = C.named(name)
    sa, sb = strings(B, fam, np.arange(len(fam.a)), csr)
    cap = 2 * k + 1
    if packed:
        out, words, ne = B.levenshtein_trace_batch_packed(sa, sb, k, fam.costs, cap=cap)
        got = B.packed_to_lists(words, ne)
    else:
        out, edits, ne = B.levenshtein_trace_batch(sa, sb, k, fam.costs, cap=cap)
        got = B.edits_to_lists(edits, ne)
    route = _route()
    assert expect(route), (name, k, route)
    d = out.cpu().numpy().view(np.uint32)
    some = 0
    for i, (wd, we) in enumerate(scripts(name, k)):
        if wd is None:
            assert d[i] == NONE and got[i] == [], (i, fam.rows[i])
        else:
            assert d[i] == wd and got[i] == we, (i, fam.rows[i], got[i], we)
            some += 1
    return some


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("csr", [False, True])
@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_trace_checkpoint_route(costs, csr, packed, monkeypatch):
    """scripts edit for edit on the checkpoint route (tiles of 16 columns): the family and its twin whose excursions begin at columns 15,
    16, 17; then the same with the strings fetched 128 columns at a time (TA_TRACE_STILE=128)"""
    k = 30 if costs[3] else 32
    for stile in (None, "128"):
        if stile:
            monkeypatch.setenv("TA_TRACE_STILE", stile)
        for m0s in (False, True):
            name = fam_name(256, 256, k, costs, m0s=m0s)
            assert trace_case(name, k, CKPT, csr, packed) > trace_case(name, k - 1, CKPT, csr, packed) >= 20


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("la,lb,k,costs", [(256, 256, 32, RDAM), (256, 256, 40, LEV), (256, 256, 40, W1)])
def test_trace_record_routes(la, lb, k, costs, packed):
    """bands beyond the checkpoint route's 33 diagonals, and weighted costs: the DP band kernel's records and a walk"""
    name = fam_name(la, lb, k, costs)
    fam = C.named(name)
    for kk in (C.plain_cost(fam) - 1, k):
        assert trace_case(name, kk, RECORD, True, packed) >= 20


# ================================================================ the exp rounds, tokens
@pytest.mark.parametrize("costs", [LEV, W1])
def test_exp_batch(costs):
    """the 256 / 256 and 300 / 291 families (distances of 30 .. 66 straddle the first thresholds) tiled to 1,100"""
    _, _, B = _mods()
    a, b = [], []
    for nm in (fam_name(256, 256, 32, LEV), fam_name(300, 291, 32, LEV), fam_name(300, 291, 40, LEV), fam_name(256, 256, 40, W1)):
        a += C.named(nm).a; b += C.named(nm).b
    w = O.levenshtein_exp_batch(O.csr_from_list(a), O.csr_from_list(b), costs)
    assert len({int(x) for x in w} & set(range(30, 67))) >= 4
    idx = np.resize(np.arange(len(a)), 1100)
    got = B.levenshtein_exp_batch(B.Strings.from_list([a[i] for i in idx]), B.Strings.from_list([b[i] for i in idx]), costs).cpu().numpy().view(np.uint32)
    assert _route()[0] in (1, 2, 3, 4), _route()
    assert np.array_equal(got, w[idx]), np.flatnonzero(got != w[idx])[:8]


def test_token_batches():
    """the 256 / 256 k = 32 family with its bytes mapped to token ids above 2^16"""
    _, T, B = _mods()
    name = fam_name(256, 256, 32, LEV)
    fam = C.named(name)
    tok = lambda rows: [[0x10000 + 65537 * c for c in s] for s in rows]                        # noqa: E731
    ta, tb = B.Tokens.from_list(tok(fam.a)), B.Tokens.from_list(tok(fam.b))
    for k in C.ks(fam):
        got = B.levenshtein_k_batch_tokens(ta, tb, k, LEV).cpu().numpy().view(np.uint32)
        assert T.last_kernel_name().startswith(("lev_bits", "lev_widebits")), T.last_kernel_name()
        assert np.array_equal(got, want(name, k)), (k, np.flatnonzero(got != want(name, k))[:8])
    for k in (31, 32):
        out, edits, ne = B.levenshtein_trace_batch_tokens(ta, tb, k, LEV)
        assert "lev_bits_trace_kernel" in T.last_kernel_name(), T.last_kernel_name()
        got = B.edits_to_lists(edits, ne)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want(name, k))
        assert got == [(s or []) for _, s in scripts(name, k)]


# ================================================================ the cross window kernel
def _ww(unit_k):
    need = (2 * unit_k + 15) // 32 + 2
    return 2 if need <= 2 else 3 if need <= 3 else 4 if need <= 4 else 8


@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("k", [8, 16, 24, 32, 40, 41])
@pytest.mark.parametrize("lq", [150, 256])
def test_cross_window_kernel(lq, k, costs):
    """levenshtein_cross_with_opts: 24 queries of the family (both sides, every placement) against all of its partners and the single-run
    targets |len(q) - len(t)| = k with the run at the front, in the middle and at the end; hits, count, nearest and per-query counts"""
    torch, T, B = _mods()
    fam = C.named(fam_name(lq, lq, k, costs, "acgt"))
    g = np.random.default_rng(lq + k)
    qi = [i for i, r in enumerate(fam.rows) if r.cls in ("edge", "plus2") and not r.sub and not r.swap][:24]
    queries = [fam.a[i] for i in qi]
    targets = list(fam.b)
    for q in queries[:6]:
        h = lq // 2
        x = bytes(g.choice(C.ACGT, k + 1))
        for r in (k, k + 1):
            targets += [q[r:], q[:h] + q[h + r:], q[:lq - r], x[:r] + q, q[:h] + x[:r] + q[h:], q + x[:r]]
    qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
    nq, nt = len(queries), len(targets)
    a = O.csr_from_list([q for q in queries for _ in targets])
    b = O.csr_from_list(targets * nq)
    for kk in (k - 1, k, k + 1):
        d = O.levenshtein_k_batch(a, b, kk, costs).reshape(nq, nt)
        hits = [(q, t, int(d[q, t])) for q in range(nq) for t in range(nt) if d[q, t] != NONE]
        near = [min(((int(d[q, t]) << 32 | t) for t in range(nt) if d[q, t] != NONE), default=0xFFFFFFFFFFFFFFFF) for q in range(nq)]
        counts = [int((d[q] != NONE).sum()) for q in range(nq)]
        if kk == k:
            assert sum(1 for j, i in enumerate(qi) if fam.rows[i].cls == "edge" and d[j, i] == fam.rows[i].cost) >= 8
            assert sum(1 for q, t, x in hits if t >= len(fam.b) and x == k) >= 12, "the single-run targets at distance k"
        h, c, n, p = B.levenshtein_cross_with_opts(qs, ts, kk, costs, cap=nq * nt, nearest=True, per_query=True)
        torch.cuda.synchronize()
        assert T.last_kernel_name() == "lev_cross_win_kernel<%d, %s>" % (_ww(kk), "true" if costs[3] else "false"), T.last_kernel_name()
        gq, gt, gd = B.cross_to_arrays(h, c)
        got = list(zip(gq.tolist(), gt.tolist(), gd.tolist()))
        assert int(c.item()) == len(hits) and got == hits, (kk, sorted(set(hits) ^ set(got))[:6])
        assert [int(w) for w in n.cpu().numpy().view(np.uint64)] == near and [int(x) for x in p.cpu().numpy().view(np.uint32)] == counts
