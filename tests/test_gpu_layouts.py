"""-m gpu: every device entry, on every kernel route, under hostile memory layouts (tests/layout_arena.py).

The C ABI (include/triple_accel_amd.h, ta_strings) lets `stride` exceed or undercut `len`, lets CSR offsets start anywhere, lets a blob
pointer have any byte alignment and says nothing about the bytes around the strings.  Strings.from_list / Strings.from_fixed produce one
layout each (blob at the base of a fresh allocation, off[0] == 0, stride == len, zero slack), and the kernels earn their speed exactly
there: whole 128-byte lines per string, 16-byte pieces that run past a string's end, wave-uniform predicates on fixed-length batches,
NUL as the value outside a string.  Each case here runs one batch under the plain layout and under hostile ones and asserts

  1. the plain layout's answers equal the oracle's, bit for bit (scripts edit for edit, match lists row for row);
  2. every hostile layout's answers are byte-identical to the plain layout's over the WHOLE batch;
  3. the guard bands around every output are untouched (and the slots documented as unwritten still hold the pre-fill);
  4. the route is the intended one, and the same under every layout (last_launch_info / last_kernel_name).

Layouts per route (not the full cross product): every form at the fill 0xFF, every fill at the nastiest form, every blob shift at one
form; the a-side and the b-side always take different shifts.  CSR-built routes take the forms csr (off[0] = 0 and 5) and csr_view (rows
lo..hi of a larger batch: an interior pointer into the offsets, decoy strings around); fixed-length routes take strided (stride = len +
pad) and overlap (stride < len: sliding windows over one sequence -- a batch of its own, the windows are the strings).  A fixed-length
batch handed over as CSR is a CSR batch to the launcher (chunk fetch form): its shifts are swept on the strided form instead.
Fills: 00 (the kernels' own pad value), ff, 0c (the byte-test constant of ne12), echo (the gap behind a row repeats the row, the slack
behind the last string repeats the partner's bytes there), continue (an exact occurrence of the needle straddles the haystack's end),
nul (a 0x00 right behind a NUL-free haystack).

The datasets come from the generator functions below; tests/test_layout_arena_cpu.py checks on the oracle alone that none of them lets a
case pass vacuously (both answers occur, pairs at k and just above it, length differences around the band's edge, haystacks with 0, 1 and
several hits).

Where the issue's table and the code disagree the code wins: see the docstrings of the cases.
Mutation check (done once, by hand, on a scratch copy of the library; each edit reverted afterwards):
  * load_str's strided address computed as `idx * s.len` (wave.h): 44 of the 94 cases fail -- every case with a strided side and pad > 0
    or a stride below len: fixed_up_to_one_line, line_form, static_and_sliding_windows, two_pairs_per_lane, small_alphabet_kernels,
    dp_band_kernel (all), dp_band_cost_form_in_a_child_process, one_string_against_a_batch_stride_0, exp_batch_over_windows,
    trace_checkpoint_route, trace_record_route_and_cut_scripts, levenshtein_cross, hamming_cross.  No older GPU test passes stride != len
    through load_str: the old suite cannot see it.
  * the result store of lev_bits_body.h also taken for slot n (`valid | (pair == P.n)`): 32 cases fail, all on the guard behind `out` --
    every case that runs the bit-parallel band kernel on a pair count that is no multiple of 64 (csr_chunk_form_batch_order,
    length_ordered[TA_NO_LENGTH_ORDER], fixed_up_to_one_line, line_form, static_and_sliding_windows, two_pairs_per_lane,
    unit_costs_times_g, one_string_against_a_batch_stride_0, exp_batch_over_windows, both trace cases, token_batches).  The old suite's
    tests/test_gpu_lev_bits.py and test_gpu_lev_bits_core.py stay green under it (57 passed): nothing there looks behind `out`.
  * the LINE fetch's in-string predicate loosened by one piece (`off < alen_u + 16`, lev_bits_body.h fetch_a): SURVIVES, all 94 cases
    green, and so do the old suite's two files above.  It has to: the piece it lets in holds bytes of `a` at and behind a_len + 0..15,
    i.e. rows below row a_len of the matrix, and no cell of rows <= a_len depends on a row below it (the recurrence looks up, left and
    up-left; the transposition term one row and column BACK) -- the answer is read at row a_len.  The predicate guards memory (a piece
    that starts behind the string's end reaches past the 16 bytes of read slack), not answers; the arena's 256-byte margin keeps such a
    read inside the test's own memory, and no test may turn it into a fault.  The same holds for `b`: columns behind b_len are never
    run."""

import functools

import numpy as np
import pytest

import datagen as Dg
import layout_arena as A
import oracle_lib as O
from layout_arena import Layout

pytestmark = pytest.mark.gpu

LEV, RDAM = (1, 1, 0, None), (1, 1, 0, 1)
PRINT = np.arange(33, 127, dtype=np.uint8)
ACGT = np.frombuffer(b"ACGT", np.uint8)
FOREIGN = 0x20                                                     # a byte outside every alphabet used here


def _mods():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    return torch, T, B


# ================================================================ datasets (pure numpy: imported by the CPU file as well)
def unit_k_of(k, costs):
    return max(k - costs[2], 0) // costs[1]


def _edit(g, s, edits, alphabet, trans):
    """`edits` random edits; substitutions write FOREIGN (never a match by accident)"""
    s = bytearray(s)
    for _ in range(edits):
        t = int(g.integers(0, 4 if trans else 3))
        if t == 0 and s:
            s[int(g.integers(len(s)))] = FOREIGN
        elif t == 1:
            s.insert(int(g.integers(len(s) + 1)), int(g.choice(alphabet)))
        elif t == 2 and s:
            del s[int(g.integers(len(s)))]
        elif t == 3 and len(s) > 1:
            p = int(g.integers(len(s) - 1))
            s[p], s[p + 1] = s[p + 1], s[p]
    return bytes(s)


def achievable(total, costs, max_ops=1 << 20):
    """the cheapest recipe (substitutions, transpositions, gap run lengths) whose cost under `costs` is exactly `total`, or None"""
    mc, gc, sg, tc = costs
    best = None
    for t in range(0, 4 if tc else 1):
        for runs in range(0, 8):
            for extra in range(0, 12):                              # gap items beyond one per run
                rest = total - t * (tc or 0) - runs * (sg + gc) - (extra * gc if runs else 0)
                if rest < 0 or rest % mc or (extra and not runs):
                    continue
                ops = rest // mc + t + runs + extra
                if ops <= max_ops and (best is None or ops < best[0]):
                    best = (ops, rest // mc, t, [1 + extra] + [1] * (runs - 1) if runs else [])
    return None if best is None else best[1:]


def next_above(k, costs):
    """the smallest cost above k that some script has under `costs` (k + 1 for unit costs; 39 for k = 36 under (3, 3, 0, 3))"""
    t = k + 1
    while achievable(t, costs) is None:
        t += 1
    return t


def _plant(g, n_len, total, costs, alphabet):
    """a pair of distance `total` (by construction; the CPU file asks the oracle): x random, y = x with the recipe's edits up to 8 bytes apart"""
    subs, trans, runs = achievable(total, costs)
    x = bytearray(g.choice(alphabet, n_len))
    for p in range(1, n_len):                                       # no equal neighbours: a transposition is a real edit
        while x[p] == x[p - 1]:
            x[p] = int(g.choice(alphabet))
    y, p = bytearray(x), 4
    ops = ["s"] * subs + ["t"] * trans + runs
    step = min(8, (n_len - 8 - max(runs or [0])) // max(len(ops), 1))
    assert step >= 2, "string too short for the recipe"
    cut = []
    for op in ops:
        if op == "s":
            y[p] = FOREIGN
        elif op == "t":
            y[p], y[p + 1] = y[p + 1], y[p]
        else:
            cut.append((p, op))
        p += step
    for q, r in reversed(cut):
        del y[q:q + r]
    return bytes(x), bytes(y)


@functools.lru_cache(maxsize=None)
def ds_ragged(seed, n, max_len, k, costs, min_len=0):
    """n ragged pairs, lengths min_len..max_len (min_len = 0: empty strings included): half mutated with 0 .. about k worth of edits, a fifth with a length
    difference within 2 of unit_k, a fifth unrelated, a tenth planted at distance k and at the next cost above k; sides swapped on odd
    pairs.  -> (a, b) lists of bytes"""
    alphabet = PRINT
    g = Dg.rng(seed)
    uk = unit_k_of(k, costs)
    per_edit = min(costs[0], costs[1] + costs[2])
    e_max = k // per_edit + 3
    a, b = [], []
    for i in range(n):
        cls = i % 10
        x = bytes(g.choice(alphabet, int(g.integers(min_len, max_len + 1))))
        if cls < 5:
            y = _edit(g, x, int(g.integers(0, e_max + 1)), alphabet, costs[3] is not None)
        elif cls < 7:
            d = max(0, uk + int(g.integers(-2, 3)))
            y = x + bytes(g.choice(alphabet, d)) if (len(x) < d or g.integers(2)) else x[:len(x) - d]
        elif cls < 9:
            y = bytes(g.choice(alphabet, int(g.integers(min_len, max_len + 1))))
        else:
            x, y = _plant(g, max((min_len + max_len) // 2, max_len * 3 // 4, 64), k if i % 20 == 9 else next_above(k, costs), costs, alphabet)
        if i % 2:
            x, y = y, x
        a.append(x); b.append(y)
    return a, b


def fixed_recipe(total, costs, d):
    """a script of cost `total` between strings whose lengths differ by d: one run of d + e deletions, one run of e insertions, t
    transpositions, s substitutions -> (e, t, s) with the fewest edits, or None"""
    mc, gc, sg, tc = costs
    best = None
    for e in range(0, 5):
        gaps = ((sg + (d + e) * gc) if d + e else 0) + ((sg + e * gc) if e else 0)
        for t in range(0, 4 if tc else 1):
            rest = total - gaps - t * (tc or 0)
            if rest >= 0 and rest % mc == 0 and (best is None or e + t + rest // mc < sum(best)):
                best = (e, t, rest // mc)
    return best


def fixed_edges(k, costs, d):
    """the costs nearest to k on either side that fixed_recipe reaches: (largest <= k, smallest > k); k and k + 1 under unit costs"""
    lo = k
    while lo >= 0 and fixed_recipe(lo, costs, d) is None:
        lo -= 1
    hi = k + 1
    while fixed_recipe(hi, costs, d) is None:
        hi += 1
    return lo, hi


@functools.lru_cache(maxsize=None)
def ds_fixed(seed, n, la, lb, k, costs, alphabet_name="print"):
    """n pairs of fixed lengths la >= lb: b = a with one run of la - lb deletions and then length-preserving edits worth 0 .. about the
    rest of k (two thirds), unrelated (a quarter), planted at the two costs of fixed_edges (the rest).  -> (n, la), (n, lb) uint8 arrays"""
    alphabet = PRINT if alphabet_name == "print" else ACGT
    g = Dg.rng(seed)
    trans = costs[3] is not None
    d = la - lb
    base = (costs[2] + d * costs[1]) if d else 0                    # the deletions as one run
    room = max(k - base, 0) // costs[0]                             # substitutions that still fit
    edges = fixed_edges(k, costs, d)
    a = g.choice(alphabet, (n, la)).astype(np.uint8)
    for r in a:                                                     # no equal neighbours: a transposition is a real edit
        same = np.flatnonzero(r[1:] == r[:-1]) + 1
        while len(same):
            r[same] = g.choice(alphabet, len(same))
            same = np.flatnonzero(r[1:] == r[:-1]) + 1
    b = np.empty((n, lb), dtype=np.uint8)
    for i in range(n):
        cls = i % 12
        x = bytearray(a[i])
        if cls < 3:
            y = bytearray(g.choice(alphabet, lb))
        elif cls == 11:
            e, t, subs = fixed_recipe(edges[(i // 12) % 2], costs, d)
            y = x[:4] + x[4 + d + e:]                               # the deletion run at 4; everything else up to 4 bytes apart behind it
            step = min(4, (lb - 12 - e) // max(subs + t, 1))
            assert step >= 2, "strings too short for the recipe"
            q = 8
            for _ in range(subs):
                y[q] = FOREIGN
                q += step
            for _ in range(t):
                y[q], y[q + 1] = y[q + 1], y[q]
                q += step
            y[q + 2:q + 2] = bytes([FOREIGN]) * e                   # the insertion run
            assert len(y) == lb
        else:
            p = int(g.integers(0, lb + 1))
            y = x[:p] + x[p + d:]                                   # one run of d deletions
            for _ in range(int(g.integers(0, room + 3))):
                q = int(g.integers(lb - 1))
                if trans and g.integers(3) == 0:
                    y[q], y[q + 1] = y[q + 1], y[q]
                else:
                    y[q] = FOREIGN
        b[i] = np.frombuffer(bytes(y), dtype=np.uint8)
    return a, b


@functools.lru_cache(maxsize=None)
def ds_overlap(seed, n, la, lb, step, k, costs, alphabet_name="print"):
    """n pairs that are sliding windows (distance `step`) over two sequences: seq_b = seq_a with substitutions whose density swings between
    none and more than k per window, so the windows' distances pass through k and k + 1.  -> (n, la), (n, lb) uint8 arrays of the windows"""
    alphabet = PRINT if alphabet_name == "print" else ACGT
    g = Dg.rng(seed)
    total = (n - 1) * step + la
    sa = g.choice(alphabet, total).astype(np.uint8)
    sb = sa.copy()
    d = la - lb
    room = max(k - ((costs[2] + d * costs[1]) if d else 0), 0) / costs[0]
    period = 6.0 * la
    rate = (1.0 - np.cos(2 * np.pi * np.arange(total) / period)) * (room + 4.0) / la       # substitutions per byte: 0 .. 2 (room + 4) / la
    sb[g.random(total) < rate] = FOREIGN
    win = lambda s, length: np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(s, length)[::step][:n])   # noqa: E731
    return win(sa, la), win(sb[d:] if d else sb, lb)                # (b's windows start d bytes on: the cheapest script is not forced to gap)


@functools.lru_cache(maxsize=None)
def ds_fixed_big(seed, n, la, lb, k, costs, alphabet_name="print"):
    """ds_fixed for the big unit-cost batches, vectorised: one deletion run of la - lb bytes, then 0 .. room + 2 substitutions at distinct
    random places (every twelfth pair exactly enough for distance k, or k + 1), a third of the pairs one adjacent swap when the costs have
    the transposition, a quarter of the pairs unrelated.  Substitutions stay inside a four-letter alphabet (the next letter)."""
    alphabet = PRINT if alphabet_name == "print" else ACGT
    g = Dg.rng(seed)
    d = la - lb
    base = (costs[2] + d * costs[1]) if d else 0
    room = max(k - base, 0) // costs[0]
    a = g.choice(alphabet, (n, la)).astype(np.uint8)
    p = g.integers(0, lb + 1, n)
    cols = np.arange(lb)[None, :]
    b = np.take_along_axis(a, cols + (cols >= p[:, None]) * d, axis=1)
    i = np.arange(n)
    e = g.integers(0, room + 3, n)
    e[i % 12 == 11] = room
    e[i % 24 == 23] = room + 1
    rank = np.argsort(np.argsort(g.random((n, lb)), axis=1), axis=1)
    mask = rank < e[:, None]
    if alphabet_name == "print":
        b[mask] = FOREIGN
    else:
        nxt = np.zeros(256, dtype=np.uint8)
        nxt[alphabet] = np.roll(alphabet, -1)
        b[mask] = nxt[b[mask]]
    if costs[3] is not None:
        sel = np.flatnonzero(i % 3 == 1)
        q = g.integers(0, lb - 1, len(sel))
        b[sel, q], b[sel, q + 1] = b[sel, q + 1].copy(), b[sel, q].copy()
    far = np.flatnonzero(i % 4 == 2)
    b[far] = g.choice(alphabet, (len(far), lb))
    return a, np.ascontiguousarray(b)


def rows_of(arr):
    return [r.tobytes() for r in arr]


# DP band cost settings: (costs, k, length of b against a = 150).  150 / 143 leaves room only under the third: with (2, 3, 1, None) k = 20
# unit_k = (20 - 1) / 3 = 6 and with (2, 2, 1, 3) k = 12 unit_k = 5 -- a length difference of 7 answers None for EVERY pair, which the
# dataset conditions forbid -- so those two take 150 / 147.
WEIGHTED = (((2, 3, 1, None), 20, 147), ((2, 2, 1, 3), 12, 147), ((100, 90, 3, 150), 700, 143))


# the widest k whose band fits the stride-8 window of 33 diagonals: k + 1 of them, + 2 for the transposition test (the issue's "k = 32
# (stride-8 window)" holds for LEVENSHTEIN_COSTS; under RDAMERAU_COSTS k = 32 asks for 35 diagonals and takes the static window)
S8K = {"lev": 32, "rdam": 30}


def _registry():
    """the distance datasets of the cases below: name -> (thunk -> (a, b), k, costs, ragged); built on first use, shared with the CPU file"""
    reg = {}

    def add(name, k, costs, ragged, fn, *args):
        kind = {ds_ragged: "ragged", ds_fixed: "fixed", ds_fixed_big: "fixed", ds_overlap: "overlap"}[fn]
        reg[name] = (lambda: fn(*args), k, costs, ragged, kind, 0 if ragged else args[2] - args[3])
    for costs in (LEV, RDAM):
        fam = "rdam" if costs[3] else "lev"
        s8k = S8K[fam]
        for k in sorted({12, 32, s8k}):
            add("ragged1100-%s-k%d" % (fam, k), k, costs, True, ds_ragged, 0x1A00 + k, 1100, 200, k, costs)
        add("ragged4500-%s-k%d" % (fam, s8k), s8k, costs, True, ds_ragged, 0x1A45, 4500, 200, s8k, costs)
        add("fixed100_97-%s-k20" % fam, 20, costs, False, ds_fixed, 0x1B00, 2000, 100, 97, 20, costs)
        for k in sorted({12, 32, 40, s8k}):
            add("fixed300_291-%s-k%d" % (fam, k), k, costs, False, ds_fixed, 0x1C00 + k, 2000, 300, 291, k, costs)
        add("fixed100_97-%s-k40" % fam, 40, costs, False, ds_fixed, 0x1B40, 2000, 100, 97, 40, costs)
        add("acgt150-%s-k16" % fam, 16, costs, False, ds_fixed_big, 0x1D00, 16385, 150, 150, 16, costs, "acgt")
        add("pairs24_23-%s-k6" % fam, 6, costs, False, ds_fixed_big, 0x1E00, 262144 + 65, 24, 23, 6, costs)
        for step in A.OVERLAP_STRIDES:
            add("overlap100_97-%s-k20-step%d" % (fam, step), 20, costs, False, ds_overlap, 0x1F00 + step, 2000, 100, 97, step, 20, costs)
            add("overlap300_291-%s-k%d-step%d" % (fam, s8k, step), s8k, costs, False, ds_overlap, 0x1F30 + step, 2000, 300, 291, step, s8k, costs)
        add("long40-%s-k300" % fam, 300, costs, True, ds_ragged, 0x3A00, 40, 2600, 300, costs, 2100)
        add("lone-%s-k20" % fam, 20, costs, True, ds_ragged, 0x2F00, 20, 300, 20, costs)
    for costs, k, lb in WEIGHTED:
        tag = "w%d_%d_%d_%s" % costs
        add("ragged1100-%s-k%d" % (tag, k), k, costs, True, ds_ragged, 0x2A00 + k, 1100, 200, k, costs)
        add("fixed150_%d-%s-k%d" % (lb, tag, k), k, costs, False, ds_fixed, 0x2B00 + k, 2000, 150, lb, k, costs)
        add("overlap150_%d-%s-k%d-step7" % (lb, tag, k), k, costs, False, ds_overlap, 0x2C00 + k, 2000, 150, lb, 7, k, costs)
    add("ragged1100-w3_3_0_3-k36", 36, (3, 3, 0, 3), True, ds_ragged, 0x2D00, 1100, 200, 36, (3, 3, 0, 3))
    add("ragged300-wide-k40", 40, (2, 3, 1, None), True, ds_ragged, 0x2E00, 300, 300, 40, (2, 3, 1, None))
    return reg


DISTANCE_DATASETS = _registry()


@functools.lru_cache(maxsize=None)
def dataset(name):
    """-> ((a rows, b rows), k, costs, ragged)"""
    thunk, k, costs, ragged = DISTANCE_DATASETS[name][:4]
    a, b = thunk()
    return ((a, b) if ragged else (rows_of(a), rows_of(b))), k, costs, ragged


def edge_costs(name):
    """the two distances a dataset must hold a pair at: k and the next cost above it; for fixed-length pairs, where the length difference
    d is part of every script, the nearest costs on either side of k that fixed_recipe reaches (k and k + 1 under unit costs); for the
    windows over one sequence, which differ by substitutions only, the nearest costs on either side of k of d deletions + substitutions"""
    _, k, costs, _, kind, d = DISTANCE_DATASETS[name]
    if kind == "ragged":
        return k, next_above(k, costs)
    if kind == "fixed":
        return fixed_edges(k, costs, d)
    base = (costs[2] + d * costs[1]) if d else 0
    lo = base + (k - base) // costs[0] * costs[0]
    return lo, lo + costs[0]


DEV_SHIFTS = (1, 17, 127)                                         # the single-haystack case's blob shifts


# ================================================================ layout plans: (tag, layout of a, layout of b)
def _shift_pairs():
    s = A.SHIFTS
    return [(s[i], s[(i + 4) % len(s)]) for i in range(len(s))]       # both sides see every shift, never the same one together


def csr_plans(fills=("00", "0c", "echo")):
    plans = [("csr-lead0", Layout("csr", 3, lead=0), Layout("csr", 17, lead=0)),
             ("csr-lead5", Layout("csr", 1, lead=5), Layout("csr", 65, lead=0)),
             ("csr-view", Layout("csr_view", 15), Layout("csr_view", 63))]
    plans += [("csr-view-" + f, Layout("csr_view", 65, fill=f), Layout("csr_view", 1, fill=f)) for f in fills]
    plans += [("csr-shift%d" % sa, Layout("csr", sa, lead=5, fill="0c"), Layout("csr", sb, lead=5, fill="0c")) for sa, sb in _shift_pairs()]
    return plans


def strided_plans(fills=("00", "0c", "echo"), pads=A.PADS):
    plans = [("pad%d" % p, Layout("strided", 3, pad=p), Layout("strided", 17, pad=A.PADS[(i + 2) % len(A.PADS)] if p else 0))
             for i, p in enumerate(pads)]
    plans += [("pad61-" + f, Layout("strided", 65, pad=61, fill=f), Layout("strided", 1, pad=3, fill=f)) for f in fills]
    plans += [("pad1-shift%d" % sa, Layout("strided", sa, pad=1, fill="0c"), Layout("strided", sb, pad=1, fill="0c")) for sa, sb in _shift_pairs()]
    return plans


def overlap_plans(step):
    return [("step%d-%s" % (step, f), Layout("overlap", 3, stride=step, fill=f), Layout("overlap", 17, stride=step, fill=f)) for f in ("ff", "echo")]


def lone_plans(i):
    """pair i of a lone-pair dataset: -> (CSR plans, strided plans); every shift 0..15 for the first two pairs, one shift pair else.  (One
    string per side: the strided form's pad is never stepped over, its fill surrounds the string.)"""
    shifts = [(s, (s + 5) % 16) for s in range(16)] if i < 2 else [(i % 16, (3 * i + 1) % 16)]
    csr = [("csr-shift%d" % sa, Layout("csr", sa, lead=5, fill="echo"), Layout("csr", sb, lead=0, fill="echo")) for sa, sb in shifts]
    strided = [("strided-shift%d" % sa, Layout("strided", sa, pad=3, fill="0c"), Layout("strided", sb, pad=1, fill="0c")) for sa, sb in shifts]
    return csr, strided


def shared_plans():
    """one side ONE string for every pair (stride 0), the other strided"""
    return [("shared-%s-shift%d" % (f, sa), Layout("shared", sa, fill=f), Layout("strided", sb, pad=p, fill=f))
            for sa, sb, p, f in ((1, 17, 3, "ff"), (15, 0, 0, "00"), (65, 3, 61, "echo"), (127, 16, 1, "0c"))]


def plan_layouts():
    """every Layout a case of this file uses (the CPU file verifies the arena under each of them)"""
    seen = {}
    plans = csr_plans() + strided_plans() + [p for s in A.OVERLAP_STRIDES for p in overlap_plans(s)] + shared_plans()
    plans += [p for i in range(20) for half in lone_plans(i) for p in half] + _cross_plans(True) + _cross_plans(False)
    plans += [("dev", Layout("strided", sh, pad=0, fill="continue"), Layout("strided", sh, pad=0, fill="continue")) for sh in DEV_SHIFTS]
    for _, la, lb in plans:
        seen[la] = seen[lb] = True
    return list(seen)


# ================================================================ harness
def _route():
    _, T, _ = _mods()
    return T.last_launch_info()["kernel"], T.last_kernel_name()


def _sides(a, b, la, lb):
    """rows (lists of bytes) under the two layouts -> two Strings; the arena reproduces the rows (asserted: an overlap batch must already
    be windows)"""
    ha, hb = A.host_side(a, la, partner=b), A.host_side(b, lb, partner=a, seed=1)
    assert ha.oracle == a and hb.oracle == b
    return A.to_strings(ha), A.to_strings(hb)


def _plain(B, a, b, ragged):
    if ragged:
        return B.Strings.from_list(a), B.Strings.from_list(b)
    arr = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)      # noqa: E731
    return B.Strings.from_fixed(arr(a)), B.Strings.from_fixed(arr(b))


def _oracle_csr(rows):
    return O.csr_from_list(rows)


def _run_u32(fn, sa, sb):
    """fn(sa, sb, out) with a guarded out -> (answers as uint32, route); the guards checked"""
    torch, _, _ = _mods()
    g = A.guarded(sa.n, torch.int32)
    fn(sa, sb, g.view)
    g.check()
    return g.numpy().view(np.uint32).copy(), _route()


def _u32_case(fn, a, b, want, ragged, plans, expect):
    """the four assertions of the module docstring for an entry that answers one u32 per pair; expect(route) -> bool"""
    _, _, B = _mods()
    plain, route = _run_u32(fn, *_plain(B, a, b, ragged))
    print("route:", route)
    assert np.array_equal(plain, want), ("plain layout against the oracle", np.flatnonzero(plain != want)[:8])
    assert expect(route), route
    for tag, la, lb in plans:
        got, r = _run_u32(fn, *_sides(a, b, la, lb))
        assert np.array_equal(got, plain), (tag, np.flatnonzero(got != plain)[:8])
        assert r == route, (tag, r, route)
    return plain, route


def _k_case(name, plans, expect, alphabet=None):
    (a, b), k, costs, ragged = dataset(name)
    _, _, B = _mods()
    want = O.levenshtein_k_batch(_oracle_csr(a), _oracle_csr(b), k, costs)
    fn = lambda sa, sb, out: B.levenshtein_k_batch(sa, sb, k, costs, out=out, alphabet=alphabet)      # noqa: E731
    return _u32_case(fn, a, b, want, ragged, plans, expect)


def _fam(costs):
    return "rdam" if costs[3] else "lev"


# ================================================================ the k-bounded distance routes
def _is_s8(k, costs):
    return 25 <= k + 1 + (2 if costs[3] else 0) <= 33


@pytest.mark.parametrize("costs,k", [(LEV, 12), (LEV, 32), (RDAM, 12), (RDAM, 30), (RDAM, 32)])
def test_bits_band_csr_chunk_form_batch_order(costs, k):
    """1,100 ragged pairs (< 4,096: batch order), the bit-parallel band kernel's chunk fetch form: sliding window at k = 12, stride-8 window
    at k = 32 (RDAMERAU: 30), and RDAMERAU's k = 32 -- 35 diagonals -- in the static window."""
    name = "lev_bits_s8_kernel<" if _is_s8(k, costs) else "lev_bits_kernel<"
    _k_case("ragged1100-%s-k%d" % (_fam(costs), k), csr_plans(), lambda r: r[0] == 3 and r[1].startswith(name))


@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("switch", [None, "TA_NO_LENGTH_ORDER", "TA_BITS_VLINE"])
def test_bits_band_csr_length_ordered_and_vline(costs, switch, monkeypatch):
    """4,500 ragged pairs (>= 4,096: a length-ordered subset list) in the stride-8 window, the same in batch order (TA_NO_LENGTH_ORDER=1)
    and through the VLINE fetch form (TA_BITS_VLINE=1: whole lines per lane, per-lane alignment)."""
    if switch:
        monkeypatch.setenv(switch, "1")
    vline = switch == "TA_BITS_VLINE"
    fam = _fam(costs)
    _k_case("ragged4500-%s-k%d" % (fam, S8K[fam]), csr_plans(),
            lambda r: r[0] == 3 and r[1].startswith("lev_bits_s8v_kernel<" if vline else "lev_bits_s8_kernel<"))


@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_bits_band_fixed_up_to_one_line(costs):
    """2,000 fixed-length pairs of 100 / 97 bytes, k = 20: strings of up to one 128-byte line keep the chunk form, with the wave-uniform
    in-string predicates of a fixed-length batch; strided with every pad, then windows over one sequence (stride 1 and 7 < len)."""
    fam = _fam(costs)
    expect = lambda r: r[0] == 3 and r[1].startswith("lev_bits_kernel<")                     # noqa: E731
    _k_case("fixed100_97-%s-k20" % fam, strided_plans(), expect)
    for step in A.OVERLAP_STRIDES:
        _k_case("overlap100_97-%s-k20-step%d" % (fam, step), overlap_plans(step), expect)


@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("early", [False, True])
def test_bits_band_line_form(costs, early, monkeypatch):
    """2,000 fixed-length pairs of 300 / 291 bytes: strings longer than a line take the LINE fetch form (every 128-byte line of a string
    requested once) -- sliding window at k = 12, stride-8 window at k = 32 (RDAMERAU: 30; its k = 32 is the static window's LINE form),
    with and without the early out, which lives in the stride-8 LINE form."""
    if early:
        monkeypatch.setenv("TA_EARLY_OUT", "1")
    fam = _fam(costs)
    line = lambda r: r[0] == 3 and r[1].startswith("lev_bits_line_kernel<")                  # noqa: E731
    _k_case("fixed300_291-%s-k12" % fam, strided_plans(), line)
    if costs == RDAM:
        _k_case("fixed300_291-rdam-k32", strided_plans(fills=("echo",), pads=(0, 3, 61)), line)
    s8 = "lev_bits_s8_kernel<%s, true, %s>" % ("true" if costs[3] else "false", "true" if early else "false")
    _k_case("fixed300_291-%s-k%d" % (fam, S8K[fam]), strided_plans(), lambda r: r == (3, s8))
    for step in A.OVERLAP_STRIDES:
        _k_case("overlap300_291-%s-k%d-step%d" % (fam, S8K[fam], step), overlap_plans(step), lambda r: r == (3, s8))


@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("env", [{"TA_BITS_STATIC": "1"}, {"TA_BITS_STATIC": "2"}, {"TA_FORCE_NA": "12"}])
def test_bits_band_static_and_sliding_windows(costs, env, monkeypatch):
    """the 2,000-pair batches at k = 40 (41 diagonals: beyond the stride-8 window) with the window layout pinned: sliding, static, and a
    forced register count -- chunk form (100 / 97 bytes) and LINE form (300 / 291 bytes)."""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    fam = _fam(costs)
    stat = env.get("TA_BITS_STATIC") != "1"                             # (a forced register count leaves the window to the planner: static from 8 dwords on)
    tail = ", %s>" % ("true" if stat else "false")
    plans = strided_plans(fills=("echo",), pads=(0, 3, 61))
    _k_case("fixed100_97-%s-k40" % fam, plans, lambda r: r[0] == 3 and r[1].startswith("lev_bits_kernel<") and r[1].endswith(tail))
    _k_case("fixed300_291-%s-k40" % fam, plans, lambda r: r[0] == 3 and r[1].startswith("lev_bits_line_kernel<") and r[1].endswith(tail))


@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_two_pairs_per_lane(costs, monkeypatch):
    """262,144 + 65 fixed-length pairs of 24 / 23 bytes, k = 6 (13 diagonals): two pairs per lane, 128 pairs per wavefront, the last
    wavefront holding 65 -- every pair against the oracle, byte-identical under every strided layout and to the one-pair-per-lane kernel
    (TA_NO_BITS2=1)."""
    _, T, _ = _mods()
    name = "pairs24_23-%s-k6" % _fam(costs)
    plans = strided_plans(fills=("echo",), pads=(0, 1, 61))[:5]           # the three pads, pad 61 under echo, one shift pair: 5 uploads of 6 MB
    plain, _ = _k_case(name, plans, lambda r: r[0] == 3 and r[1].startswith("lev_bits2_kernel<") and T.last_launch_info()["pairs_per_wave"] == 128)
    monkeypatch.setenv("TA_NO_BITS2", "1")
    one, _ = _k_case(name, plans[:1], lambda r: r[0] == 3 and r[1].startswith("lev_bits_kernel<") and T.last_launch_info()["pairs_per_wave"] == 64)
    assert np.array_equal(one, plain)


@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("wide", [False, True])
def test_small_alphabet_kernels(costs, wide, monkeypatch):
    """16,384 + 1 pairs of 150 bytes over ACGT, k = 16, alphabet=b"ACGT": the 2-bit-code kernel, and the 5-bit-code kernel under
    TA_BITSQ_WIDE=1.  Every strided layout surrounds the strings with bytes OUTSIDE the alphabet (0xFF, 0x0C, 0x00): the answers are the
    plain layout's under every one of them.  NOT asserted: that no pair reaches the general kernel's list because of a gap byte -- the
    list's length stays on the device and the pass reports its first kernel either way, so a scan that read gap bytes would only cost
    time, unseen here."""
    if wide:
        monkeypatch.setenv("TA_BITSQ_WIDE", "1")
    kern = "lev_bitsqw_kernel<" if wide else "lev_bitsq_kernel<"
    _k_case("acgt150-%s-k16" % _fam(costs), strided_plans(fills=("00", "0c"), pads=(0, 1, 16, 61)), lambda r: r[0] == 7 and r[1].startswith(kern),
            alphabet=b"ACGT")


@pytest.mark.parametrize("costs,k,lb,env", [w + (e,) for w in WEIGHTED for e in ({}, {"TA_BAND_NO_LINE": "1"}, {"TA_FORCE_TRANS_SELECT": "1"})
                                            if w[0][3] is not None or "TA_FORCE_TRANS_SELECT" not in e])
def test_dp_band_kernel(costs, k, lb, env, monkeypatch):
    """the DP band kernel under weighted costs -- affine gaps, the transposition as a dot4 penalty and as a select -- on 2,000 fixed-length
    pairs (150 / 147 or 143 bytes, see WEIGHTED), windows over one sequence, and 1,100 ragged pairs.  All three settings take the score
    form, whose fixed-length one-lane-per-pair batches fetch whole lines (TA_BAND_NO_LINE=1: the chunk fetch); the select form of the
    transposition (TA_FORCE_TRANS_SELECT=1) exists in the COST form only, so those cases run the cost form too; the cost form of every setting is
    test_dp_band_cost_form_in_a_child_process."""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    tag = "w%d_%d_%d_%s" % costs
    if env.get("TA_FORCE_TRANS_SELECT"):
        fixed = ragged = lambda r: r[0] == 1 and r[1].startswith("lev_band_kernel<") and ", 2, " in r[1]         # noqa: E731
    else:
        fixed = lambda r: r[0] == 1 and r[1].startswith("lev_band_score_kernel<" if env else "lev_band_score_line_kernel<")   # noqa: E731
        ragged = lambda r: r[0] == 1 and r[1].startswith("lev_band_score_kernel<")                               # noqa: E731
    _k_case("fixed150_%d-%s-k%d" % (lb, tag, k), strided_plans(), fixed)
    _k_case("overlap150_%d-%s-k%d-step7" % (lb, tag, k), overlap_plans(7), fixed)
    _k_case("ragged1100-%s-k%d" % (tag, k), csr_plans(), ragged)


def _cost_form_child():
    """runs in a fresh process started with TA_NO_SCORE_FORM=1 (the switch is read once, at the process's first DP band launch)"""
    cost = lambda r: r[0] == 1 and r[1].startswith("lev_band_kernel<")                                           # noqa: E731
    for costs, k, lb in WEIGHTED:
        tag = "w%d_%d_%d_%s" % costs
        _k_case("fixed150_%d-%s-k%d" % (lb, tag, k), strided_plans(), cost)
        _k_case("overlap150_%d-%s-k%d-step7" % (lb, tag, k), overlap_plans(7), cost)
        _k_case("ragged1100-%s-k%d" % (tag, k), csr_plans(), cost)
    print("cost form ok")


def test_dp_band_cost_form_in_a_child_process():
    """TA_NO_SCORE_FORM=1: the COST form of the DP band kernel (lev_band_kernel<...>) for all three settings -- affine gaps without a
    transposition, the dot4 transposition, the big costs -- on the same batches and the same plans as test_dp_band_kernel.  The library
    reads the switch once per process, so the cases run in a fresh child (which is what this test is about)."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, TA_NO_SCORE_FORM="1", TA_TUNING="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_layouts as G; G._cost_form_child()" % (os.path.dirname(here), here)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "cost form ok" in r.stdout, r.stderr[-3000:]


def test_wide_dp_kernel(monkeypatch):
    """300 ragged pairs of up to 300 bytes through the DP wide kernel (TA_FORCE_WIDE=1)."""
    monkeypatch.setenv("TA_FORCE_WIDE", "1")
    _k_case("ragged300-wide-k40", csr_plans(), lambda r: r[0] == 2)


@pytest.mark.parametrize("costs", [LEV, RDAM])
@pytest.mark.parametrize("rows", [32, 64])
def test_row_blocked_bit_parallel(costs, rows, monkeypatch):
    """40 pairs of 2,100..2,600 bytes, k = 300, through the row-blocked bit-parallel kernel (TA_FORCE_WIDEBITS=32 / 64)."""
    _, T, _ = _mods()
    monkeypatch.setenv("TA_FORCE_WIDEBITS", str(rows))
    _k_case("long40-%s-k300" % _fam(costs), csr_plans(), lambda r: r[0] == 4 and T.last_launch_info()["diags_per_lane"] == rows)


@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_lone_pair_on_the_scalar_unit(costs):
    """n = 1 (the scalar-unit recurrence, one wavefront): pairs of up to 300 bytes, the first two with their blobs at every shift 0..15
    (CSR and strided), the others at one shift pair each."""
    _, _, B = _mods()
    (a, b), k, _, _ = dataset("lone-%s-k20" % _fam(costs))
    fn = lambda sa, sb, out: B.levenshtein_k_batch(sa, sb, k, costs, out=out)                 # noqa: E731
    expect = lambda r: r[0] == 6 and r[1].startswith("lev_one_kernel<")                       # noqa: E731
    for i in range(len(a)):
        want = O.levenshtein_k_batch(_oracle_csr(a[i:i + 1]), _oracle_csr(b[i:i + 1]), k, costs)
        csr, strided = lone_plans(i)
        _u32_case(fn, a[i:i + 1], b[i:i + 1], want, True, csr, expect)
        _u32_case(fn, a[i:i + 1], b[i:i + 1], want, False, strided, expect)


def test_unit_costs_times_g():
    """(3, 3, 0, 3): the unit-cost kernels with k / 3 and the answers times 3 (a second store to every slot)."""
    _k_case("ragged1100-w3_3_0_3-k36", csr_plans(), lambda r: r[0] == 3 and r[1].startswith("lev_bits_kernel<"))


@pytest.mark.parametrize("costs", [LEV, (2, 3, 1, None)])
def test_exp_batch_device_driven_rounds(costs):
    """levenshtein_exp_batch on 1,100 ragged pairs (>= 1,024: the whole k schedule enqueued, list lengths on the device)."""
    _, _, B = _mods()
    (a, b), _, _, _ = dataset("ragged1100-lev-k32")
    want = O.levenshtein_exp_batch(_oracle_csr(a), _oracle_csr(b), costs)
    fn = lambda sa, sb, out: B.levenshtein_exp_batch(sa, sb, costs, out=out)                  # noqa: E731
    _u32_case(fn, a, b, want, True, csr_plans(), lambda r: r[0] in (1, 2, 3, 4))       # (the last round's kernel: the unbounded pass)


# ================================================================ hamming_batch
def test_hamming_batch():
    """200 x 1,024 bytes strided with every pad and as windows over one sequence, and 500 ragged pairs (a third of them of unequal
    lengths: TA_NONE)."""
    _, _, B = _mods()
    g = Dg.rng(0x4A00)
    x = g.choice(PRINT, (200, 1024)).astype(np.uint8)
    y = x.copy()
    y[g.random(y.shape) < 0.01] = FOREIGN
    fn = lambda sa, sb, out: B.hamming_batch(sa, sb, out=out)                                   # noqa: E731
    anyroute = lambda r: r[1] == "hamming_batch_kernel"                                         # noqa: E731  (its one kernel; it leaves no launch info)
    a, b = rows_of(x), rows_of(y)
    want = O.hamming_batch(_oracle_csr(a), _oracle_csr(b))
    assert len(set(want.tolist())) > 5
    _u32_case(fn, a, b, want, False, strided_plans(), anyroute)
    for step in A.OVERLAP_STRIDES:
        wa = rows_of(np.lib.stride_tricks.sliding_window_view(x.reshape(-1), 1024)[::step][:200])
        wb = rows_of(np.lib.stride_tricks.sliding_window_view(y.reshape(-1), 1024)[::step][:200])
        _u32_case(fn, wa, wb, O.hamming_batch(_oracle_csr(wa), _oracle_csr(wb)), False, overlap_plans(step), anyroute)
    ra = [bytes(g.choice(PRINT, int(g.integers(0, 300)))) for _ in range(500)]
    rb = [(_edit(g, s, 3, PRINT, False) if i % 3 == 0 else bytes(np.where(g.random(len(s)) < 0.05, FOREIGN, np.frombuffer(s, np.uint8)).astype(np.uint8)))
          for i, s in enumerate(ra)]
    want = O.hamming_batch(_oracle_csr(ra), _oracle_csr(rb))
    assert (want == O.NONE).sum() > 50 and (want != O.NONE).sum() > 200
    _u32_case(fn, ra, rb, want, True, csr_plans(), anyroute)


@pytest.mark.parametrize("la,lb,k", [(100, 97, 20), (300, 291, 32)])
def test_one_string_against_a_batch_stride_0(la, lb, k):
    """stride 0 on a PAIR entry: one side is ONE string, blob[0 .. len), compared with every string of the other side (the header allows
    it: stride and len are independent).  k_batch in the chunk form (100 / 97 bytes) and the LINE form (300 / 291), hamming_batch, exp and
    the checkpoint trace; the plain layout is the string written out n times."""
    _, _, B = _mods()
    g = Dg.rng(0x4B00 + la)
    n = 1500
    s = bytes(g.choice(PRINT, la))
    cut = g.integers(0, lb + 1, n)
    rows = []
    for i in range(n):
        y = bytearray(s[:cut[i]] + s[cut[i] + la - lb:])
        for q in g.choice(lb, int(g.integers(0, k + 2)) if i % 4 else lb // 2, replace=False):
            y[int(q)] = FOREIGN
        rows.append(bytes(y))
    a = [s] * n
    want = O.levenshtein_k_batch(_oracle_csr(a), _oracle_csr(rows), k, LEV)
    assert 0.1 < (want != O.NONE).mean() < 0.9
    line = la > 128

    def case(fn, b, w, expect):
        plain, route = _run_u32(fn, *_plain(B, a, b, False))
        print("route:", route)
        assert np.array_equal(plain, w) and expect(route), route
        for tag, l_one, l_rows in shared_plans():
            one, hb = A.host_side([s], l_one, n=n, partner=b), A.host_side(b, l_rows, partner=a, seed=1)
            assert one.oracle == a and one.stride == 0 and hb.oracle == b
            for sa, sb, flip in ((A.to_strings(one), A.to_strings(hb), False), (A.to_strings(hb), A.to_strings(one), True)):
                if flip and fn is not ham:
                    continue                                    # (the distance entries with the one string as a; hamming both ways round)
                got, r = _run_u32(fn, sa, sb)
                assert np.array_equal(got, plain) and r == route, (tag, flip, r, np.flatnonzero(got != plain)[:8])

    kb = lambda sa, sb, out: B.levenshtein_k_batch(sa, sb, k, LEV, out=out)                  # noqa: E731
    ex = lambda sa, sb, out: B.levenshtein_exp_batch(sa, sb, LEV, out=out)                   # noqa: E731
    ham = lambda sa, sb, out: B.hamming_batch(sa, sb, out=out)                               # noqa: E731
    case(kb, rows, want, lambda r: r[0] == 3 and r[1].startswith("lev_bits_s8_kernel<false, true" if line else "lev_bits_kernel<"))
    case(ex, rows, O.levenshtein_exp_batch(_oracle_csr(a), _oracle_csr(rows), LEV), lambda r: r[0] in (1, 2, 3, 4))
    same = [bytes(np.where(g.random(la) < 0.03, FOREIGN, np.frombuffer(s, np.uint8)).astype(np.uint8)) for _ in range(n)]
    case(ham, same, O.hamming_batch(_oracle_csr(a), _oracle_csr(same)), lambda r: r[1] == "hamming_batch_kernel")
    if not line:
        wt = _oracle_scripts(a, rows, k, LEV)
        d, scripts, ne, route = _run_trace(*_plain(B, a, rows, False), k, LEV, 2 * k + 1, False)
        assert CKPT(route) and [x for x, _ in wt] == [None if v == O.NONE else int(v) for v in d] and scripts == [(e or []) for _, e in wt]
        for tag, l_one, l_rows in shared_plans():
            one, hb = A.host_side([s], l_one, n=n, partner=rows), A.host_side(rows, l_rows, partner=a, seed=1)
            d2, s2, ne2, r2 = _run_trace(A.to_strings(one), A.to_strings(hb), k, LEV, 2 * k + 1, False)
            assert np.array_equal(d2, d) and np.array_equal(ne2, ne) and s2 == scripts and r2 == route, tag


def test_exp_batch_over_windows():
    """levenshtein_exp_batch on fixed-length batches: strided with pads, and both sides windows of one sequence (stride 1 and 7)."""
    _, _, B = _mods()
    fn = lambda sa, sb, out: B.levenshtein_exp_batch(sa, sb, LEV, out=out)                    # noqa: E731
    for name, plans in (("fixed100_97-lev-k20", strided_plans(fills=("echo",), pads=(0, 3, 61))),
                        ("overlap100_97-lev-k20-step1", overlap_plans(1)), ("overlap100_97-lev-k20-step7", overlap_plans(7))):
        (a, b), _, _, _ = dataset(name)
        want = O.levenshtein_exp_batch(_oracle_csr(a), _oracle_csr(b), LEV)
        _u32_case(fn, a, b, want, False, plans, lambda r: r[0] in (1, 2, 3, 4))


# ================================================================ scripts: levenshtein_trace_batch and its packed form
def _oracle_scripts(a, b, k, costs):
    return [O.levenshtein_simd_k_with_opts(x, y, k, True, costs) for x, y in zip(a, b)]


def _run_trace(sa, sb, k, costs, cap, packed):
    """-> (distances u32, scripts, n_edits, route); out, edits / packed and n_edits guarded; the packed words in front of a script (all of
    a None pair's slot) still hold the pre-fill"""
    torch, _, B = _mods()
    n = sa.n
    go, gn = A.guarded(n, torch.int32), A.guarded(n, torch.int32)
    if packed:
        ge = A.guarded((n, cap), torch.int32)
        B.levenshtein_trace_batch_packed(sa, sb, k, costs, cap=cap, out=go.view, packed=ge.view, n_edits=gn.view)
    else:
        ge = A.guarded((n, cap, 2), torch.int64)
        B.levenshtein_trace_batch(sa, sb, k, costs, cap=cap, out=go.view, edits=ge.view, n_edits=gn.view)
    for g in (go, ge, gn):
        g.check()
    route = _route()
    ne = gn.numpy().copy()
    if packed:
        front = np.arange(cap)[None, :] < (cap - np.minimum(ne, cap))[:, None]
        assert ge.unwritten()[front].all(), "a packed word in front of a script was written"
        scripts = B.packed_to_lists(ge.view, gn.view, allow_cut=True)
    else:
        scripts = B.edits_to_lists(ge.view, gn.view, allow_cut=True)
    return go.numpy().view(np.uint32).copy(), scripts, ne, route


def _trace_case(name, plans, expect, cap=None, packed=False):
    (a, b), k, costs, ragged = dataset(name)
    _, _, B = _mods()
    cap = 2 * k + 1 if cap is None else cap
    want = _oracle_scripts(a, b, k, costs)
    d, scripts, ne, route = _run_trace(*_plain(B, a, b, ragged), k, costs, cap, packed)
    print("route:", route)
    assert expect(route), route
    cut = 0
    for i, (wd, we) in enumerate(want):
        if wd is None:
            assert d[i] == O.NONE and ne[i] == 0 and scripts[i] == [], i
        else:
            assert d[i] == wd and ne[i] == len(we), (i, d[i], wd)
            assert scripts[i] == (we[len(we) - cap:] if packed and len(we) > cap else we[:cap]), (i, scripts[i], we)
            cut += len(we) > cap
    for tag, la, lb in plans:
        d2, s2, ne2, r2 = _run_trace(*_sides(a, b, la, lb), k, costs, cap, packed)
        assert np.array_equal(d2, d) and np.array_equal(ne2, ne) and s2 == scripts, tag
        assert r2 == route, (tag, r2, route)
    return cut


CKPT = lambda r: r[0] == 8 and "lev_bits_trace_kernel" in r[1]                                 # noqa: E731


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_trace_checkpoint_route(costs, packed, monkeypatch):
    """1,500 pairs of up to 150 bytes on the checkpoint route: CSR, fixed-length (the distance pass is the forward sweep), windows over
    one sequence, and sub-batches of 192 pairs -- whose
    views are blob + lo * stride and off + lo, the library's own interior pointers on top of the caller's."""
    fam = _fam(costs)
    _trace_case("trace-ragged1500-%s-k20" % fam, csr_plans(), CKPT, packed=packed)
    fixed = lambda r: CKPT(r) and r[1].endswith("true>")                                        # noqa: E731
    _trace_case("trace-fixed150_147-%s-k20" % fam, strided_plans(), fixed, packed=packed)
    _trace_case("overlap100_97-%s-k20-step7" % fam, overlap_plans(7), fixed, packed=packed)
    _trace_case("overlap100_97-%s-k20-step1" % fam, overlap_plans(1), fixed, packed=packed)
    monkeypatch.setenv("TA_TRACE_CHUNK_PAIRS", "192")
    _trace_case("trace-ragged1500-%s-k20" % fam, csr_plans()[:6], CKPT, packed=packed)
    _trace_case("trace-fixed150_147-%s-k20" % fam, strided_plans()[:8], fixed, packed=packed)


@pytest.mark.parametrize("packed", [False, True])
def test_trace_record_route_and_cut_scripts(packed):
    """weighted costs: the DP band kernel's argmin codes and a walk kernel (record route); and cap = 5, which cuts most scripts -- the
    first five runs in the ta_edit form, the last five right-aligned in the packed form, n_edits the true length either way."""
    rec = lambda r: r[0] == 1                                                                    # noqa: E731
    _trace_case("trace-ragged1500-w2_3_1_None-k20", csr_plans(), rec, packed=packed)
    _trace_case("trace-fixed150_147-w2_2_1_3-k12", strided_plans(), rec, packed=packed)
    assert _trace_case("trace-ragged1500-lev-k20", csr_plans(), CKPT, cap=5, packed=packed) > 100
    assert _trace_case("trace-ragged1500-w2_3_1_None-k20", csr_plans()[:6], rec, cap=5, packed=packed) > 100


def _trace_registry():
    reg = DISTANCE_DATASETS
    for costs in (LEV, RDAM):
        fam = _fam(costs)
        reg["trace-ragged1500-%s-k20" % fam] = (lambda c=costs: ds_ragged(0x5A00, 1500, 150, 20, c), 20, costs, True, "ragged", 0)
        reg["trace-fixed150_147-%s-k20" % fam] = (lambda c=costs: ds_fixed(0x5B00, 1500, 150, 147, 20, c), 20, costs, False, "fixed", 3)
    w1, w2 = (2, 3, 1, None), (2, 2, 1, 3)
    reg["trace-ragged1500-w2_3_1_None-k20"] = (lambda: ds_ragged(0x5C00, 1500, 150, 20, w1), 20, w1, True, "ragged", 0)
    reg["trace-fixed150_147-w2_2_1_3-k12"] = (lambda: ds_fixed(0x5D00, 1500, 150, 147, 12, w2), 12, w2, False, "fixed", 3)


_trace_registry()


# ================================================================ search over batches of (needle, haystack) pairs
NEEDLE = b"GATTACAGGTCA"                                            # 12 bytes: the shared needle
ORACLE_SAMPLES = [(4096, 2), (64, 1), (262144 + 65, 1)]             # (pairs, step) of every case that asks the oracle about a sample only


@functools.lru_cache(maxsize=None)
def search_dataset(name):
    """-> (needles, haystacks, k, kind): name = kind-needles-form-n.  Haystacks over ACGT (no NUL), up to 120 bytes (form fixed: exactly
    120): a quarter without the needle, a quarter with one exact copy, a quarter with two, a quarter ENDING with a proper prefix of their
    needle (3..11 bytes: the `continue` fill completes the occurrence behind the haystack's end)."""
    kind, who, form, n = name.split("-")
    n = int(n)
    g = Dg.rng(0x6A00 + n + len(name))
    needles, hays = [], []
    for i in range(n):
        nd = NEEDLE if who == "shared" else bytes(g.choice(ACGT, 12 if form == "fixed" else int(g.integers(8, 17))))
        h = bytearray(g.choice(ACGT, 120 if form == "fixed" else int(g.integers(40, 121))))
        cls = i % 4
        if cls in (1, 2):
            h[5:5 + len(nd)] = nd
        if cls == 2:
            h[30:30 + len(nd)] = nd
        if cls == 3:
            j = int(g.integers(3, len(nd)))
            h[len(h) - j:] = nd[:j]
        if form != "fixed" and i % 16 == 0:
            h = bytearray()                                         # empty haystacks among the others
        needles.append(nd); hays.append(bytes(h))
    return needles, hays, 1, kind


SEARCH_DATASETS = ["%s-%s-%s-%d" % (kind, who, form, n) for kind in ("lev", "hamming") for who in ("shared", "perpair")
                   for form in ("ragged", "fixed") for n in (64, 4096)]


def search_plans(kind, who, form):
    """(tag, needle layout, haystack layout): the haystacks CSR (off[0] = 5, a view of a larger batch) or strided with a pad that holds
    the rest of a needle; the fills that bite a search -- continue, and echo (lev) / nul (hamming)"""
    other = "echo" if kind == "lev" else "nul"
    if form == "ragged":
        hay = [Layout("csr", 3, lead=5, fill="continue"), Layout("csr_view", 65, fill="continue"), Layout("csr_view", 1, fill=other),
               Layout("csr", 127, lead=0, fill="ff")]
        per = [Layout("csr", 15, lead=5, fill="0c"), Layout("csr_view", 17), Layout("csr", 63, lead=0, fill="00"), Layout("csr_view", 16)]
    else:
        hay = [Layout("strided", 17, pad=16, fill="continue"), Layout("strided", 127, pad=61, fill="continue"),
               Layout("strided", 1, pad=3, fill=other), Layout("strided", 15, pad=1, fill=other)]
        per = [Layout("strided", 3, pad=3, fill="0c"), Layout("strided", 65, pad=0), Layout("strided", 16, pad=61, fill="00"), Layout("strided", 63, pad=1)]
    if who == "shared":
        per = [Layout("shared", s, fill=f) for s, f in ((1, "ff"), (15, "00"), (65, "0c"), (127, "ff"))]
    return [("%s|%s" % (nl.tag(), hl.tag()), nl, hl) for nl, hl in zip(per, hay)]


def search_layouts():
    seen = {}
    for kind in ("lev", "hamming"):
        for who in ("shared", "perpair"):
            for form in ("ragged", "fixed"):
                for _, nl, hl in search_plans(kind, who, form):
                    seen[nl] = seen[hl] = True
    return list(seen)


def _search_sides(needles, hays, who, nl, hl):
    hh = A.host_side(hays, hl, partner=needles, needles=needles)
    assert hh.oracle == hays
    if who == "shared":
        hn = A.host_side([needles[0]], nl, n=len(hays))
    else:
        hn = A.host_side(needles, nl, partner=hays, seed=1)
        assert hn.oracle == needles
    return A.to_strings(hn), A.to_strings(hh)


def _search_plain(B, needles, hays, who, form):
    arr = lambda rows: np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), -1)          # noqa: E731
    hs = B.Strings.from_fixed(arr(hays)) if form == "fixed" else B.Strings.from_list(hays)
    if who == "shared":
        return B.Strings.shared(needles[0], len(hays)), hs
    return (B.Strings.from_fixed(arr(needles)) if form == "fixed" else B.Strings.from_list(needles)), hs


def _run_search(fn, ns, hs, cap):
    """fn(ns, hs, cap, matches, counts) with guarded outputs -> (counts, rows per pair, kernel name)"""
    torch, T, _ = _mods()
    gm, gc = A.guarded((hs.n, cap, 3), torch.int64), A.guarded(hs.n, torch.int32)
    fn(ns, hs, cap, gm.view, gc.view)
    gm.check(); gc.check()
    c, m = gc.numpy().copy(), gm.numpy()
    rows = [[(int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF) for r in m[i, :max(0, min(int(c[i]), cap))]] for i in range(len(c))]
    return c, rows, T.last_kernel_name()


def _search_case(name, fn, oracle, expect, cap=16):
    needles, hays, k, kind = search_dataset(name)
    _, who, form, n = name.split("-")
    _, _, B = _mods()
    c, rows, kern = _run_search(fn, *_search_plain(B, needles, hays, who, form), cap)
    print("route:", kern)
    assert expect(kern), kern
    assert int(c.max()) <= cap and int(c.min()) >= 0
    step = dict((x, y) for x, y in ORACLE_SAMPLES)[int(n)]
    for i in range(0, len(hays), step):
        assert rows[i] == oracle(needles[i], hays[i]), (i, needles[i], hays[i])
    for tag, nl, hl in search_plans(kind, who, form):
        c2, rows2, kern2 = _run_search(fn, *_search_sides(needles, hays, who, nl, hl), cap)
        assert np.array_equal(c2, c) and rows2 == rows, (tag, np.flatnonzero(c2 != c)[:8])
        assert kern2 == kern, (tag, kern2, kern)


@pytest.mark.parametrize("n", [64, 4096])
@pytest.mark.parametrize("form", ["ragged", "fixed"])
@pytest.mark.parametrize("who", ["shared", "perpair"])
def test_levenshtein_search_batch(who, form, n):
    """shared needle (the scan route: a bit-parallel filter, then the exact recurrence on the candidate spans) and per-pair needles, All
    and Best, anchored.  Under `continue` an exact copy of the needle straddles every fourth haystack's end: a kernel that scans one byte
    too far reports it at distance 0 where the oracle sees distance 1 or nothing."""
    _, _, B = _mods()
    name = "lev-%s-%s-%d" % (who, form, n)
    for st, costs, anchored in ((O.ALL, LEV, False), (O.BEST, RDAM, False), (O.BEST, (2, 3, 1, None), False), (O.ALL, LEV, True)):
        fn = lambda ns, hs, cap, m, c: B.levenshtein_search_batch(ns, hs, 1, st, costs, anchored, cap=cap, matches=m, counts=c)     # noqa: E731
        oracle = lambda nd, h: O.levenshtein_search_naive_with_opts(nd, h, 1, st, costs, anchored)                                 # noqa: E731
        scan = who == "shared" and not anchored
        _search_case(name, fn, oracle, lambda kern: kern.startswith("lev_search_batch_") and ("scan" in kern) == scan)


@pytest.mark.parametrize("n", [64, 4096])
@pytest.mark.parametrize("form", ["ragged", "fixed"])
@pytest.mark.parametrize("who", ["shared", "perpair"])
@pytest.mark.parametrize("general", [False, True])
def test_hamming_search_batch(general, who, form, n, monkeypatch):
    """the bit-sliced route (shared needle of 12 bytes, 4 k <= 12) and the SWAR window compare (TA_HSEARCH_BATCH_GENERAL=1, per-pair
    needles).  Under `nul` a 0x00 sits right behind every NUL-free haystack: a kernel that scans one byte too far answers -1 for the pair."""
    _, _, B = _mods()
    if general:
        monkeypatch.setenv("TA_HSEARCH_BATCH_GENERAL", "1")
    name = "hamming-%s-%s-%d" % (who, form, n)
    bits = who == "shared" and not general
    for st in (O.ALL, O.BEST):
        fn = lambda ns, hs, cap, m, c: B.hamming_search_batch(ns, hs, 1, st, cap=cap, matches=m, counts=c)                          # noqa: E731
        oracle = lambda nd, h: O.hamming_search_simd_with_opts(nd, h, 1, st)                                                        # noqa: E731
        _search_case(name, fn, oracle, lambda kern: kern.startswith("ham_search_batch_") and ("bits" in kern) == bits)


# ================================================================ every query against every target
def _cross_batches(seed, nq, nt):
    """-> ragged (queries of 0..64 bytes, targets of 0..70: half of them a query with 0..3 edits) and fixed (21-byte queries, 21-byte
    targets: every string of the strided form starts at another alignment)"""
    g = Dg.rng(seed)
    rq = [bytes(g.choice(ACGT, int(g.integers(0, 65)))) for _ in range(nq)]
    rq[0], rq[-1] = b"", bytes(g.choice(ACGT, 64))
    rt = [(_edit(g, rq[int(g.integers(nq))], int(g.integers(0, 4)), ACGT, True) if i % 2 else bytes(g.choice(ACGT, int(g.integers(0, 71))))) for i in range(nt)]
    fq = [bytes(g.choice(ACGT, 21)) for _ in range(nq)]
    ft = [bytes(np.where(g.random(21) < 0.08, ord("N"), np.frombuffer(fq[int(g.integers(nq))], np.uint8)).astype(np.uint8)) if i % 3 else bytes(g.choice(ACGT, 21))
          for i in range(nt)]
    return (rq, rt), (fq, ft)


def _cross_plans(ragged):
    if ragged:
        plans = [("view", Layout("csr_view", 15, fill="echo"), Layout("csr_view", 63, fill="echo")), ("lead5", Layout("csr", 1, lead=5), Layout("csr", 65, lead=5, fill="0c"))]
        plans += [("shift%d" % sa, Layout("csr", sa, lead=5, fill="00"), Layout("csr", sb, lead=0, fill="ff")) for sa, sb in _shift_pairs()]
    else:
        plans = [("pad%d" % p, Layout("strided", 3, pad=p, fill="echo"), Layout("strided", 17, pad=A.PADS[(i + 2) % 5], fill="echo")) for i, p in enumerate(A.PADS)]
        plans += [("shift%d" % sa, Layout("strided", sa, pad=1, fill="0c"), Layout("strided", sb, pad=3, fill="00")) for sa, sb in _shift_pairs()]
    return plans


def _run_cross(call, qs, ts, cap, per_query):
    """call(qs, ts, cap, hits, count, nearest, per_query) with every output guarded -> (sorted hits, count, nearest words, per-query
    counts, kernel name)"""
    torch, T, B = _mods()
    gh, gc, gn = A.guarded((cap, 4), torch.int32), A.guarded(1, torch.int64), A.guarded(qs.n, torch.int64)
    gp = A.guarded(qs.n, torch.int32) if per_query else None
    call(qs, ts, cap, gh.view, gc.view, gn.view, gp.view if gp else None)
    for g in (gh, gc, gn) + ((gp,) if gp else ()):
        g.check()
    q, t, d = B.cross_to_arrays(gh.view, gc.view)
    n = int(gc.numpy()[0])
    return (list(zip(q.tolist(), t.tolist(), d.tolist())), n, gn.numpy().view(np.uint64).tolist(),
            gp.numpy().view(np.uint32).tolist() if gp else None, T.last_kernel_name())


def _cross_case(call, want, queries, targets, ragged, expect, per_query):
    _, _, B = _mods()
    cap = len(queries) * len(targets)
    plain = _run_cross(call, *_plain(B, queries, targets, ragged), cap, per_query)
    print("route:", plain[4])
    assert expect(plain[4]), plain[4]
    assert plain[:4] == want, "plain layout against the oracle"
    for tag, lq, lt in _cross_plans(ragged):
        got = _run_cross(call, *_sides(queries, targets, lq, lt), cap, per_query)
        assert got == plain, tag


@pytest.mark.parametrize("shape", [(63, 65), (130, 1030)])
@pytest.mark.parametrize("costs", [LEV, RDAM])
def test_levenshtein_cross(shape, costs):
    """nq x nt on both sides of the wavefront and of the query tile; CSR views with decoys, off[0] = 5, every shift; 21-byte strings strided
    with every pad."""
    _, _, B = _mods()
    k = 3
    for ragged, (queries, targets) in zip((True, False), _cross_batches(0x7A00 + shape[0], *shape)):
        nq, nt = shape
        d = O.levenshtein_k_batch(_oracle_csr([q for q in queries for _ in range(nt)]), _oracle_csr([t for _ in range(nq) for t in targets]), k, costs).reshape(nq, nt)
        hits = [(q, t, int(d[q, t])) for q in range(nq) for t in range(nt) if d[q, t] != O.NONE]
        near = [min(((int(d[q, t]) << 32 | t) for t in range(nt) if d[q, t] != O.NONE), default=0xFFFFFFFFFFFFFFFF) for q in range(nq)]
        assert nt // 4 < len(hits) < nq * nt // 2
        call = lambda qs, ts, cap, h, c, n, p: B.levenshtein_cross(qs, ts, k, costs, cap=cap, hits=h, count=c, nearest=n)               # noqa: E731
        _cross_case(call, (hits, len(hits), near, None), queries, targets, ragged, lambda kern: kern.startswith("lev_cross_kernel<"), False)


@pytest.mark.parametrize("shape", [(63, 65), (130, 1030)])
@pytest.mark.parametrize("upper", [False, True])
def test_hamming_cross(shape, upper):
    """the Hamming twin, with nearest, per_query and upper: equal lengths only, so the ragged batch hits where a target is a substituted
    query (or both are empty) and the 21-byte strided batch hits everywhere a target came from a query."""
    _, _, B = _mods()
    k = 3
    for ragged, (queries, targets) in zip((True, False), _cross_batches(0x7B00 + shape[0], *shape)):
        if ragged:                                                  # edits that keep the length: substitutions only
            g = Dg.rng(0x7B01)
            targets = [bytes(np.where(g.random(len(t)) < 0.05, ord("N"), np.frombuffer(t, np.uint8)).astype(np.uint8)) if i % 2 else t
                       for i, t in enumerate(queries[int(j)] for j in g.integers(len(queries), size=len(targets)))]
        hits, near, counts = [], [], []
        for q, s in enumerate(queries):
            row = [(q, t, sum(x != y for x, y in zip(s, u))) for t, u in enumerate(targets) if len(u) == len(s) and (not upper or t > q)]
            row = [h for h in row if h[2] <= k]
            hits += row
            near.append(min((d << 32 | t for _, t, d in row), default=0xFFFFFFFFFFFFFFFF))
            counts.append(len(row))
        assert len(hits) > (0 if upper and ragged else 10)
        call = lambda qs, ts, cap, h, c, n, p: B.hamming_cross(qs, ts, k, cap=cap, hits=h, count=c, nearest=n, per_query=p, upper=upper)   # noqa: E731
        _cross_case(call, (hits, len(hits), near, counts), queries, targets, ragged, lambda kern: kern.startswith("ham_cross_kernel<"), True)


# ================================================================ one long haystack
@pytest.mark.parametrize("shift", DEV_SHIFTS)
def test_single_haystack_search_as_an_interior_view(shift):
    """levenshtein_search_dev / _best_dev / hamming_search_dev over one 150,000-byte haystack that is an interior view of a larger tensor;
    the haystack ends with the first 8 bytes of the needle and the memory behind it goes on with the rest."""
    torch, T, B = _mods()
    g = Dg.rng(0x8A00)
    needle = b"GATTACAGGTCATGCA"
    hay = bytearray(g.choice(ACGT, 150_000))
    for p in range(700, len(hay) - 100, 9_000):
        hay[p:p + len(needle)] = _edit(g, needle, int(g.integers(0, 3)), ACGT, False)[:len(needle)].ljust(len(needle), b"A")
    hay[len(hay) - 8:] = needle[:8]
    hay = bytes(hay)
    h = A.host_side([hay], Layout("strided", shift, pad=0, fill="continue"), needles=needle)
    assert h.buf[h.last_end():h.last_end() + 8].tobytes() == needle[8:]
    t = torch.from_numpy(h.buf).cuda()
    view = (t[h.base:], len(hay))
    plain = B.haystack_tensor(hay)
    for costs, k in ((LEV, 2), ((2, 3, 1, None), 4)):
        want = O.levenshtein_search_naive_with_opts(needle, hay, k, O.ALL, costs)
        assert len(want) > 5 and all(e <= len(hay) for _, e, _ in want)
        got = [tuple(int(x) for x in r) for r in B.levenshtein_search_dev(needle, view, k, costs)]
        name = T.last_kernel_name()
        print("route:", name)
        assert name.startswith(("lev_search", "lev_filter")), name          # the tiled exact search, or the unit-cost filter in front of it
        assert got == want and got == [tuple(int(x) for x in r) for r in B.levenshtein_search_dev(needle, plain, k, costs)]
        assert T.last_kernel_name() == name
        best = [tuple(int(x) for x in r) for r in B.levenshtein_search_best_dev(needle, view, k, costs)]
        assert best == [tuple(int(x) for x in r) for r in B.levenshtein_search_best_dev(needle, plain, k, costs)] and len(best) > 0
        assert B.levenshtein_search_first_dev(needle, view, k, costs) == want[0]
    want = O.hamming_search_naive_with_opts(needle, hay, 2, O.ALL)
    got = [tuple(int(x) for x in r) for r in B.hamming_search_dev(needle, view, 2)]
    assert T.last_kernel_name().startswith("hamming_search_"), T.last_kernel_name()
    assert len(want) > 5 and got == want and got == [tuple(int(x) for x in r) for r in B.hamming_search_dev(needle, plain, 2)]


# ================================================================ token batches
def test_token_batches_as_interior_views():
    """1,100 CSR sequences of 32-bit items: the values an interior view (at every 4-byte multiple 0..3 items), off[0] = 5, the items around
    them a sentinel that is ALSO a token of the vocabulary.  The binding has no element stride: CSR only."""
    import tokens_ref as R
    torch, T, B = _mods()
    g = Dg.rng(0x9A00)
    vocab = np.concatenate([g.integers(0, 1 << 32, 150, dtype=np.uint64), [0x5A5A5A5A, 0, 0xFFFFFFFF]]).astype(np.int64)
    a, b = [], []
    for i in range(1100):
        x = [int(v) for v in g.choice(vocab, int(g.integers(0, 100)))]
        y = list(x)
        for _ in range(int(g.integers(0, 14))):
            op, p = int(g.integers(3)), int(g.integers(len(y) + 1))
            if op == 0 or not y:
                y.insert(p, int(g.choice(vocab)))
            elif op == 1:
                del y[min(p, len(y) - 1)]
            else:
                y[min(p, len(y) - 1)] = int(g.choice(vocab))
        if i % 5 == 0:
            y = [int(v) for v in g.choice(vocab, int(g.integers(0, 100)))]
        a.append(x); b.append(y)
    coded = [R.codes(x, y) for x, y in zip(a, b)]
    ca, cb = _oracle_csr([c[0] for c in coded]), _oracle_csr([c[1] for c in coded])
    k = 8
    want = O.levenshtein_k_batch(ca, cb, k, LEV)
    want_exp = O.levenshtein_exp_batch(ca, cb, RDAM)
    assert 0.1 < (want != O.NONE).mean() < 0.9
    want_scripts = [O.levenshtein_simd_k_with_opts(c[0], c[1], k, True, LEV) for c in coded]

    def run(ta, tb):
        go, gx, gd, gn = (A.guarded(1100, torch.int32) for _ in range(4))
        ge = A.guarded((1100, 2 * k + 1, 2), torch.int64)
        B.levenshtein_k_batch_tokens(ta, tb, k, LEV, out=go.view)
        name = T.last_kernel_name()
        B.levenshtein_exp_batch_tokens(ta, tb, RDAM, out=gx.view)
        B.levenshtein_trace_batch_tokens(ta, tb, k, LEV, out=gd.view, edits=ge.view, n_edits=gn.view)
        for x in (go, gx, gd, gn, ge):
            x.check()
        return go.numpy().view(np.uint32).copy(), gx.numpy().view(np.uint32).copy(), gd.numpy().view(np.uint32).copy(), B.edits_to_lists(ge.view, gn.view), name

    plain = run(B.Tokens.from_list(a), B.Tokens.from_list(b))
    assert np.array_equal(plain[0], want) and np.array_equal(plain[1], want_exp) and np.array_equal(plain[2], want)
    assert plain[3] == [(s or []) for _, s in want_scripts]
    for shift in range(4):
        ta = A.to_tokens(*A.host_tokens(a, shift_items=shift, lead=5))
        tb = A.to_tokens(*A.host_tokens(b, shift_items=(shift + 1) % 4, lead=3, sentinel=0))
        got = run(ta, tb)
        assert all(np.array_equal(x, y) for x, y in zip(got[:3], plain[:3])) and got[3] == plain[3] and got[4] == plain[4], shift
