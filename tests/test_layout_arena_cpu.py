"""The hostile arena of tests/layout_arena.py is right, byte for byte, and the datasets of tests/test_gpu_layouts.py are worth running:
none of the GPU cases can pass vacuously.  No GPU: the arena's host stage is plain numpy and the dataset conditions are the oracle's."""
import numpy as np
import pytest

import datagen as Dg
import layout_arena as A
import oracle_lib as O
import test_gpu_layouts as G
from layout_arena import Layout

LAYOUTS = list(dict.fromkeys(G.plan_layouts() + G.search_layouts()))


def _strings_for(layout, seed=0):
    """(rows, partner rows, needles) that fit the layout's form: ragged with empty strings for CSR, one length for the strided forms"""
    g = Dg.rng(0x5EED + seed)
    if layout.form in ("csr", "csr_view"):
        rows = [bytes(g.integers(1, 255, int(g.integers(0, 40)), dtype=np.uint8)) for _ in range(37)]
        rows[5] = rows[-1] = b""
        if layout.fill in ("continue", "nul"):
            rows[-1] = bytes(g.integers(1, 255, 30, dtype=np.uint8))
    elif layout.form == "shared":
        rows = [bytes(g.integers(1, 255, 21, dtype=np.uint8))]
    else:
        seq = g.integers(1, 255, 36 * 7 + 50, dtype=np.uint8)
        step = layout.stride if layout.form == "overlap" else 50
        rows = [seq[i * step:i * step + 50].tobytes() for i in range(1 + (len(seq) - 50) // step)][:37]
    partner = [bytes(g.integers(1, 255, len(r) + 40, dtype=np.uint8)) for r in rows]
    needles = [bytes(g.integers(1, 255, 9, dtype=np.uint8)) for _ in rows]
    return rows, partner, needles


@pytest.mark.parametrize("layout", LAYOUTS, ids=[x.tag() for x in LAYOUTS])
def test_arena_reproduces_the_strings_and_fills_everything_else(layout):
    rows, partner, needles = _strings_for(layout)
    n = 11 if layout.form == "shared" else None
    h = A.host_side(rows, layout, n=n, partner=partner, needles=needles)
    # the strings, read the way the C ABI reads them
    if h.off is not None:
        o = h.off[h.row0:h.row0 + h.n + 1]
        got = [h.buf[h.base + int(o[i]):h.base + int(o[i + 1])].tobytes() for i in range(h.n)]
    else:
        got = [h.buf[h.base + i * h.stride:h.base + i * h.stride + h.length].tobytes() for i in range(h.n)]
    assert got == h.oracle == h.extract()
    assert h.oracle == (rows * n if layout.form == "shared" else rows)         # (the overlap rows here ARE windows: nothing is re-derived)
    # the layout is the one asked for
    assert h.base % 256 == layout.shift and h.base >= A.MARGIN
    if layout.form == "csr":
        assert h.row0 == 0 and int(h.off[0]) == layout.lead
    if layout.form == "csr_view":
        assert h.row0 > 0 and int(h.off[h.row0]) > 0 and len(h.off) > h.row0 + h.n + 1      # an interior slice of a larger batch
    if layout.form == "strided":
        assert h.stride == h.length + layout.pad
    if layout.form == "overlap":
        assert 0 < h.stride == layout.stride < h.length
    if layout.form == "shared":
        assert h.stride == 0 and h.n == n
    # the margins: at least MARGIN bytes in front of the first string, SLACK + MARGIN behind the last one
    first = min(s for s, _ in h.spans())
    assert first >= A.MARGIN and len(h.buf) - h.last_end() >= A.SLACK + A.MARGIN
    # every byte that belongs to no string: the fill (decoy strings and the special gaps apart)
    owned = np.zeros(len(h.buf), dtype=bool)
    for s, e in h.spans():
        owned[s:e] = True
    assert np.array_equal(owned, h.owned)
    free = ~owned & ~h.decoy & ~h.special
    assert (h.buf[free] == A.BASE_OF_FILL[layout.fill]).all()
    assert h.decoy.any() == (layout.form == "csr_view") and not (h.decoy & owned).any()
    if layout.fill in A.PLAIN_FILLS:
        assert not h.special.any()
        assert (h.buf[:first][~h.decoy[:first]] == A.PLAIN_FILLS[layout.fill]).all()
        tail = h.buf[h.last_end():h.last_end() + A.SLACK]
        assert layout.form == "csr_view" or (tail == A.PLAIN_FILLS[layout.fill]).all()


def _gap_after(h, i):
    """the bytes between string i and the next thing the layout puts there (the whole tail behind the batch's last byte)"""
    spans = h.spans()
    end = spans[i][1]
    if end == h.last_end():
        return h.buf[end:end + A.SLACK + A.MARGIN // 2]
    return h.buf[end:spans[i + 1][0]]


@pytest.mark.parametrize("form,kw", [("strided", {"pad": 61}), ("strided", {"pad": 3}), ("csr", {"lead": 5}), ("csr_view", {})])
def test_echo_repeats_the_row_in_its_gap_and_the_partner_behind_the_last_string(form, kw):
    layout = Layout(form, 17, fill="echo", **kw)
    rows, partner, _ = _strings_for(layout, 1)
    rows[-1] = rows[-1] or b"tail"
    h = A.host_side(rows, layout, partner=partner)
    last = len(rows) - 1
    tail = _gap_after(h, last)
    want = partner[last][len(rows[last]):]
    assert len(want) >= A.SLACK and tail[:len(want)].tobytes() == want      # a kernel that compares past the end of a sees b's own bytes
    if form == "strided":
        for i in range(last):
            gap = _gap_after(h, i).tobytes()
            assert len(gap) == kw["pad"] and gap == (rows[i] * 3)[:len(gap)]  # ... and one that reads past a row sees the row again


@pytest.mark.parametrize("form,kw", [("strided", {"pad": 16}), ("strided", {"pad": 61}), ("csr", {"lead": 5}), ("csr_view", {})])
def test_continue_plants_an_occurrence_that_straddles_the_end(form, kw):
    """the oracle on haystack + gap finds a match that ends behind the haystack's end; on the haystack alone it cannot"""
    layout = Layout(form, 3, fill="continue", **kw)
    g = Dg.rng(0xC0)
    needle = b"GATTACAGGT"
    hays = [bytes(g.choice(G.ACGT, 60)) for _ in range(9)]
    hays[2] = hays[2][:-4] + needle[:4]                                     # ends with a proper prefix of the needle
    hays[-1] = hays[-1][:-7] + needle[:7]
    h = A.host_side(hays, layout, needles=needle)
    rows = range(len(hays)) if form == "strided" else [len(hays) - 1]       # (CSR rows touch: only the last one has bytes behind it)
    for i in rows:
        gap = _gap_after(h, i).tobytes()
        assert gap.startswith(A.continuation(hays[i], needle))
        inside = O.levenshtein_search_naive_with_opts(needle, hays[i], 0, O.ALL)
        beyond = O.levenshtein_search_naive_with_opts(needle, hays[i] + gap, 0, O.ALL)
        assert all(e <= len(hays[i]) for _, e, _ in inside)
        assert any(e > len(hays[i]) and s <= len(hays[i]) for s, e, _ in beyond), i
        assert [m for m in O.hamming_search_naive_with_opts(needle, hays[i] + gap, 0, O.ALL) if m[1] > len(hays[i])]
    assert A.continuation(hays[2], needle) == needle[4:] and A.continuation(hays[-1], needle) == needle[7:]


@pytest.mark.parametrize("form,kw", [("strided", {"pad": 1}), ("strided", {"pad": 61}), ("csr", {"lead": 0}), ("csr_view", {})])
def test_nul_sits_right_behind_a_nul_free_haystack(form, kw):
    layout = Layout(form, 65, fill="nul", **kw)
    g = Dg.rng(0xC1)
    hays = [bytes(g.choice(G.ACGT, 40)) for _ in range(7)]
    h = A.host_side(hays, layout)
    for i in (range(len(hays)) if form == "strided" else [len(hays) - 1]):
        gap = _gap_after(h, i)
        assert gap[0] == 0 and 0 not in hays[i]
        O.hamming_search_simd_with_opts(b"ACG", hays[i], 1, O.ALL)          # fine ...
        with pytest.raises(ValueError):                                       # ... and one byte further the reference panics
            O.hamming_search_simd_with_opts(b"ACG", hays[i] + gap[:1].tobytes(), 1, O.ALL)


def test_overlap_rows_are_derived_from_the_layout():
    """rows that are NOT windows of one sequence: the arena builds the sequence from their heads and hands back the windows it made"""
    g = Dg.rng(0xC2)
    rows = [bytes(g.integers(1, 255, 20, dtype=np.uint8)) for _ in range(30)]
    for step in A.OVERLAP_STRIDES:
        h = A.host_side(rows, Layout("overlap", 1, stride=step))
        seq = b"".join(r[:step] for r in rows[:-1]) + rows[-1]
        assert h.oracle == [seq[i * step:i * step + 20] for i in range(30)] == h.extract()
        assert h.oracle[-1] == rows[-1] and h.oracle[0][:step] == rows[0][:step] and h.oracle != rows


def test_token_arena():
    g = Dg.rng(0xC3)
    seqs = [list(g.integers(0, 1 << 32, int(g.integers(0, 30)), dtype=np.uint64)) for _ in range(40)]
    vals, base, off = A.host_tokens(seqs, shift_items=3, lead=5)
    assert int(off[0]) == 5 and base % 4 == 3
    assert [list(vals[base + off[i]:base + off[i + 1]]) for i in range(40)] == [[int(x) for x in s] for s in seqs]
    mask = np.ones(len(vals), dtype=bool)
    mask[base + off[0]:base + off[-1]] = False
    assert (vals[mask] == 0x5A5A5A5A).all() and mask[:base + 5].all() and mask[-64:].all()


# ================================================================ the datasets of the GPU file
@pytest.mark.parametrize("name", sorted(G.DISTANCE_DATASETS))
def test_distance_dataset_conditions(name):
    """both answers occur (Some in [0.1, 0.9] at the case's k), a pair sits at each of the two costs that hug k (edge_costs: k and k + 1
    wherever a script can cost that), and -- ragged datasets; a fixed-length batch has ONE length difference by construction -- at
    least 5 % of the pairs have a length difference within 2 of the dispatcher's unit_k, on either side."""
    (a, b), k, costs, ragged = G.dataset(name)
    lo, hi = G.edge_costs(name)
    assert lo <= k < hi
    d = O.levenshtein_k_batch(O.csr_from_list(a), O.csr_from_list(b), hi, costs)
    some = float((d <= k).mean())
    assert 0.1 <= some <= 0.9, some
    assert (d == lo).any() and (d == hi).any(), ((d == lo).sum(), (d == hi).sum())
    if ragged:
        la, lb = np.array([len(x) for x in a]), np.array([len(x) for x in b])
        uk = np.array([O.levenshtein_select(int(x), int(y), k, costs)[1] for x, y in zip(la, lb)])
        near = np.abs(np.abs(la - lb) - uk) <= 2
        assert near.mean() >= 0.05, near.mean()
        assert (np.abs(la - lb) > uk).any() and (np.abs(la - lb) < uk).any()
    if G.DISTANCE_DATASETS[name][4] == "overlap":                          # the rows really are windows: the arena re-derives nothing
        step = int(name.rsplit("step", 1)[1])
        for rows in (a, b):
            assert A.host_side(rows, Layout("overlap", 0, stride=step)).oracle == rows


@pytest.mark.parametrize("name", sorted(G.SEARCH_DATASETS))
def test_search_dataset_conditions(name):
    """haystacks with no hit, with one hit and with several, under the case's own search (and, for hamming search, no NUL byte)"""
    needles, hays, k, kind = G.search_dataset(name)
    counts = []
    for nd, h in zip(needles, hays):
        if kind == "hamming":
            assert 0 not in h and 0 not in nd
            counts.append(len(O.hamming_search_simd_with_opts(nd, h, k, O.BEST)))
        else:
            counts.append(len(O.levenshtein_search_naive_with_opts(nd, h, k, O.BEST)))
    counts = np.array(counts)
    assert (counts == 0).sum() >= 3 and (counts == 1).sum() >= 3 and (counts > 1).sum() >= 3, np.bincount(np.minimum(counts, 3))
    # some haystacks end with a proper prefix of their needle: the `continue` fill completes an occurrence there
    assert sum(1 for nd, h in zip(needles, hays) if nd and len(A.continuation(h, nd)) < len(nd)) >= 3


def test_samples_are_big_enough():
    """where a GPU case asks the oracle about a sample only, the sample is 2,000 pairs or every pair"""
    for n, step in G.ORACLE_SAMPLES:
        assert len(range(0, n, step)) >= min(2000, n), (n, step)
