"""-m gpu: the column recurrence of the stride-8 band kernel (lev_bits_body.h, step8) in every instantiation that goes through it, answer
by answer against the CPU oracle: the line form, the chunk form, capped blocks (CSR), the transposition term, the checkpoint + recompute
traceback (edit for edit) and the early-out instantiation.  209 = 64 * 3 + 17 pairs: the last wavefront is ragged.  The inputs aim at the
recurrence's edges: distances of exactly k and k + 1, paths along the band's outermost diagonal on either side, and the alphabets {0x00},
{0x0C, 0x0D} (the window keeps `a` XOR 0x0C) and 0..255."""
import functools

import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

pytestmark = pytest.mark.gpu

LEV, RDAM = (1, 1, 0, None), (1, 1, 0, 1)
N = 64 * 3 + 17
NONE = 0xFFFFFFFF


@pytest.fixture(autouse=True)
def throughput_choice(monkeypatch):
    """A pass of up to 1,024 pairs is given to the kernel whose ONE wavefront is shortest (lev_plan.h: the row-blocked kernel for these
    209 pairs); TA_NO_LATENCY_RULE=1 keeps the choice a big batch gets, which is the kernel this file is about."""
    monkeypatch.setenv("TA_NO_LATENCY_RULE", "1")


def _edit_within(g, row, n_edits, alphabet):
    """n_edits random substitutions / insertions / deletions with characters of `alphabet`, cut or padded back to the row's length"""
    s = bytearray(row.tobytes())
    for _ in range(n_edits):
        t = int(g.integers(0, 3))
        c = int(alphabet[int(g.integers(0, len(alphabet)))])
        if t == 0:
            s[int(g.integers(0, len(s)))] = c
        elif t == 1:
            s.insert(int(g.integers(0, len(s) + 1)), c)
        elif len(s) > 1:
            del s[int(g.integers(0, len(s)))]
    pad = alphabet[g.integers(0, len(alphabet), size=len(row))].astype(np.uint8).tobytes()
    return np.frombuffer((bytes(s) + pad)[:len(row)], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def pairs(L, k, swaps=False):
    """(a, b): two (209, L) byte arrays, built once per geometry and shared (read only)"""
    g = Dg.rng(0xC07E + 1000 * L + k + (500 if swaps else 0))
    a = g.integers(33, 127, size=(N, L), dtype=np.uint8)
    b = a.copy()
    i = 0
    # exactly d substitutions by a character outside the alphabet, d around k: distances of k - 1, k, k + 1, k + 2
    for rep in range(10):
        for d in (k - 1, k, k + 1, k + 2):
            pos = g.choice(L, size=min(d, L), replace=False)
            b[i, pos] = 32
            i += 1
    # the path along the band's outermost diagonal: a = P M, b = M Q with |P| = |Q| = 16, and the same with the sides swapped; 15 as well,
    # which is the outermost diagonal of the transposition family's k = 30
    for plen in (16, 16, 16, 16, 15, 15, 15, 15, 16, 16):
        m = g.integers(33, 127, size=L - plen, dtype=np.uint8)
        p, q = g.integers(33, 127, size=plen, dtype=np.uint8), g.integers(33, 127, size=plen, dtype=np.uint8)
        a[i], b[i] = np.concatenate([p, m]), np.concatenate([m, q])
        a[i + 1], b[i + 1] = b[i], a[i]
        i += 2
    # mutated copies (substitute / insert / delete, adjacent swaps for the transposition family), up to k + 1 edits
    for rep in range(40):
        m = Dg.mutate(g, a[i].tobytes(), k + 1, swaps)
        b[i] = np.frombuffer((m + Dg.rand_str(g, L))[:L], dtype=np.uint8)
        i += 1
    # small alphabets: one symbol; the two symbols 0x0C, 0x0D; and all 256 byte values
    for alphabet, cnt in ((np.array([0]), 8), (np.array([0x0C, 0x0D]), 30), (np.arange(256), 30)):
        for rep in range(cnt):
            a[i] = alphabet[g.integers(0, len(alphabet), size=L)]
            b[i] = _edit_within(g, a[i], int(g.integers(0, k + 2)), alphabet)
            i += 1
    # the rest: unrelated strings (None), one identical pair
    b[i:] = g.integers(33, 127, size=(N - i, L), dtype=np.uint8)
    b[N - 1] = a[N - 1]
    assert i < N - 1
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def want_fixed(L, k, costs):
    a, b = pairs(L, k, costs[3] is not None)
    return O.levenshtein_k_batch(O.csr_from_fixed(a), O.csr_from_fixed(b), k, costs)


def gpu_fixed(L, k, costs):
    from triple_accel_amd import batch as B
    a, b = pairs(L, k, costs[3] is not None)
    return B.levenshtein_k_batch(B.Strings.from_fixed(np.array(a)), B.Strings.from_fixed(np.array(b)), k, costs).cpu().numpy().view(np.uint32)


def check_inputs_reach_the_edges(L, k, costs):
    a, b = pairs(L, k, costs[3] is not None)
    want = want_fixed(L, k, costs)
    beyond = O.levenshtein_k_batch(O.csr_from_fixed(a), O.csr_from_fixed(b), k + 1, costs)
    assert (want == k).any() and ((want == NONE) & (beyond == k + 1)).any(), "the batch holds distances of exactly k and k + 1"
    assert (want == 0).any() and (want == NONE).sum() > 10 and (want != NONE).sum() > 60


def test_core_line_form_256():
    import triple_accel_amd as T
    check_inputs_reach_the_edges(256, 32, LEV)
    got = gpu_fixed(256, 32, LEV)
    assert "lev_bits_s8_kernel<false, true, false>" in T.last_kernel_name(), T.last_kernel_name()
    want = want_fixed(256, 32, LEV)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    # the pairs P M / M Q: 32 edits along the outermost diagonal, found on either side
    assert (want[40:48] == 32).all() and (want[48:56] == 30).all()


@pytest.mark.parametrize("L", [96, 128])
def test_core_chunk_form(L):
    import triple_accel_amd as T
    check_inputs_reach_the_edges(L, 32, LEV)
    got = gpu_fixed(L, 32, LEV)
    assert "lev_bits_s8_kernel<false, false, false>" in T.last_kernel_name(), T.last_kernel_name()
    want = want_fixed(L, 32, LEV)
    assert np.array_equal(got, want), (L, np.flatnonzero(got != want)[:10])


def test_core_csr_capped_blocks():
    """lengths 32..256 inside one wavefront: pairs end inside a block of eight columns while others run on"""
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    a, b = pairs(256, 32)
    g = Dg.rng(0xC5A)
    la = g.integers(32, 257, size=N)
    lb = np.clip(la + g.integers(-4, 5, size=N), 32, 256)
    al, bl = [a[i, :la[i]].tobytes() for i in range(N)], [b[i, :lb[i]].tobytes() for i in range(N)]
    got = B.levenshtein_k_batch(B.Strings.from_list(al), B.Strings.from_list(bl), 32, LEV).cpu().numpy().view(np.uint32)
    info = T.last_launch_info()
    assert info["kernel"] == 3 and info["diags_per_lane"] == 33, info
    want = O.levenshtein_k_batch(O.csr_from_list(al), O.csr_from_list(bl), 32, LEV)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert (want != NONE).sum() > 60 and (want == NONE).sum() > 10


def test_core_transposition_256():
    import triple_accel_amd as T
    check_inputs_reach_the_edges(256, 30, RDAM)
    got = gpu_fixed(256, 30, RDAM)
    assert "lev_bits_s8_kernel<true, true, false>" in T.last_kernel_name(), T.last_kernel_name()
    want = want_fixed(256, 30, RDAM)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert (want[48:56] == 30).all() and (want[40:48] == NONE).all()      # |P| = |Q| = 15: the outermost diagonal of k = 30; 16: outside
    lev = O.levenshtein_k_batch(O.csr_from_fixed(pairs(256, 30, True)[0]), O.csr_from_fixed(pairs(256, 30, True)[1]), 30, LEV)
    assert not np.array_equal(want, lev), "some pair's answer needs the transposition term"


@pytest.mark.parametrize("costs,k", [(LEV, 32), (RDAM, 32), (RDAM, 30)])
def test_core_trace_256(costs, k):
    """levenshtein_trace_batch at length 256: the distance pass leaves the checkpoints (CKPT), the walk recomputes tiles (REC); k = 32
    with the transposition term is a band of 35 diagonals -- whatever kernel the library picks for it, the scripts are the oracle's"""
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    a, b = pairs(256, k, costs[3] is not None)
    out, edits, ne = B.levenshtein_trace_batch(B.Strings.from_fixed(np.array(a)), B.Strings.from_fixed(np.array(b)), k, costs)
    if k + (2 if costs[3] is not None else 0) <= 32:
        assert "lev_bits_trace_kernel" in T.last_kernel_name(), T.last_kernel_name()
    got_d, got_e = out.cpu().numpy().view(np.uint32), B.edits_to_lists(edits, ne)
    assert np.array_equal(got_d, want_fixed(256, k, costs))
    n_some = 0
    for i in range(N):
        wd, we = O.levenshtein_simd_k_with_opts(a[i].tobytes(), b[i].tobytes(), k, True, costs)
        if wd is None:
            assert got_d[i] == NONE and got_e[i] == [], i
        else:
            n_some += 1
            assert got_d[i] == wd and got_e[i] == we, (i, got_e[i], we)
    assert n_some > 60


def test_core_early_out_256():
    import triple_accel_amd as T
    T.set_option(T.OPT_EARLY_OUT, True)
    try:
        got = gpu_fixed(256, 32, LEV)
        name = T.last_kernel_name()
    finally:
        T.set_option(T.OPT_EARLY_OUT, False)
    assert "lev_bits_s8_kernel<false, true, true>" in name, name
    want = want_fixed(256, 32, LEV)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
