"""-m gpu: one distance pass per kind of the route (triple_accel_amd/csrc/lev_route.h: LevPassKind) at the smallest shape that reaches it
with no switch set -- the answers against the oracle, ta_last_launch_info against the literal row (the same rows: check_spots of
tests/cpp/lev_route_check.cpp), and a single call on the row's first pair (the single-call path waits by the route's single_store)."""
import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

pytestmark = pytest.mark.gpu

MAX = 0xFFFFFFFF
UNIT = (1, 1, 0, None)
# (kind, pairs, length, k, costs) -> kernel, diags_per_lane, lanes_per_pair, pairs_per_wave, band_offset
ROWS = [
    ("single pair, scalar unit", 1, 40, 5, UNIT, (6, 64, 64, 1, 0)),
    ("bit-parallel band", 64, 100, 10, UNIT, (3, 12, 1, 64, 0)),
    ("two pairs per lane", 262144, 16, 3, UNIT, (3, 15, 1, 128, 0)),
    ("row-blocked", 1, 3000, MAX, UNIT, (4, 64, 64, 1, 0)),
    ("row-blocked tiled", 1, 8200, MAX, UNIT, (4, 64, 64, 1, 0)),
    ("DP band", 64, 100, 10, (3, 2, 1, None), (1, 6, 1, 64, 3)),
    ("wide DP", 2, 2816, MAX, (3, 2, 1, None), (2, 32, 64, 0, 2113)),         # (diagonals per thread, threads per pair: the launcher's)
    ("unit-scale", 64, 100, 20, (2, 2, 0, None), (3, 12, 1, 64, 0)),
]


def pairs(n, length, k):
    """Strided pairs: even ones a few edits apart (within k where k is a bound), odd ones unrelated."""
    g = Dg.rng(0x18 + n + length)
    a = g.integers(33, 127, size=(n, length), dtype=np.uint8)
    b = a.copy()
    edits = max(1, min(k, length) // 2)
    rows = np.arange(n)
    for _ in range(edits):                                   # substitutions, and one shift of the tail: gaps as well as mismatches
        b[rows, g.integers(0, length, size=n)] = 32
    if length > 8:
        b[:, length // 2 + 1:] = b[:, length // 2:-1].copy()
    odd = rows[1::2]
    b[odd] = g.integers(33, 127, size=(len(odd), length), dtype=np.uint8)
    return a, b


@pytest.mark.parametrize("kind,n,length,k,costs,row", ROWS, ids=[r[0] for r in ROWS])
def test_kind_at_its_smallest_shape(kind, n, length, k, costs, row):
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    a, b = pairs(n, length, k)
    want = O.levenshtein_k_batch(O.csr_from_fixed(a), O.csr_from_fixed(b), k, costs)
    got = B.levenshtein_k_batch(B.Strings.from_fixed(a), B.Strings.from_fixed(b), k, costs).cpu().numpy().view(np.uint32)
    info = T.last_launch_info()
    print(kind, info)
    assert np.array_equal(got, want), (kind, np.flatnonzero(got != want)[:10])
    seen = (info["kernel"], info["diags_per_lane"], info["lanes_per_pair"], info["pairs_per_wave"], info["band_offset"])
    assert seen == row, (kind, seen, row)
    if kind == "unit-scale":
        assert (got[got != MAX] % 2 == 0).all() and (got != MAX).any()
    # the single-call path on the first pair: it watches the pinned result word or waits for the stream as the route's single_store says
    # (false for the tiled form and for scaled answers) -- either way the right value
    one = T.levenshtein_simd_k_with_opts(a[0].tobytes(), b[0].tobytes(), k, False, T.EditCosts(*costs))
    assert (MAX if one is None else one[0]) == want[0], (kind, one, want[0])
