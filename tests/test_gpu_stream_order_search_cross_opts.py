"""gpu: the threading contract of include/triple_accel_amd.h for ta_levenshtein_search_cross_with_opts' two-word route, with the gate
and the runner of tests/stream_order_lib.py (see tests/test_gpu_stream_order.py for the method).  The entry keeps its candidate count,
its records, its own nearest words and -- needles beyond 32 bytes -- the exact pass's memory-backed columns in thread-local scratch
(SLOT_SX_CTL, SLOT_SX_REC, SLOT_SX_NEAR, SLOT_SX_COL): a call that used them records, and a later call on another stream waits."""
import functools

import pytest

import stream_order_lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gate():
    return L.Gate()


@functools.lru_cache(maxsize=None)
def _d_search_cross_opts(seed):
    import search_cross_cases as Sx
    import search_cross_opts_cases as Sy
    needles = Sy.panel(seed, 12)
    assert max(map(len, needles)) > 32
    hays = Sx.reads(seed + 1, 48, needles, lo=80, hi=140)
    return needles, hays, Sx.join(needles, hays, 2, L.UNIT, False)


def search_cross_opts(seed):
    """12 needles of up to 64 bytes in 48 haystacks: the candidate records, their count, the library's nearest words (best without
    nearest) and the memory-backed columns"""
    torch, T, B = L._mods()
    needles, hays, (recs, nearest, best, per) = _d_search_cross_opts(seed)
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)

    def check(r):
        hits, count, _, got_best, _ = r
        L._cross_records(B, hits, count, recs)
        gb = got_best.cpu().numpy()
        assert [(int(x[0]), int(x[1]), int(x[2]) & L.NONE) for x in gb] == [tuple(x) for x in best]

    return L.Case(lambda: B.levenshtein_search_cross_with_opts(nd, hs, 2, L.UNIT, best=True), check, L._name_has("lev_search_cross_w2_scan_kernel"))


def test_async_call_records(gate):
    """A (the two-word route on s1 behind the gate) took scratch, so it recorded; B (a small ragged k batch on s2) waited for it"""
    L.run_gated(gate, search_cross_opts(101), L.k_small_ragged(202), b_async=True)


def test_async_call_waits(gate):
    """A = levenshtein_exp_batch on s1 behind the gate; B = the two-word route on s2: complete once an event recorded on s2 after it has
    been synchronised, and by then nothing of s1 may be pending"""
    L.run_gated(gate, L.exp_batch(101), search_cross_opts(404), b_async=True)


def test_the_column_slot_is_ordered_across_a_stream_switch(gate):
    """A and B both take the two-word route, on different streams and different strings: B's columns and records are A's buffers"""
    L.run_gated(gate, search_cross_opts(101), search_cross_opts(404), b_async=True)
