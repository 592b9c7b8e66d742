"""gpu: the threading contract of include/triple_accel_amd.h for ta_hamming_search_cross_with_opts' two-word route, with the gate and
the runner of tests/stream_order_lib.py (see tests/test_gpu_stream_order.py for the method).  The entry keeps the packed nearest words
in thread-local scratch (SLOT_HSX_CTL, SLOT_HSX_WORD, shared with ta_hamming_search_cross): a call that used them records, and a later
call on another stream waits."""
import functools

import pytest

import stream_order_lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gate():
    return L.Gate()


@functools.lru_cache(maxsize=None)
def _d_hsearch_cross_opts(seed):
    import hsearch_cross_opts_cases as Hy
    needles = Hy.panel(seed, 12)
    assert max(map(len, needles)) > 32
    hays = Hy.reads(seed + 1, 48, needles, lo=80, hi=140)
    return needles, hays, Hy.join(needles, hays, 2)


def hsearch_cross_opts(seed):
    """12 needles of up to 64 bytes in 48 haystacks: the packed nearest words, unpacked by the finish kernel"""
    torch, T, B = L._mods()
    needles, hays, (recs, nearest, best, per) = _d_hsearch_cross_opts(seed)
    nd, hs = B.Strings.from_list(needles), B.Strings.from_list(hays)

    def check(r):
        hits, count, got_near, got_best, got_per = r
        L._cross_records(B, hits, count, recs)
        assert [int(x) & 0xFFFFFFFFFFFFFFFF for x in got_near.cpu().numpy()] == list(nearest)
        assert [(int(x[0]), int(x[1]), int(x[2]) & L.NONE) for x in got_best.cpu().numpy()] == [tuple(x) for x in best]
        assert [int(x) & L.NONE for x in got_per.cpu().numpy()] == list(per)

    return L.Case(lambda: B.hamming_search_cross_with_opts(nd, hs, 2, nearest=True, best=True, per_haystack=True), check,
                  L._name_has("ham_search_cross_w2_kernel"))


def test_async_call_records(gate):
    """A (the two-word route on s1 behind the gate) took scratch, so it recorded; B (a small ragged k batch on s2) waited for it"""
    L.run_gated(gate, hsearch_cross_opts(101), L.k_small_ragged(202), b_async=True)


def test_async_call_waits(gate):
    """A = levenshtein_exp_batch on s1 behind the gate; B = the two-word route on s2: complete once an event recorded on s2 after it has
    been synchronised, and by then nothing of s1 may be pending"""
    L.run_gated(gate, L.exp_batch(101), hsearch_cross_opts(404), b_async=True)


def test_the_packed_words_are_ordered_across_a_stream_switch(gate):
    """A and B both take the two-word route, on different streams and different strings: B's packed words are A's buffer"""
    L.run_gated(gate, hsearch_cross_opts(101), hsearch_cross_opts(404), b_async=True)


def test_the_one_word_entry_and_the_two_word_route_share_the_slots(gate):
    """A = ta_hamming_search_cross on s1, B = the two-word route on s2: one host path, the same two slots"""
    L.run_gated(gate, L.hamming_search_cross(101), hsearch_cross_opts(404), b_async=True)
