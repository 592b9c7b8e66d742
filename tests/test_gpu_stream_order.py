"""gpu: the threading contract of include/triple_accel_amd.h, asserted entry by entry -- a call that used thread-local scratch records an
event at its end, and a later call of the same thread on ANOTHER stream waits for it before it touches scratch (StreamGuard).

The test is deterministic and never lets two library calls overlap (stream_order_lib.py): call A is enqueued on stream s1 behind a
device-side delay of about 50 ms (torch.cuda._sleep), call B is made on another stream.  If the library ordered B after A, s1 has
nothing pending once B is complete; if it did not, B completes while s1 is still asleep.  Every case
  * makes all of its calls once, with the same shapes, and synchronises, before the gate is armed (scratch growth synchronises);
  * asserts the premise -- A is still pending right before B -- so an A that synchronised internally fails instead of passing for nothing;
  * compares A's and B's answers (different strings) with the oracle, and the route of a call where it is observable;
and the module's streams are chosen by a control: the library's own stream and s2 really overtake a gate on s1.

Part 1 (test_async_call_records): A varies, B is a small ragged levenshtein_k_batch on s2 -- every scratch-using asynchronous route records.
Part 2 (test_single_call_waits, test_async_call_waits): A is levenshtein_exp_batch on 1,024 fixed-length pairs, B varies -- every entry waits.

Every entry point of the header that takes a stream or runs on the thread's stream, and what covers it:
  ta_hamming                              Part 2: a short pair; a pair above TA_HAM_HOST_CHUNK (the chunked form)
  ta_levenshtein_simd_k_with_opts         Part 2: a short pair; a pair on the DP wide kernel
  ta_levenshtein_simd_k, ta_levenshtein, ta_rdamerau                  one-line wrappers of ta_levenshtein_simd_k_with_opts: covered by it
  ta_levenshtein_exp_with_opts, ta_levenshtein_exp, ta_rdamerau_exp   Part 2 (levenshtein_exp); the other two are its wrappers
  ta_levenshtein_trace                    Part 2: register band, trace_widebits, trace_wide
  ta_levenshtein_exp_trace                Part 2
  ta_levenshtein_tokens                   Part 2: coded and wide_pair_u32, each with and without edits
  ta_levenshtein_search_simd_with_opts    Part 2: All and Best
  ta_levenshtein_search                   wrapper of the above (Best): covered by it
  ta_levenshtein_search_first             Part 2
  ta_levenshtein_search_resume            Part 2 (the lazy iterator's second element)
  ta_hamming_search_simd_with_opts, ta_hamming_search                 Part 2 (hamming_search; the former is what it calls)
  ta_hamming_search_naive_with_opts       Part 2 (All mode, a NUL byte in the haystack)
  ta_queue_flush                          Part 2 (with a control of its own: the queue has a stream of its own)
  ta_levenshtein_k_batch                  Part 1: length order (4,096 ragged pairs), unit prefilter, row-blocked kernel with boundary lines
                                          and in its tiled form, DP wide kernel; Part 2: the same and the two no-scratch routes.
                                          Fixed-length batches on the bit-parallel kernels and ragged ones below 4,096 pairs: no
                                          scratch, records nothing by design
  ta_levenshtein_k_batch_alphabet         Part 1 and 2: 16,384 ACGT pairs, a few with another byte
  ta_levenshtein_exp_batch                Part 1 and 2: 1,024 fixed-length pairs (smaller batches synchronise between rounds)
  ta_levenshtein_trace_batch              Part 1 and 2: checkpoint route, record route
  ta_levenshtein_trace_batch_packed       Part 1 and 2: both routes
  ta_levenshtein_k_batch_tokens           Part 1 and 2: with overflow pairs
  ta_levenshtein_exp_batch_tokens         Part 1 and 2: 1,024 pairs and overflow pairs
  ta_levenshtein_trace_batch_tokens       Part 1: WITHOUT overflow pairs -- with them the entry reads their count back and walks them on
                                          the host: it has no asynchronous form then; Part 2: both
  ta_levenshtein_search_batch             Part 1 and 2: the shared-needle scan route; needles beyond 32 bytes.  The exact route with
                                          needles up to 32 bytes below 4,096 pairs: no scratch, records nothing by design
  ta_hamming_search_batch                 Part 1 and 2: 4,096 CSR haystacks (the length order is its only scratch; below: records nothing by design)
  ta_levenshtein_search_cross             Part 1 and 2
  ta_hamming_search_cross                 Part 1 and 2
  ta_hamming_batch                        Part 1 and 2: strings of 64 KiB (the sliced form); Part 2: short strings -- no scratch, records nothing by design
  ta_hamming_dev                          Part 1 and 2: 64 KiB
  ta_levenshtein_cross, ta_levenshtein_cross_with_opts, ta_hamming_cross
                                          Part 2.  With both length bounds known (the only asynchronous form) they take no scratch:
                                          records nothing by design; a CSR side with max_len = 0 takes two words to measure it and synchronises
  ta_levenshtein_search_dev, ta_levenshtein_search_best_dev, ta_levenshtein_search_first_dev, ta_hamming_search_dev_sorted
                                          Part 2, on s2: they read their count back, so they are complete when they return (no asynchronous form)
  ta_hamming_search_dev                   what ta_hamming_search_dev_sorted and the host forms call: covered by them
  ta_search_best_hits_dev                 Part 2, on s2, over records that already lie in HBM (it copies its selection back: complete on return)
  ta_thread_release                       synchronises the device: nothing to order
  ta_*_batch_host, ta_sharded_pairs_*, ta_sharded_haystack_*           worker threads with scratch of their own: out of scope
"""
import pytest

import stream_order_lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gate():
    return L.Gate()


def _id(case):
    return case.__name__


def test_control_the_other_streams_overtake_the_gate(gate):
    """the chosen streams, once more: a gate on s1 alone holds up neither a single call on the library's stream nor work on s2"""
    assert gate.control_sync(gate.s1), "the library's own stream queued up behind s1"
    assert gate.control_async(gate.s2), "s2 queued up behind s1"
    assert L.GATE_MS / 4 <= gate.gate_ms <= L.GATE_MAX_MS, gate.gate_ms


@pytest.mark.parametrize("case", L.PART1, ids=_id)
def test_async_call_records(gate, case):
    """Part 1: A (this case, on s1 behind the gate) took scratch, so it recorded; B (a small ragged k batch on s2) waited for it"""
    L.run_gated(gate, case(101), L.k_small_ragged(202), b_async=True)


@pytest.mark.parametrize("case", L.PART2_SYNC, ids=_id)
def test_single_call_waits(gate, case):
    """Part 2: A = levenshtein_exp_batch on s1 behind the gate; B = a single-call function on the library's own stream: complete when it
    returns, and by then nothing of s1 may be pending"""
    L.run_gated(gate, L.exp_batch(101), case(303), b_async=False)


@pytest.mark.parametrize("case", L.PART2_ASYNC, ids=_id)
def test_async_call_waits(gate, case):
    """Part 2: B = a batch / *_dev call on s2: complete once an event recorded on s2 after it has been synchronised"""
    L.run_gated(gate, L.exp_batch(101), case(404), b_async=True)
