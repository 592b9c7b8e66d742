"""gpu: the threading contract of include/triple_accel_amd.h for ta_levenshtein_cross_tokens, with the gate and the runner of
tests/stream_order_lib.py (see tests/test_gpu_stream_order.py for the method).  With both length bounds known -- its only asynchronous
form -- the entry takes no scratch; a CSR side with max_len = 0 is measured into thread-local scratch (SLOT_CROSS_CTL) under one
synchronisation, so that form has no asynchronous A.  Both forms as B: a call on another stream waits for the gated call's scratch."""
import functools

import pytest

import stream_order_lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gate():
    return L.Gate()


@functools.lru_cache(maxsize=None)
def _d_cross_tokens(seed):
    import cross_tokens_cases as X
    import datagen as Dg
    g = Dg.rng(seed)
    voc = X.vocab("32k")[:16]
    targets = [X.rand_seq(g, voc, int(g.integers(10, 41))) for _ in range(200)]
    queries = [X.edited(g, targets[int(g.integers(200))], i % 3, voc)[:64] for i in range(40)]
    return queries, targets, X.join(queries, targets, 2, L.UNIT)[0]


def cross_tokens(seed, measured):
    torch, T, B = L._mods()
    queries, targets, rows = _d_cross_tokens(seed)
    qs, ts = B.Tokens.from_list(queries), B.Tokens.from_list(targets)
    if measured:
        qs.max_len = ts.max_len = 0

    def check(r):
        q, t, d = B.cross_to_arrays(r[0], r[1])
        assert list(zip(q.tolist(), t.tolist(), d.tolist())) == rows and len(rows) >= 16

    return L.Case(lambda: B.levenshtein_cross_tokens(qs, ts, 2), check, L._name_has("lev_cross_tok_kernel"))


@pytest.mark.parametrize("measured", [False, True], ids=["bounds_given", "bounds_measured"])
def test_async_call_waits(gate, measured):
    """A = levenshtein_exp_batch on s1 behind the gate; B = the token cross entry on s2: complete once an event recorded on s2 after it
    has been synchronised, and by then nothing of s1 may be pending"""
    L.run_gated(gate, L.exp_batch(101), cross_tokens(505, measured), b_async=True)
