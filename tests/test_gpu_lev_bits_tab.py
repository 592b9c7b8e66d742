"""-m gpu: the table form of the band kernel (lev_bits_tab_kernel: the match vector from two per-pair nibble tables in LDS) on the device,
answer by answer against the CPU oracle.  Under TA_FORCE_TAB_FORM=1 the geometries, pair counts and alphabets of tab_cases.py, and the same
batches re-hosted by layout_arena (a shifted blob, padded strides, guard bands round the output); with no switch the route itself:
262,144 pairs of 256 bytes take the table form and equal the stride-8 kernel's answers pair by pair (TA_NO_TAB_FORM=1 in a fresh child
process) and the oracle's on 4,000 sampled pairs, 262,143 pairs keep the stride-8 kernel; and three passes captured into one graph."""
import os
import subprocess
import sys

import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O
import tab_cases as TC

pytestmark = pytest.mark.gpu

TAB, S8 = "lev_bits_tab_kernel", "lev_bits_s8_kernel<false, true, false>"
BIG = 262144


@pytest.fixture
def forced(monkeypatch):
    """TA_NO_LATENCY_RULE=1 as in test_gpu_lev_bits_core.py (the choice a big batch gets), and the table form at any pair count"""
    monkeypatch.setenv("TA_NO_LATENCY_RULE", "1")
    monkeypatch.setenv("TA_FORCE_TAB_FORM", "1")


def gpu(a, b, k, costs):
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    out = B.levenshtein_k_batch(B.Strings.from_fixed(np.array(a)), B.Strings.from_fixed(np.array(b)), k, costs).cpu().numpy().view(np.uint32)
    return out, T.last_kernel_name(), T.last_launch_info()


@pytest.mark.parametrize("kind", ["core", "alpha"])
@pytest.mark.parametrize("la,lb,k,costs", TC.SHAPES)
def test_shapes(forced, la, lb, k, costs, kind):
    a, b = (TC.core_pairs if kind == "core" else TC.alphabet_pairs)(la, lb, k // costs[0])
    got, name, info = gpu(a, b, k, costs)
    assert TAB in name, name
    assert info["kernel"] == 3 and info["diags_per_lane"] == 33 and info["pairs_per_wave"] == 64, info
    want = TC.want(kind, la, lb, k, costs)
    assert (want != TC.NONE).sum() >= 20 and (want == TC.NONE).sum() >= 20, "the batch holds answers within k and beyond it"
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


@pytest.mark.parametrize("n", TC.PAIR_COUNTS)
def test_pair_counts(forced, n, monkeypatch):
    """n = 1: a wavefront with one valid lane.  A lone pair is otherwise the single-pair kernel's (lev_one_kernel, chosen in front of the
    band kernels' launcher); TA_NO_ONE=1 keeps it away, so the table form runs here at every n and its name is asserted at every n."""
    monkeypatch.setenv("TA_NO_ONE", "1")
    a, b = TC.core_pairs(256, 256, 32)
    got, name, info = gpu(a[:n], b[:n], 32, TC.LEV)
    assert TAB in name, name
    assert info["kernel"] == 3 and info["diags_per_lane"] == 33 and info["pairs_per_wave"] == 64 and info["grid"] == (n + 63) // 64, info
    assert np.array_equal(got, TC.want("core", 256, 256, 32, TC.LEV)[:n])


LAYOUTS = [(0, 0, "ff"), (5, 3, "echo"), (13, 17, "0c"), (1, 128, "00")]      # (blob shift, stride padding, what the gaps hold)


@pytest.mark.parametrize("kind", ["core", "alpha"])
@pytest.mark.parametrize("la,lb,k,costs", TC.SHAPES)
def test_hostile_layouts(forced, la, lb, k, costs, kind):
    """the same batches as test_shapes, re-hosted: the blob `shift` bytes behind a 256-byte boundary, strides of len + pad with the gaps
    filled, the output between guard bands -- identical answers, intact guards, the same kernel"""
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    import layout_arena as A
    a, b = (TC.core_pairs if kind == "core" else TC.alphabet_pairs)(la, lb, k // costs[0])
    want = TC.want(kind, la, lb, k, costs)
    for shift, pad, fill in LAYOUTS:
        ha = A.host_side(np.array(a), A.Layout("strided", shift=shift, pad=pad, fill=fill), partner=np.array(b))
        hb = A.host_side(np.array(b), A.Layout("strided", shift=(shift * 7) % 16, pad=pad, fill=fill), partner=np.array(a), seed=1)
        g = A.guarded(a.shape[0], torch.int32)
        B.levenshtein_k_batch(A.to_strings(ha), A.to_strings(hb), k, costs, out=g.view)
        g.check()
        assert TAB in T.last_kernel_name(), T.last_kernel_name()
        got = g.numpy().view(np.uint32)
        assert np.array_equal(got, want), (shift, pad, fill, np.flatnonzero(got != want)[:10])


def big_batch(n):
    """n pairs of 256 bytes: the core and the alphabet pairs drawn at random, one more substitution in half of them"""
    g = Dg.rng(0xB16)
    ca, cb = TC.core_pairs(256, 256, 32)
    aa, ab = TC.alphabet_pairs(256, 256, 32)
    base_a, base_b = np.concatenate([ca, aa]), np.concatenate([cb, ab])
    idx = g.integers(0, len(base_a), size=n)
    a, b = base_a[idx], base_b[idx]
    rows = np.flatnonzero(g.integers(0, 2, size=n))
    b[rows, g.integers(0, 256, size=len(rows))] = g.integers(0, 256, size=len(rows), dtype=np.uint8)
    return a, b


def _s8_child(path):
    """runs in a fresh process started with TA_NO_TAB_FORM=1: the stride-8 kernel's answers for big_batch(BIG)"""
    import triple_accel_amd as T
    a, b = big_batch(BIG)
    got, name, _ = gpu(a, b, 32, TC.LEV)
    assert S8 in name, name
    np.save(path, got)
    print("s8 child ok", T.version())


def test_default_route_takes_the_table_form_from_262144_pairs(tmp_path):
    a, b = big_batch(BIG)
    got, name, info = gpu(a, b, 32, TC.LEV)
    assert TAB in name, name
    assert info["kernel"] == 3 and info["diags_per_lane"] == 33 and info["pairs_per_wave"] == 64, info
    # one pair fewer: the stride-8 kernel, the same answers
    got1, name1, _ = gpu(a[:BIG - 1], b[:BIG - 1], 32, TC.LEV)
    assert S8 in name1, name1
    assert np.array_equal(got1, got[:BIG - 1])
    # the oracle on 4,000 sampled pairs
    pick = Dg.rng(0x5A3).choice(BIG, size=4000, replace=False)
    want = O.levenshtein_k_batch(O.csr_from_fixed(a[pick]), O.csr_from_fixed(b[pick]), 32, TC.LEV)
    assert np.array_equal(got[pick], want), np.flatnonzero(got[pick] != want)[:10]
    assert (want == 32).any() and (want == TC.NONE).any() and (want == 0).any()
    # the stride-8 kernel on the whole batch, pair by pair: the switch is honoured under TA_TUNING, in a fresh process
    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp_path / "s8.npy")
    env = dict(os.environ, TA_NO_TAB_FORM="1", TA_TUNING="1")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_lev_bits_tab as G; G._s8_child(%r)" % (os.path.dirname(here), here, path)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "s8 child ok" in r.stdout, r.stderr[-3000:]
    assert np.array_equal(np.load(path), got)


def test_three_passes_in_one_graph(forced):
    """the timed path of the benchmark replays a graph: three passes captured into one, replayed on new bytes"""
    import torch
    from triple_accel_amd import batch as B
    a, b = TC.core_pairs(256, 256, 32)
    aa, ab = TC.alphabet_pairs(256, 256, 32)
    sa, sb = B.Strings.from_fixed(np.array(a)), B.Strings.from_fixed(np.array(b))
    ta, tb = sa.blob[:a.size], sb.blob[:b.size]            # the bytes the captured passes read
    outs = [torch.empty(a.shape[0], dtype=torch.int32, device="cuda") for _ in range(3)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        direct = B.levenshtein_k_batch(sa, sb, 32, TC.LEV).cpu().numpy().view(np.uint32)      # (sizes the scratch outside the capture)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            for o in outs:
                B.levenshtein_k_batch(sa, sb, 32, TC.LEV, out=o)
        for xa, xb, kind in ((a, b, "core"), (aa, ab, "alpha")):
            ta.copy_(torch.from_numpy(np.array(xa)).reshape(-1))
            tb.copy_(torch.from_numpy(np.array(xb)).reshape(-1))
            for o in outs:
                o.fill_(-7)
            graph.replay()
            s.synchronize()
            want = TC.want(kind, 256, 256, 32, TC.LEV)
            for o in outs:
                assert np.array_equal(o.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(direct, TC.want("core", 256, 256, 32, TC.LEV))
