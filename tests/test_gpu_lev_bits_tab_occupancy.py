"""-m gpu: the table form of the band kernel (lev_bits_tab_kernel) at four wavefronts per SIMD, 16 per CU.  Fresh child processes with
TA_TUNING and TA_FORCE_TAB_FORM, as in test_gpu_lev_bits_tab_regs.py:
(a) 4,096 + 37 mutated pairs of 256 bytes, k = 32 (a ragged last wavefront, more than one wavefront per SIMD on a few CUs), and the same
    with `a` cut to 250 bytes (nlo = 13: the window starts inside a piece), answer by answer against the oracle;
(b) 262,144 + 64 random and mutated pairs -- one wavefront more than the 256 CUs x 16 wavefronts that are resident at once, so the
    dispatcher refills -- pair by pair against the stride-8 form forced in a second child (TA_NO_TAB_FORM);
(c) the batches of (a) with TA_TAB_LDS_PAD_KB=5, the occupancy probe at 12 wavefronts per CU: the same answers as (a)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

pytestmark = pytest.mark.gpu

TAB, S8 = "lev_bits_tab_kernel", "lev_bits_s8_kernel<false, true, false>"
LEV = (1, 1, 0, None)
NONE = 0xFFFFFFFF
K = 32
N_A = 4096 + 37
N_B = 262144 + 64
PAD_KB = 5                                  # 8,192 + 5,120 bytes per wavefront: 12 of them in a CU's 160 KB
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def batch_a():
    """N_A pairs of 256 bytes, 10..20 edits apart, every fifth `b` replaced by random bytes; and `a` cut to 250 bytes.  Read only."""
    a, b = Dg.pairs_mutated_fixed(0x0CC1, N_A, 256, 20)
    b[4::5] = Dg.random_bytes(Dg.rng(0x0CC2), len(b[4::5]) * 256).reshape(-1, 256)
    a250 = np.ascontiguousarray(a[:, :250])
    for x in (a, b, a250):
        x.setflags(write=False)
    return (a, b), (a250, b)


@functools.lru_cache(maxsize=None)
def batch_b():
    """N_B pairs of 256 bytes: the pairs of batch_a drawn at random, one more substitution in half of them; every third pair random"""
    g = Dg.rng(0x0CC3)
    (a0, b0), _ = batch_a()
    idx = g.integers(0, N_A, size=N_B)
    a, b = a0[idx], b0[idx]
    rows = np.flatnonzero(g.integers(0, 2, size=N_B))
    b[rows, g.integers(0, 256, size=len(rows))] = g.integers(0, 256, size=len(rows), dtype=np.uint8)
    b[2::3] = Dg.random_bytes(g, len(b[2::3]) * 256).reshape(-1, 256)
    return a, b


@functools.lru_cache(maxsize=None)
def want_a():
    return tuple(O.levenshtein_k_batch(O.csr_from_fixed(np.array(a)), O.csr_from_fixed(np.array(b)), K, LEV) for a, b in batch_a())


def _run(a, b):
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    out = B.levenshtein_k_batch(B.Strings.from_fixed(np.array(a)), B.Strings.from_fixed(np.array(b)), K, LEV).cpu().numpy().view(np.uint32)
    info = T.last_launch_info()
    return out, T.last_kernel_name(), np.array([info["lds_bytes"], info["kernel"], info["pairs_per_wave"], info["grid"]])


def _tab_child(path, big):
    """runs in a fresh process started with TA_FORCE_TAB_FORM=1 (and the probe's pad, or none): the batches of (a), then (b) if asked"""
    res = {}
    for i, (a, b) in enumerate(batch_a()):
        res["a%d" % i], name, res["info_a%d" % i] = _run(a, b)
        assert TAB in name, name
    if big:
        res["b"], name, res["info_b"] = _run(*batch_b())
        assert TAB in name, name
    np.savez(path, **res)
    print("tab child ok")


def _s8_child(path, _big):
    """runs in a fresh process started with TA_NO_TAB_FORM=1: the stride-8 kernel's answers for (b)"""
    out, name, _ = _run(*batch_b())
    assert S8 in name, name
    np.save(path, out)
    print("s8 child ok")


def _child(fn, path, big, **env):
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_lev_bits_tab_occupancy as G; G.%s(%r, %r)" % (os.path.dirname(HERE), HERE, fn, path, big)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=dict(os.environ, TA_TUNING="1", TA_NO_LATENCY_RULE="1", TA_NO_ONE="1", **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


@pytest.fixture(scope="module")
def tab_results(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tab_occupancy") / "tab.npz")
    _child("_tab_child", path, True, TA_FORCE_TAB_FORM="1")
    return np.load(path)


@pytest.mark.parametrize("i", [0, 1], ids=["256x256", "250x256_nlo13"])
def test_ragged_batch_against_the_oracle(tab_results, i):
    got, want = tab_results["a%d" % i], want_a()[i]
    print("differing", int((got != want).sum()), "within k", int((want != NONE).sum()), "beyond", int((want == NONE).sum()))
    assert tuple(int(x) for x in tab_results["info_a%d" % i]) == (8192, 3, 64, (N_A + 63) // 64)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert (want != NONE).sum() > N_A // 2 and (want == NONE).sum() > N_A // 8


def test_one_wavefront_past_the_resident_set_against_the_stride8_form(tab_results, tmp_path):
    path = str(tmp_path / "s8.npy")
    _child("_s8_child", path, True, TA_NO_TAB_FORM="1")
    got, s8 = tab_results["b"], np.load(path)
    print("differing", int((got != s8).sum()), "within k", int((got != NONE).sum()))
    assert tuple(int(x) for x in tab_results["info_b"]) == (8192, 3, 64, N_B // 64)
    assert N_B // 64 == 256 * 16 + 1
    assert np.array_equal(got, s8), np.flatnonzero(got != s8)[:10]
    assert (got != NONE).sum() > N_B // 4 and (got == NONE).sum() > N_B // 8


def test_probe_at_12_wavefronts_per_cu_gives_the_same_answers(tab_results, tmp_path):
    path = str(tmp_path / "pad.npz")
    _child("_tab_child", path, False, TA_FORCE_TAB_FORM="1", TA_TAB_LDS_PAD_KB=str(PAD_KB))
    pad = np.load(path)
    for i in (0, 1):
        assert tuple(int(x) for x in pad["info_a%d" % i]) == (8192 + 1024 * PAD_KB, 3, 64, (N_A + 63) // 64)
        assert (160 * 1024) // (8192 + 1024 * PAD_KB) == 12
        assert np.array_equal(pad["a%d" % i], tab_results["a%d" % i]), np.flatnonzero(pad["a%d" % i] != tab_results["a%d" % i])[:10]
