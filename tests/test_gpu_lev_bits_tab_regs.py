"""-m gpu: the table form of the band kernel with its strings taken from the parked registers (lev_bits_tab_kernel: LDS holds the nibble
tables and nothing else) on the device.  A child process with TA_TUNING and TA_FORCE_TAB_FORM runs every geometry of
tab_regs_cases.GEOMETRIES at 200 pairs through levenshtein_k_batch: the answers equal the oracle's, the kernel is the table kernel and it
was launched with 8,192 bytes of LDS.  And 4,096 pairs at the benchmark's geometry (256 x 256, k = 32), pair by pair against the stride-8
form forced in a second child process (TA_NO_TAB_FORM)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import datagen as Dg
import tab_regs_cases as RC

pytestmark = pytest.mark.gpu

TAB, S8 = "lev_bits_tab_kernel", "lev_bits_s8_kernel<false, true, false>"
N, BIG = 200, 4096
HERE = os.path.dirname(os.path.abspath(__file__))


def big_batch():
    """4,096 pairs of 256 bytes: the 200 pairs of the benchmark's geometry drawn at random, one more substitution in half of them"""
    g = Dg.rng(0x4B16)
    a, b = RC.pairs(256, 256, 32, N)
    idx = g.integers(0, N, size=BIG)
    a, b = a[idx], b[idx]
    rows = np.flatnonzero(g.integers(0, 2, size=BIG))
    b[rows, g.integers(0, 256, size=len(rows))] = g.integers(0, 256, size=len(rows), dtype=np.uint8)
    return a, b


def _run(a, b, k):
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    out = B.levenshtein_k_batch(B.Strings.from_fixed(np.array(a)), B.Strings.from_fixed(np.array(b)), k, RC.LEV).cpu().numpy().view(np.uint32)
    return out, T.last_kernel_name(), T.last_launch_info()


def _tab_child(path):
    """runs in a fresh process started with TA_FORCE_TAB_FORM=1: every geometry, then the big batch"""
    res = {}
    for i, (la, lb, k) in enumerate(RC.GEOMETRIES):
        a, b = RC.pairs(la, lb, k, N)
        out, name, info = _run(a, b, k)
        assert TAB in name, (la, lb, k, name)
        res["out%d" % i] = out
        res["lds%d" % i] = np.array([info["lds_bytes"], info["kernel"], info["pairs_per_wave"], info["grid"]])
    out, name, info = _run(*big_batch(), 32)
    assert TAB in name, name
    res["big"] = out
    res["ldsbig"] = np.array([info["lds_bytes"], info["kernel"], info["pairs_per_wave"], info["grid"]])
    np.savez(path, **res)
    print("tab child ok")


def _s8_child(path):
    """runs in a fresh process started with TA_NO_TAB_FORM=1: the stride-8 kernel's answers for the big batch"""
    out, name, _ = _run(*big_batch(), 32)
    assert S8 in name, name
    np.save(path, out)
    print("s8 child ok")


def _child(fn, path, **env):
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_lev_bits_tab_regs as G; G.%s(%r)" % (os.path.dirname(HERE), HERE, fn, path)
    r = subprocess.run([sys.executable, "-s", "-c", code], env=dict(os.environ, TA_TUNING="1", TA_NO_LATENCY_RULE="1", TA_NO_ONE="1", **env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


@pytest.fixture(scope="module")
def tab_results(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tab_regs") / "tab.npz")
    _child("_tab_child", path, TA_FORCE_TAB_FORM="1")
    return np.load(path)


@pytest.mark.parametrize("i", range(len(RC.GEOMETRIES)), ids=["%dx%d_k%d" % g for g in RC.GEOMETRIES])
def test_geometry(tab_results, i):
    la, lb, k = RC.GEOMETRIES[i]
    got, want = tab_results["out%d" % i], RC.want(la, lb, k, N)
    lds, kernel, ppw, grid = (int(x) for x in tab_results["lds%d" % i])
    print("nlo", RC.nlo(la, lb, k), "lds", lds, "differing", int((got != want).sum()))
    assert (lds, kernel, ppw, grid) == (8192, 3, 64, (N + 63) // 64)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert (want[0::2] != RC.NONE).all() and (want[5::6] == RC.NONE).any()


def test_benchmark_geometry_against_the_stride8_form(tab_results, tmp_path):
    path = str(tmp_path / "s8.npy")
    _child("_s8_child", path, TA_NO_TAB_FORM="1")
    got, s8 = tab_results["big"], np.load(path)
    lds, kernel, ppw, grid = (int(x) for x in tab_results["ldsbig"])
    assert (lds, kernel, ppw, grid) == (8192, 3, 64, BIG // 64)
    print("differing", int((got != s8).sum()), "within k", int((got != RC.NONE).sum()))
    assert np.array_equal(got, s8), np.flatnonzero(got != s8)[:10]
    assert (got != RC.NONE).sum() > BIG // 4 and (got == RC.NONE).sum() > BIG // 8
