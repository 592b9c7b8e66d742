"""-m gpu: the table form of the band kernel at both depths of its LDS stream (lev_bits_tab_body.h, LevBitsTab's DEPTH): the kernel that
ships, lev_bits_tab_kernel, and the other depth's, lev_tab_depth_kernel<d> of lev_bits_tab_alt.hip, which TA_TAB_DEPTH=d selects under
TA_TUNING.  A fresh child process per TA_TAB_DEPTH value with TA_TUNING and TA_FORCE_TAB_FORM, as in test_gpu_lev_bits_tab_occupancy.py;
each runs every shape of tab_depth_cases.py (tails of 1, 2, 3, 15 and 16 columns in both phases, whole spans only; `a` as long as `b`,
shorter, longer; k = 24 and 32; 101 pairs) and asserts the kernel's name after every launch, so a shape outside the form's domain fails
there.  The answers are compared one by one with the oracle."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import tab_depth_cases as DC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHIPPED = int(re.search(r"^constexpr int LEV_TAB_DEPTH = (\d);", open(os.path.join(os.path.dirname(HERE), "triple_accel_amd", "csrc", "lev_bits_tab_body.h")).read(), re.M).group(1))


def kernel_name(depth):
    return "lev_bits_tab_kernel" if depth == SHIPPED else "lev_tab_depth_kernel<%d>" % depth


def _depth_child(path, depth):
    """runs in a fresh process started with TA_TUNING=1 TA_FORCE_TAB_FORM=1 TA_TAB_DEPTH=depth"""
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    res = {}
    for la, lb, k in DC.SHAPES:
        a, b = DC.pairs(la, lb)
        out = B.levenshtein_k_batch(B.Strings.from_fixed(np.array(a)), B.Strings.from_fixed(np.array(b)), k, DC.LEV).cpu().numpy().view(np.uint32)
        name, info = T.last_kernel_name(), T.last_launch_info()
        assert name == kernel_name(depth), (la, lb, k, name)
        assert (info["lds_bytes"], info["kernel"], info["pairs_per_wave"], info["grid"]) == (8192, 3, 64, 2), info
        res["%d_%d_%d" % (la, lb, k)] = out
    np.savez(path, **res)
    print("depth child ok")


@pytest.fixture(scope="module", params=[1, 2])
def depth_results(request, tmp_path_factory):
    depth = request.param
    path = str(tmp_path_factory.mktemp("tab_depth") / ("depth%d.npz" % depth))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_lev_bits_tab_depth as G; G._depth_child(%r, %r)" % (os.path.dirname(HERE), HERE, path, depth)
    r = subprocess.run([sys.executable, "-s", "-c", code],
                       env=dict(os.environ, TA_TUNING="1", TA_NO_LATENCY_RULE="1", TA_NO_ONE="1", TA_FORCE_TAB_FORM="1", TA_TAB_DEPTH=str(depth)),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
    return depth, np.load(path)


def test_every_shape_against_the_oracle(depth_results):
    depth, res = depth_results
    bad = []
    for la, lb, k in DC.SHAPES:
        got, want = res["%d_%d_%d" % (la, lb, k)], DC.want(la, lb, k)
        DC.check_shares(want)
        if not np.array_equal(got, want):
            bad.append((la, lb, k, np.flatnonzero(got != want)[:5].tolist()))
    print("depth", depth, kernel_name(depth), len(DC.SHAPES), "shapes,", len(bad), "differ")
    assert not bad, bad[:10]
