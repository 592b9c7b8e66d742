"""The pure route of the distance pass (triple_accel_amd/csrc/lev_route.h: lev_pass_route, lev_select, the exp schedule) against the
cascade, the width-class arithmetic and the two schedule copies it replaced, written out independently, and the GPU spot test's rows as
literals (tests/cpp/lev_route_check.cpp, plain g++); once more as a TA_EXPERIMENTAL build for the pair-sliced kind."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(name, *defines):
    exe = os.path.join(ROOT, "tests", "cpp", "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", *defines, "-I", os.path.join(ROOT, "triple_accel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "lev_route_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name,defines", [("lev_route_check", ()), ("lev_route_check_experimental", ("-DTA_EXPERIMENTAL",))])
def test_lev_pass_route_matches_the_cascade(name, defines):
    out = subprocess.run([build(name, *defines)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "lev route: ok" in out.stdout
