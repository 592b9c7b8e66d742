"""The pure route of the single-haystack hamming_search (triple_accel_amd/csrc/ham_search_plan.h: ham_search_route, the tile rules, the
kernel names) against the launcher's former cascade written out independently, the GPU test's (n, k) -> kernel spot table as literal rows
and the tiles at their edges (tests/cpp/ham_route_check.cpp, plain g++)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "ham_route_check")


def build():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "triple_accel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ham_route_check.cpp"), "-o", EXE])
    return EXE


def test_ham_search_route_matches_the_cascade():
    out = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ham route: ok" in out.stdout
