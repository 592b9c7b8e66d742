"""The pure host rules of triple_accel_amd/csrc/lev_plan.h -- lev_costs_valid, lev_is_unit, lev_cost_scale / lev_unit_scale, cross_qtile,
lev_wants_length_order -- against their definitions written out independently (tests/cpp/host_rules_check.cpp, plain g++)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "host_rules_check")


def build():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "triple_accel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "host_rules_check.cpp"), "-o", EXE])
    return EXE


def test_host_rules_match_their_definitions():
    out = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host rules: ok" in out.stdout
