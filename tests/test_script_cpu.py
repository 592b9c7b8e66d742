"""The host half of a traceback, triple_accel_amd/csrc/lev_script.h -- ScriptBuilder (step codes to the run-length edit script), wide_trace_code
and band_trace_code (the DP kernels' record layouts) -- against definitions written out independently (tests/cpp/script_check.cpp, plain g++)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "script_check")


def build():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "triple_accel_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "script_check.cpp"), "-o", EXE])
    return EXE


def test_script_matches_its_definition():
    out = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "script: ok" in out.stdout
