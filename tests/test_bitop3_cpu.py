"""bitop3<TT>() (triple_accel_amd/csrc/bitop3.h): the generic path -- what the host and the 64-lane emulation of the kernel bodies run --
against the definition of a truth table, all 256 tables x 8 input rows, and the tables the band kernel uses against their written-out
expressions (tests/cpp/bitop3_check.cpp, plain g++)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build", "bitop3_check")


def build():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "triple_accel_amd", "csrc"),
                           "-I", os.path.join(ROOT, "tests", "emu"), os.path.join(ROOT, "tests", "cpp", "bitop3_check.cpp"), "-o", EXE])
    return EXE


def test_bitop3_generic_path_matches_every_truth_table():
    out = subprocess.run([build()], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bitop3: ok" in out.stdout
