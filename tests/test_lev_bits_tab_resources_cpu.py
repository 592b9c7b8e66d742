"""The table form's kernel (lev_bits_tab_kernel) must fit four wavefronts on a SIMD: hipcc compiles lev_bits_tab.hip for the device alone, to
assembly, with the Makefile's flags, and the kernel's resource metadata (the `amdhsa.kernels` entry, nothing of the instruction stream) must
say at most 128 VGPRs, no scratch and no static LDS (the tables are the dynamic request, 8,192 bytes; the body's table addresses are
absolute).  With the 32 slot-bit constants parked across the column loop the kernel took 157 registers: three wavefronts per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "triple_accel_amd", "csrc")


def makefile_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", arch)
    return flags.split()


def kernel_metadata(asm, name):
    """{key: value} of the kernel's entry in the assembly's amdhsa.kernels list (its `.key: value` lines)"""
    meta = asm[asm.index("amdhsa.kernels:"):]
    entries = re.split(r"\n  - ", meta)
    mine = [e for e in entries if re.search(r"\.name:\s+_ZN2ta\d+%s\w*\s" % name, e)]
    assert len(mine) == 1, [re.findall(r"\.name:\s+(\S+)", e) for e in entries]
    return dict(re.findall(r"^\s+\.(\w+):\s+(\S+)\s*$", mine[0], re.M))


def test_table_kernel_fits_four_wavefronts_per_simd(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path / "lev_bits_tab.s")
    r = subprocess.run([hipcc] + makefile_flags() + ["-Wno-unused-command-line-argument", "-S", "--cuda-device-only", "lev_bits_tab.hip", "-o", out],
                       cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    md = kernel_metadata(open(out).read(), "lev_bits_tab_kernel")
    print({k: md.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
    assert int(md["vgpr_count"]) + int(md.get("agpr_count", 0)) <= 128
    assert int(md["private_segment_fixed_size"]) == 0
    assert int(md["group_segment_fixed_size"]) == 0
