"""Where the table form's kernels wait for LDS (lev_bits_tab_body.h, column(): the pin).  hipcc compiles lev_bits_tab.hip and
lev_bits_tab_alt.hip for the device alone, to assembly, with the Makefile's flags, and the instruction streams are walked:

(a) the alternative kernel (the depth that does not ship, TA_TAB_DEPTH) keeps the resource line test_lev_bits_tab_resources_cpu.py asks of
    lev_bits_tab_kernel: at most 128 VGPRs + AGPRs, no scratch, no static LDS;
(b) between a lookup (its second ds_read_b32) and the next ds_xor_b32 no s_waitcnt may ask for lgkmcnt below 6 at depth 1 (the four
    flips and the lookup behind the one waited for stay outstanding) or below 12 at depth 2.  Allowed to: the edge columns of the two
    whole spans -- the first one and the last two at depth 1, the first two and the last two at depth 2, where the lead is built and
    runs out -- and every column of the two tail spans, any of which may be the last.  That is 2 * 3 + 2 * 16 = 38 waits at depth 1 and
    2 * 4 + 2 * 16 = 40 at depth 2, and the count is asserted; so is that the whole spans' other columns do wait that way (at least
    2 * 13 and 2 * 12 counted waits), which keeps (b) from passing on a stream without lookups.
    The walk is in text order, so it sees a tail span's waits only where they stand in the same run of text as their lookup.
    The commit before the pin: its assembly holds 96 `s_waitcnt lgkmcnt(0)`, one in every steady-state column; this walk meets 34 waits
    below 6 behind a lookup (all 30 steady-state columns of the two whole spans among them; the tails' stand in blocks of their own) and
    only 2 counted waits where 26 are asked for -- it fails the second assertion.  With the pin: 30 and 28 at depth 1, 20 and 24 at
    depth 2 (the low ones are the tails' and the edges');
(c) the address statements (wave_tab.h, nib_to_byte1) end without an s_nop of their own: no VALU instruction may read a register in the
    slot right behind a sub-dword write to it (LDS instructions may: they are the addresses' readers)."""
import os
import re
import shutil
import subprocess

import pytest

from test_lev_bits_tab_resources_cpu import CSRC, kernel_metadata, makefile_flags

# file, kernel, depth, violations allowed, counted waits at least
KERNELS = [("lev_bits_tab.hip", "lev_bits_tab_kernel"), ("lev_bits_tab_alt.hip", "lev_tab_depth_kernel")]
NEED = {1: 6, 2: 12}
ALLOWED = {1: 2 * 3 + 2 * 16, 2: 2 * 4 + 2 * 16}
STEADY = {1: 2 * 13, 2: 2 * 12}


def depths():
    """(depth of lev_bits_tab.hip's kernel, depth of lev_bits_tab_alt.hip's): LEV_TAB_DEPTH and the other one"""
    body = open(os.path.join(CSRC, "lev_bits_tab_body.h")).read()
    d = int(re.search(r"^constexpr int LEV_TAB_DEPTH = (\d);", body, re.M).group(1))
    assert d in (1, 2)
    return d, 3 - d


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = {}
    for src, _ in KERNELS:
        path = str(tmp_path_factory.mktemp("waits") / (src + ".s"))
        r = subprocess.run([hipcc] + makefile_flags() + ["-Wno-unused-command-line-argument", "-S", "--cuda-device-only", src, "-o", path],
                           cwd=CSRC, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        out[src] = open(path).read()
    return out


def instructions(asm, name):
    """the instruction lines of the one function whose mangled name holds `name`, in text order"""
    starts = re.findall(r"^(_ZN2ta\w*%s\w*):\s" % name, asm, re.M)
    assert len(starts) == 1, starts
    body = asm[asm.index(starts[0] + ":"):]
    body = body[:body.index(".Lfunc_end")]
    return [ln.strip() for ln in body.splitlines() if re.match(r"^\t[a-z]", ln)]


def walk_waits(ins, need):
    """-> (waits below `need` between a lookup and the next ds_xor_b32, waits at `need` or above there)"""
    low = counted = reads = 0
    for cur in ins:
        if cur.startswith("ds_read_b32"):
            reads += 1                                  # (the two reads of a lookup need not be neighbours)
        elif cur.startswith("ds_xor_b32"):
            reads = 0
        elif reads >= 2 and cur.startswith("s_waitcnt"):
            m = re.search(r"lgkmcnt\((\d+)\)", cur)
            if m and int(m.group(1)) < need:
                low += 1
            elif m:
                counted += 1
    return low, counted


@pytest.mark.parametrize("which", [0, 1], ids=["shipped", "alternative"])
def test_a_column_waits_behind_the_next_columns_lds_operations(assembly, which):
    src, name = KERNELS[which]
    depth = depths()[which]
    low, counted = walk_waits(instructions(assembly[src], name), NEED[depth])
    print(src, "depth", depth, "waits below lgkmcnt(%d) behind a lookup:" % NEED[depth], low, "allowed", ALLOWED[depth], "; counted waits:", counted)
    assert low <= ALLOWED[depth]
    assert counted >= STEADY[depth]


def test_alternative_kernel_fits_four_wavefronts_per_simd(assembly):
    md = kernel_metadata(assembly["lev_bits_tab_alt.hip"], "lev_tab_depth_kernel")
    print({k: md.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")})
    assert int(md["vgpr_count"]) + int(md.get("agpr_count", 0)) <= 128
    assert int(md["private_segment_fixed_size"]) == 0
    assert int(md["group_segment_fixed_size"]) == 0
    assert len(re.findall(r"^_ZN2ta\w*lev_bits_tab_kernel\w*:\s", assembly["lev_bits_tab_alt.hip"], re.M)) == 0


@pytest.mark.parametrize("which", [0, 1], ids=["shipped", "alternative"])
def test_no_valu_instruction_reads_an_address_in_the_slot_behind_its_write(assembly, which):
    src, name = KERNELS[which]
    ins = instructions(assembly[src], name)
    writes = 0
    for cur, nxt in zip(ins, ins[1:]):
        m = re.match(r"v_\w+_sdwa (v\d+), .*dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE", cur)
        if not m:
            continue
        writes += 1
        if nxt.startswith("v_"):
            assert not re.search(r"\b%s\b" % m.group(1), nxt), (cur, nxt)
    print(src, "sub-dword writes checked:", writes)
    assert writes >= 2 * 2 * 16 * 6 - 64          # six per column of four spans, less the lookups past a span's end
