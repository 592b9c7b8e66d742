"""Every device wave primitive against its host emulation, bit for bit (tests/wave_parity/).

The edge-aimed suites (test_emu_*.py, the emu_*batch and emu_tokens suites) run the kernel bodies on EmuWave; they speak for the HIP
kernels only as far as EmuWave::op == DevWave::op, operation by operation.  Here ONE launch runs WaveOps<DevWave> over the cases of
wave_parity_lib.build_cases() (four wavefronts per block, each its own slice of the cases), the host runs WaveOps<EmuWave> over the same
buffers, and the outputs must be equal in every lane of every case of every op.  Left out, as statements about the contract (wave.h):
lane 0 of from_lower0 / lane 63 of from_upper0, first_u32 under an empty predicate (the body does not call it then), and the primitives
without an observable value (wave_parity_lib.EXCLUDED).  The order of an append_u32 list is not defined: counter and sorted list."""
import numpy as np
import pytest

import wave_parity_lib as WP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def both():
    import torch
    inp, hdr, tags = WP.build_cases()
    names = WP.op_names()
    assert names == WP.op_names(WP.dev())
    n = inp.shape[0]
    d_in = torch.from_numpy(inp.reshape(-1).view(np.int32)).cuda()
    d_hdr = torch.from_numpy(hdr.view(np.int32)).cuda()
    d_out = torch.from_numpy(WP.new_out(n, names).reshape(-1).view(np.int32)).cuda()
    assert d_in.data_ptr() % 256 == 0 and d_hdr.data_ptr() % 8 == 0
    rc = WP.dev().ta_wave_parity_run(d_in.data_ptr(), d_hdr.data_ptr(), d_out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, "launch failed: HIP error %d" % rc
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(len(names), n, 64)
    want = WP.run_emu(inp, hdr, names)
    return inp, names, WP.canonical(got, names), WP.canonical(want, names)


def is_composition(name):
    return name.startswith("comp:")


def test_every_primitive_matches_its_emulation(both):
    inp, names, got, want = both
    lines = WP.mismatches(got, want, names, inp, which=lambda n: not is_composition(n))
    assert not lines, "device != emulation\n" + "\n".join(lines)


def test_compositions_match_their_emulation(both):
    """the asm statements back to back as the bodies write them: the carry chain in a loop with a wave-uniform counter and exit (SCC / VCC
    live across the statements), the and_or and bfi_k gathers, DPP after DPP, wave_max after a select"""
    inp, names, got, want = both
    assert sum(map(is_composition, names)) == 9
    lines = WP.mismatches(got, want, names, inp, which=is_composition)
    assert not lines, "device != emulation\n" + "\n".join(lines)
