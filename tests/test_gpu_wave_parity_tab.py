"""-m gpu: the table form's operations on the device (DevTab, triple_accel_amd/csrc/wave_tab.h) against their host emulation (EmuTab), bit
for bit, over the cases of tab_parity_lib.build_cases(): the SDWA address instructions in all four byte positions, the LDS read and XOR by
absolute address in a block of two wavefronts (the second one's LDS does not start at address 0), and a flip followed by a lookup as the
kernel body issues them."""
import numpy as np
import pytest

import tab_parity_lib as TP

pytestmark = pytest.mark.gpu


def test_table_operations_match_their_emulation():
    import torch
    inp = TP.build_cases()
    n = inp.shape[0]
    d_in = torch.from_numpy(inp.reshape(-1).view(np.int32)).cuda()
    d_out = torch.full((TP.N_OPS * n * 64,), 0x25A5A5A5, dtype=torch.int32, device="cuda")
    rc = TP.dev().ta_tab_parity_run(d_in.data_ptr(), d_out.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, "launch failed: HIP error %d" % rc
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint32).reshape(TP.N_OPS, n, 64)
    want = TP.run_emu(inp)
    for i, name in enumerate(TP.ROWS):
        bad = np.argwhere(got[i] != want[i])
        assert not len(bad), "%s: device != emulation at (case, lane) %s: %08x / %08x" % (
            name, bad[:5].tolist(), got[i][tuple(bad[0])], want[i][tuple(bad[0])])
