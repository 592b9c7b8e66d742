"""-m gpu: hamming of long strings, every pair sliced across the chip (ham_long.hip) -- ta_hamming_batch on the sliced
route (strided and CSR, natural and forced), ta_hamming_dev, the chunked host entry and one device-set row.  Every answer is compared
with numpy's (a != b).sum() and the oracle's hamming; every test asserts the kernel name the call left, so none can pass on the other
route.  TA_HAM_SLICE=1024 (the smallest slice: many slices from short strings) except where the default is the point; strings below the
rule's 64 KiB reach the sliced form through TA_FORCE_HAM_SLICED=1."""
import numpy as np
import pytest

import datagen as Dg
import layout_arena as A
import oracle_lib as O

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
NEW, OLD = "ham_long_kernel", "hamming_batch_kernel"
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _mods():
    import torch
    import triple_accel_amd as T
    from triple_accel_amd import batch as B
    return torch, T, B


def _pair(g, n, rate=0.1):
    a = g.integers(0, 256, n, dtype=np.uint8)
    b = a.copy()
    hit = g.random(n) < rate
    b[hit] ^= g.integers(1, 256, int(hit.sum()), dtype=np.uint8)
    return a, b


def _want(rows_a, rows_b):
    """numpy's count per pair (TA_NONE where the lengths differ), checked against the oracle's hamming_batch"""
    w = np.array([int((np.frombuffer(x, np.uint8) != np.frombuffer(y, np.uint8)).sum()) if len(x) == len(y) else NONE
                  for x, y in zip(rows_a, rows_b)], dtype=np.uint32)
    assert np.array_equal(w, O.hamming_batch(O.csr_from_list(rows_a), O.csr_from_list(rows_b)))
    return w


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _run(B, T, sa, sb, n):
    """hamming_batch into a guarded, garbage-filled output -> (answers, kernel name)"""
    import torch
    out = A.guarded(n, torch.int32)
    B.hamming_batch(sa, sb, out=out.view)
    name = T.last_kernel_name()
    out.check()
    assert not out.unwritten().any()
    return out.numpy().view(np.uint32), name


def _fixed(B, rows):
    return B.Strings.from_fixed(np.frombuffer(b"".join(rows), np.uint8).reshape(len(rows), len(rows[0])).copy())


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 2 * 1024 + 15, 7 * 1024 + 1])
def test_strided_one_pair(monkeypatch, n):
    """one pair at every length around the slice: on the route the rule gives it (one wavefront: below 64 KiB) and forced onto the sliced one"""
    torch, T, B = _mods()
    monkeypatch.setenv("TA_HAM_SLICE", "1024")
    a, b = _pair(Dg.rng(0x7100 + n), n)
    w = _want([a.tobytes()], [b.tobytes()])
    sa, sb = _fixed(B, [a.tobytes()]), _fixed(B, [b.tobytes()])
    got, name = _run(B, T, sa, sb, 1)
    assert got.tolist() == w.tolist() and name == OLD, (n, got, w, name)
    monkeypatch.setenv("TA_FORCE_HAM_SLICED", "1")
    got, name = _run(B, T, sa, sb, 1)
    assert got.tolist() == w.tolist() and name == NEW, (n, got, w, name)
    assert T.hamming(a.tobytes(), b.tobytes()) == int(w[0])                       # the host entry, forced the same way


@pytest.mark.parametrize("n,forced", [(3 * 16384 + 17, True), (65535, False), (65536, False), (4 * 16384 + 17, False)])
def test_strided_one_pair_at_the_default_slice(monkeypatch, n, forced):
    """slices of 16 KiB: 3 S + 17 bytes forced onto the sliced form, and the rule's own threshold -- 65,535 bytes stay on one wavefront"""
    torch, T, B = _mods()
    if forced:
        monkeypatch.setenv("TA_FORCE_HAM_SLICED", "1")
    a, b = _pair(Dg.rng(0x7200 + n), n, 0.3)
    b[-1] ^= 0x0C
    b[16384] = a[16384] ^ 1
    w = _want([a.tobytes()], [b.tobytes()])
    got, name = _run(B, T, _fixed(B, [a.tobytes()]), _fixed(B, [b.tobytes()]), 1)
    assert got.tolist() == w.tolist() and name == (NEW if forced or n >= 65536 else OLD), (got, w, name)


@pytest.mark.parametrize("form", ["pad", "overlap", "shared"])
def test_strided_three_pairs_of_5000(monkeypatch, form):
    """stride > len, stride < len (overlapping windows of one sequence) and stride = 0 (one string against three), the two blobs at
    different odd alignments with hostile bytes around them"""
    torch, T, B = _mods()
    monkeypatch.setenv("TA_HAM_SLICE", "1024")
    monkeypatch.setenv("TA_FORCE_HAM_SLICED", "1")
    g = Dg.rng(0x7300 + len(form))
    rows_a = [bytes(g.choice(ACGT, 5000)) for _ in range(3)]
    rows_b = [bytes(g.choice(ACGT, 5000)) for _ in range(3)]
    if form == "pad":
        ha = A.host_side(rows_a, A.Layout("strided", shift=1, pad=61, fill="echo"), partner=rows_b)
        hb = A.host_side(rows_b, A.Layout("strided", shift=13, pad=3, fill="0c"), partner=rows_a)
    elif form == "overlap":
        ha = A.host_side(rows_a, A.Layout("overlap", shift=3, stride=7, fill="ff"))
        hb = A.host_side(rows_b, A.Layout("overlap", shift=15, stride=1, fill="00"))
    else:
        ha = A.host_side(rows_a[:1], A.Layout("shared", shift=17, fill="echo"), n=3, partner=rows_b)
        hb = A.host_side(rows_b, A.Layout("strided", shift=63, pad=1, fill="nul"), partner=rows_a[:1] * 3)
    w = _want(ha.oracle, hb.oracle)
    assert len(set(w.tolist())) == 3
    got, name = _run(B, T, A.to_strings(ha), A.to_strings(hb), 3)
    assert got.tolist() == w.tolist() and name == NEW, (form, got, w, name)
    got, name = _run(B, T, A.to_strings(hb), A.to_strings(ha), 3)
    assert got.tolist() == w.tolist() and name == NEW, (form, got, w, name)


def _ragged(g):
    lens = [0, 5, 1024, 7 * 1024 + 3, 1, 2 * 1024, 40000]
    rows_a = [bytes(g.choice(ACGT, m)) for m in lens]
    rows_b = [bytes(np.where(g.random(m) < 0.2, ord("N"), np.frombuffer(s, np.uint8)).astype(np.uint8)) for m, s in zip(lens, rows_a)]
    rows_b[3] = rows_b[3][:-1]                                                    # unequal lengths in the middle: TA_NONE there only
    return rows_a, rows_b


@pytest.mark.parametrize("fill", ["ff", "echo", "0c"])
def test_csr_with_and_without_a_length_hint(monkeypatch, fill):
    """the device-side plan: empty pairs, a pair of unequal lengths, off[0] > 0, odd and different alignments, hostile bytes around the
    strings.  Without a max_len hint the rule slices the batch (its lengths are unknown); with the hint (40,000 < 64 KiB) it keeps one
    wavefront per pair, and forced it is sliced again: the same answers every time"""
    torch, T, B = _mods()
    monkeypatch.setenv("TA_HAM_SLICE", "1024")
    rows_a, rows_b = _ragged(Dg.rng(0x7400))
    w = _want(rows_a, rows_b)
    assert (w == NONE).tolist() == [False, False, False, True, False, False, False] and w[6] > 1000
    ha = A.host_side(rows_a, A.Layout("csr", shift=3, lead=5, fill=fill), partner=rows_b)
    hb = A.host_side(rows_b, A.Layout("csr", shift=15, lead=0, fill=fill), partner=rows_a, seed=1)
    for hint, force, kernel in ((False, None, NEW), (True, None, OLD), (True, "1", NEW), (False, "0", OLD)):
        sa, sb = A.to_strings(ha), A.to_strings(hb)
        if not hint:
            sa.max_len = sb.max_len = 0
        if force is None:
            monkeypatch.delenv("TA_FORCE_HAM_SLICED", raising=False)
        else:
            monkeypatch.setenv("TA_FORCE_HAM_SLICED", force)
        got, name = _run(B, T, sa, sb, len(rows_a))
        assert got.tolist() == w.tolist() and name == kernel, (hint, force, got, w, name)
    monkeypatch.setenv("TA_FORCE_HAM_SLICED", "1")
    hv = A.host_side(rows_a, A.Layout("csr_view", shift=127, fill="ff"))           # offsets inside a larger batch's
    got, name = _run(B, T, A.to_strings(hv), A.to_strings(hb), len(rows_a))
    assert got.tolist() == w.tolist() and name == NEW
    # a CSR side against a strided one: the strided side's length is the hint
    seven = [rows_a[3]] * 3
    got, name = _run(B, T, B.Strings.from_list(seven), _fixed(B, [rows_b[5] + rows_b[6][:5123]] * 3), 3)
    assert got.tolist() == _want(seven, [rows_b[5] + rows_b[6][:5123]] * 3).tolist() and name == NEW


def test_forced_old_against_forced_new(monkeypatch):
    torch, T, B = _mods()
    monkeypatch.setenv("TA_HAM_SLICE", "1024")
    g = Dg.rng(0x7500)
    a = g.integers(0, 256, (300, 5000), dtype=np.uint8)
    b = a.copy()
    hit = g.random(a.shape) < g.random((300, 1)) * 0.5
    b[hit] = g.integers(0, 256, int(hit.sum()), dtype=np.uint8)
    w = (a != b).sum(axis=1).astype(np.uint32)
    assert np.array_equal(w, O.hamming_batch(O.csr_from_fixed(a), O.csr_from_fixed(b))) and len(set(w.tolist())) > 100
    sa, sb = B.Strings.from_fixed(a), B.Strings.from_fixed(b)
    got = {}
    for force, kernel in (("0", OLD), ("1", NEW)):
        monkeypatch.setenv("TA_FORCE_HAM_SLICED", force)
        got[force], name = _run(B, T, sa, sb, 300)
        assert name == kernel, (force, name)
    assert np.array_equal(got["0"], got["1"]) and np.array_equal(got["1"], w)
    monkeypatch.delenv("TA_FORCE_HAM_SLICED")
    natural, name = _run(B, T, sa, sb, 300)                                       # 5,000 bytes: below the rule's 64 KiB
    assert name == OLD and np.array_equal(natural, w)
    ca, cb = B.Strings.from_list([r.tobytes() for r in a]), B.Strings.from_list([r.tobytes() for r in b])
    natural, name = _run(B, T, ca, cb, 300)                                       # the same as a CSR batch with its hint
    assert name == OLD and np.array_equal(natural, w)
    monkeypatch.setenv("TA_FORCE_HAM_SLICED", "1")
    forced, name = _run(B, T, ca, cb, 300)                                        # ... and through the plan
    assert name == NEW and np.array_equal(forced, w)


def _view(torch, data, offset, fill):
    """`data` as a 1-D view at storage offset `offset` of a tensor that holds `fill` everywhere else"""
    t = torch.full((len(data) + offset + 32,), fill, dtype=torch.uint8, device="cuda")
    v = t[offset:offset + len(data)]
    v.copy_(torch.from_numpy(data))
    assert v.storage_offset() == offset and v.is_contiguous()
    return v


@pytest.mark.parametrize("n,forced", [(0, True), (1, True), (1000, False), (1025, True), (5 * 1024 + 7, True), (5 * 1024 + 7, False),
                                      (65535, False), (65536, False), (100000, False)])
def test_hamming_dev_on_views_at_odd_storage_offsets(monkeypatch, n, forced):
    torch, T, B = _mods()
    monkeypatch.setenv("TA_HAM_SLICE", "1024")
    if forced:
        monkeypatch.setenv("TA_FORCE_HAM_SLICED", "1")
    a, b = _pair(Dg.rng(0x7600 + n), n, 0.25)
    if n:
        b[-1] = a[-1] ^ 0x0C
        b[0] = a[0] ^ 0xFF
    w = _want([a.tobytes()], [b.tobytes()])
    va, vb = _view(torch, a, 1, 0x5A), _view(torch, b, 13, 0xA5)
    out = A.guarded(1, torch.int32)
    r = B.hamming_dev(va, vb, out=out.view)
    name = T.last_kernel_name()
    out.check()
    assert r is out.view and out.numpy().view(np.uint32).tolist() == w.tolist() and name == (NEW if forced or n >= 65536 else OLD), (n, name)
    fresh = B.hamming_dev(vb, va)
    assert fresh.shape == (1,) and _u32(fresh).tolist() == w.tolist()
    with pytest.raises(T.PanicError):
        B.hamming_dev(va, vb[:-1] if n else _view(torch, np.zeros(1, np.uint8), 0, 0))
    with pytest.raises(ValueError):
        B.hamming_dev(va.cpu(), vb)


def test_hamming_dev_in_a_captured_graph_replayed_on_changed_bytes(monkeypatch):
    """one call outside the capture sizes the scratch; the captured call is one linear chain on a side stream; two replays, the inputs
    changed in between: each gives ITS input's count (partial counts that were never reset would add up)"""
    torch, T, B = _mods()
    monkeypatch.setenv("TA_HAM_SLICE", "1024")
    n = 64 * 1024 + 5
    g = Dg.rng(0x7700)
    versions = [_pair(g, n, rate) for rate in (0.5, 0.01, 0.2)]
    want = [int(_want([a.tobytes()], [b.tobytes()])[0]) for a, b in versions]
    assert len(set(want)) == 3
    va, vb = _view(torch, versions[0][0], 3, 0x11), _view(torch, versions[0][1], 9, 0xEE)
    out = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        B.hamming_dev(va, vb, out=out)
        s.synchronize()
        assert _u32(out).tolist() == [want[0]] and T.last_kernel_name() == NEW
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            B.hamming_dev(va, vb, out=out)
        assert T.last_kernel_name() == NEW
        for v in (1, 2):
            va.copy_(torch.from_numpy(versions[v][0])); vb.copy_(torch.from_numpy(versions[v][1]))
            out.fill_(-7)
            graph.replay()
            s.synchronize()
            assert _u32(out).tolist() == [want[v]], (v, _u32(out), want)


def test_host_entry_in_chunks(monkeypatch):
    """T.hamming on 3 MiB + 5 bytes, staged 1 MiB at a time: a mismatch in the very last byte and one in the first byte of the second
    chunk are each counted once"""
    torch, T, B = _mods()
    monkeypatch.setenv("TA_HAM_HOST_CHUNK", "1048576")
    n = 3 * (1 << 20) + 5
    a, b = _pair(Dg.rng(0x7800), n, 0.05)
    base = a.tobytes()
    w = int((a != b).sum())
    assert O.hamming_naive(base, b.tobytes()) == w
    assert T.hamming(base, b.tobytes()) == w and T.last_kernel_name() == NEW
    assert T.hamming(base, base) == 0
    for where in (n - 1, 1 << 20, (1 << 20) - 1, 0):
        c = a.copy()
        c[where] ^= 0x0C
        assert T.hamming(base, c.tobytes()) == 1, where
    c = a.copy()
    c[n - 1] ^= 1
    c[1 << 20] ^= 1
    assert T.hamming(c.tobytes(), base) == 2 and T.last_kernel_name() == NEW
    monkeypatch.setenv("TA_HAM_HOST_CHUNK", str(1 << 22))                          # the same pair staged whole
    assert T.hamming(base, b.tobytes()) == w and T.last_kernel_name() == NEW
    with pytest.raises(T.PanicError):
        T.hamming(b"ab", b"abc")
    with pytest.raises(T.PanicError):
        T.hamming(base, base[:-1])


def test_one_device_set_row():
    """a host batch of 4 x 200,000 bytes through the device set (two workers on device 0): the workers' ta_hamming_batch takes the
    sliced route by the rule (the kernel name is the workers' thread-local, so the answers are what is checked here)"""
    from triple_accel_amd import multi as M
    g = Dg.rng(0x7900)
    a = g.integers(0, 256, (4, 200000), dtype=np.uint8)
    b = a.copy()
    hit = g.random(a.shape) < np.array([[0.0], [0.01], [0.5], [1.0]])
    b[hit] ^= 0x0C
    w = (a != b).sum(axis=1).astype(np.uint32)
    assert np.array_equal(w, O.hamming_batch(O.csr_from_fixed(a), O.csr_from_fixed(b))) and w[0] == 0 and w[3] == 200000
    M.set_devices([0, 0])
    try:
        assert np.array_equal(M.hamming_batch_host(a, b), w)
    finally:
        M.set_devices(None)
