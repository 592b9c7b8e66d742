"""not-gpu: the Hamming cross body (ham_cross_body.h) under host emulation -- a wavefront of 64 emulated lanes loads up to 64 targets,
stages ONE chunk of queries through its slice of LDS and compares every query with every target, at every register width NW that admits
the lengths; every (query, lane) answer is compared with a numpy double loop (equal length, count the differing bytes), itself checked
against the oracle's hamming_naive.  Plus the argument errors of ta_hamming_cross and its refusal to run without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import datagen as Dg
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
EMU_DIR = os.path.join(HERE, "emu_hcross")
NONE = 0xFFFFFFFF
QUERY_LENS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64)
TARGET_LENS = QUERY_LENS + (65, 100)
ALPHABETS = {
    "acgt": np.frombuffer(b"ACGT", np.uint8),
    "lower": np.arange(97, 123, dtype=np.uint8),
    "0..255": np.arange(0, 256, dtype=np.uint8),
    "nul": np.array([0x00], np.uint8),                            # the targets' and queries' pad byte ...
    "nul+0c": np.array([0x00, 0x0C], np.uint8),                   # ... and the constant the staged queries carry
    "0c+0d": np.array([0x0C, 0x0D], np.uint8),
}
NWS = (4, 8, 16)

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(EMU_DIR, "libta_emu_hcross.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", EMU_DIR, "-s"])
        _lib = C.CDLL(path)
        _lib.emu_hcross_chunk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int,
                                          C.c_void_p, C.c_void_p]
        _lib.emu_hcross_chunk.restype = C.c_int
    return _lib


def k8_of(k):
    """what the host entry hands the kernel: eight per mismatch, k clamped to the longest string"""
    return 8 * min(k, 64) + 7


def side(strings, align, fill):
    """CSR blob whose first string starts `align` bytes past a 16-byte boundary (the others follow without gaps, so their alignments
    are whatever the lengths make them), `fill` in front and in the 16 bytes of read slack behind -> (keepalive, address, offsets)"""
    data = b"".join(strings)
    raw = np.full(len(data) + 64, fill, np.uint8)
    base = (-raw.ctypes.data) % 16 + align
    raw[base:base + len(data)] = np.frombuffer(data, np.uint8)
    off = np.zeros(len(strings) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in strings])
    return raw, raw.ctypes.data + base, off


def emu(queries, targets, k, nw, qalign=0, talign=0):
    """-> (res[len(queries)][len(targets)]: mismatches of a hit or NONE, ran[len(queries)])"""
    assert len(targets) <= 64 and len(queries) <= 256 // nw
    qraw, qaddr, qoff = side(queries, qalign, 0x5A)
    traw, taddr, toff = side(targets, talign, 0xA5)
    res, ran = np.full(64 * max(len(queries), 1), 7, np.uint32), np.zeros(max(len(queries), 1), np.uint32)
    rc = lib().emu_hcross_chunk(qaddr, qoff.ctypes.data, len(queries), taddr, toff.ctypes.data, len(targets), k8_of(k), nw,
                                res.ctypes.data, ran.ctypes.data)
    assert rc == 0, (nw, [len(q) for q in queries])
    res = res.reshape(-1, 64)[:len(queries)]
    assert (res[:, len(targets):] == NONE).all()                   # lanes without a target never hit
    return res[:, :len(targets)], ran[:len(queries)].astype(bool)


def join(queries, targets, k):
    """the numpy double loop: equal length, count the differing bytes"""
    out = np.full((len(queries), len(targets)), NONE, np.uint32)
    for i, q in enumerate(queries):
        a = np.frombuffer(q, np.uint8)
        for j, t in enumerate(targets):
            if len(t) == len(q):
                d = int((a != np.frombuffer(t, np.uint8)).sum())
                if d <= k:
                    out[i, j] = d
    return out


def check(queries, targets, ks, qalign=0, talign=0):
    longest = max([len(q) for q in queries] or [0])
    n = 0
    for nw in NWS:
        if longest > 4 * nw:
            continue
        for c0 in range(0, len(queries), 256 // nw):               # one staged chunk per call
            chunk = queries[c0:c0 + 256 // nw]
            for k in ks:
                got, ran = emu(chunk, targets, k, nw, qalign, talign)
                want = join(chunk, targets, k)
                assert np.array_equal(got, want), (nw, k, qalign, talign, np.argwhere(got != want)[:4].tolist())
                # a query whose length no target of at most 4 nw bytes shares costs no compare
                shared = [any(len(t) == len(q) and len(t) <= 4 * nw for t in targets) for q in chunk]
                assert ran.tolist() == shared, (nw, k)
                n += 1
    assert n
    return n


def rand(g, alphabet, n):
    return bytes(g.choice(alphabet, n)) if n else b""


def substitute(g, s, where, alphabet):
    """s with the bytes at `where` changed (to another symbol of the alphabet when it has one, else to any other byte)"""
    s = bytearray(s)
    for p in where:
        others = [int(c) for c in alphabet if int(c) != s[p]] or [s[p] ^ 0x0C, s[p] ^ 0xFF]
        s[p] = others[int(g.integers(len(others)))]
    return bytes(s)


def ks_of(m):
    return sorted({0, 1, 2, max(m - 1, 0), m, 64, 0xFFFFFFFF})


def test_the_double_loop_is_the_oracles_hamming_naive():
    g = Dg.rng(8001)
    for name, alphabet in ALPHABETS.items():
        for m in QUERY_LENS:
            a, b, c = rand(g, alphabet, m), rand(g, alphabet, m), rand(g, alphabet, m + 1)
            want = O.hamming_naive(a, b)
            assert want is not None and int(join([a], [b], 64)[0, 0]) == want, (name, m)
            assert O.hamming_naive(a, c) is None and int(join([a], [c], 64)[0, 0]) == NONE      # the panic: never a hit


@pytest.mark.parametrize("name", list(ALPHABETS))
def test_every_query_length_against_mixed_targets(name):
    """all thirteen query lengths in one chunk (NW = 16), and the ones that fit at NW = 8 and NW = 4; targets of every length of the
    set plus 65 and 100 (dead lanes: never loaded, never a hit), random ones and copies of queries with a few substitutions"""
    g = Dg.rng(8100 + len(name))
    alphabet = ALPHABETS[name]
    for qmax in (16, 32, 64):
        queries = [rand(g, alphabet, m) for m in QUERY_LENS if m <= qmax]
        targets = [rand(g, alphabet, n) for n in TARGET_LENS]
        for q in queries:
            for e in (0, 1, 2, 3):
                if e <= len(q):
                    targets.append(substitute(g, q, g.choice(len(q), e, replace=False) if e else [], alphabet))
        targets = targets[:64]
        g.shuffle(targets)
        check(queries, targets, (0, 1, 2, 5, 64, 0xFFFFFFFF))


@pytest.mark.parametrize("name", list(ALPHABETS))
def test_planted_at_exactly_k_and_k_plus_one(name):
    """for every query length m and every k of the issue's list: targets at exactly k and k + 1 mismatches of the query, the mismatches
    spread at random, packed at the end (the last byte included), or starting at the first byte behind a 16-byte piece boundary"""
    g = Dg.rng(8200 + len(name))
    alphabet = ALPHABETS[name]
    n = 0
    for m in QUERY_LENS:
        query = rand(g, alphabet, m)
        for k in ks_of(m):
            targets = [query, rand(g, alphabet, m), rand(g, alphabet, m + 1), rand(g, alphabet, max(m - 1, 0)), b"x" * 65, b"y" * 100]
            for e in (k, k + 1):
                if e > m:
                    continue
                spread = sorted(int(p) for p in g.choice(m, e, replace=False)) if e else []
                tail = list(range(m - e, m))
                places = [spread, tail]
                for edge in (16, 32, 48):
                    if edge + e <= m and e:
                        places.append(list(range(edge, edge + e)))
                for where in places:
                    t = substitute(g, query, where, alphabet)
                    assert int(join([query], [t], 64)[0, 0]) == e
                    targets.append(t)
            n += check([query], targets[:64], [k])
            assert len(targets) <= 64
            want = join([query], targets, k)[0].tolist()
            assert want[0] == 0 and (k > m or k in want[6:]) and (k + 1 > m or NONE in want[6:])   # exactly k hits, k + 1 does not
    assert n > 100


def test_last_byte_and_first_byte_behind_a_piece_boundary():
    g = Dg.rng(8300)
    alphabet = ALPHABETS["acgt"]
    for m in (1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64):
        query = rand(g, alphabet, m)
        targets = [query, substitute(g, query, [m - 1], alphabet), substitute(g, query, [0], alphabet)]
        for edge in (16, 32, 48):
            if edge < m:
                targets.append(substitute(g, query, [edge], alphabet))
            if edge - 1 < m:
                targets.append(substitute(g, query, [edge - 1], alphabet))
        for nw in NWS:
            if m > 4 * nw:
                continue
            got, _ = emu([query], targets, 1, nw)
            assert got[0].tolist() == [0] + [1] * (len(targets) - 1), (m, nw)
            got, _ = emu([query], targets, 0, nw)
            assert got[0].tolist() == [0] + [NONE] * (len(targets) - 1), (m, nw)


@pytest.mark.parametrize("align", range(16))
def test_every_byte_alignment_of_both_blobs(align):
    g = Dg.rng(8400 + align)
    alphabet = ALPHABETS["0..255"]
    queries = [rand(g, alphabet, m) for m in QUERY_LENS]
    targets = [substitute(g, q, g.choice(len(q), min(2, len(q)), replace=False) if len(q) else [], alphabet) for q in queries] * 4
    check(queries, targets, (1, 2), qalign=align, talign=(5 * align + 3) % 16)
    check(queries, targets, (2,), qalign=(align + 7) % 16, talign=align)


@pytest.mark.parametrize("name", ["acgt", "nul", "nul+0c", "0c+0d"])
def test_the_pad_hides_the_byte_after_the_end(name):
    """equal strings followed by DIFFERENT bytes in their blobs (another string's first byte, the slack's fill) are at distance 0, at
    every length: only the cleared pads can make that so -- and a string that continues with the other one's pad value (0x00 on the
    target side, 0x0C after the XOR on the query side) is longer, hence no hit"""
    g = Dg.rng(8500 + len(name))
    alphabet = ALPHABETS[name]
    followers = [bytes([b]) for b in (0x00, 0x0C, 0x0D, 0xFF, 0x41, 0xF3)]
    for m in QUERY_LENS:
        s = rand(g, alphabet, m)
        targets = []
        for f in followers:                                        # s, then a one-byte string that differs each time
            targets += [s, f]
        targets += [s + b"\x00", s + b"\x0c", s]                    # (the last copy is followed by the slack's fill)
        queries = [s, b"\x0c", s, b"\x00", s + b"\x00", s + b"\x0c"] if m < 64 else [s, b"\x0c", s, b"\x00"]
        for k in (0, 1):
            check(queries, targets, [k])
        want = join([s], targets, 0)[0].tolist()
        assert want.count(0) >= len(followers) + 1


def test_fewer_than_64_targets_and_an_empty_chunk():
    g = Dg.rng(8600)
    alphabet = ALPHABETS["acgt"]
    for nt in (0, 1, 2, 33, 63, 64):
        queries = [rand(g, alphabet, m) for m in (0, 5, 16)]
        targets = [rand(g, alphabet, (0, 5, 16)[i % 3]) for i in range(nt)]
        check(queries, targets, (0, 4, 16))
    got, ran = emu([], [b"ACGT"], 1, 4)
    assert got.shape == (0, 1) and ran.shape == (0,)


def test_a_full_chunk_at_every_width():
    g = Dg.rng(8700)
    alphabet = ALPHABETS["acgt"]
    for nw in NWS:
        m = 4 * nw
        base = [rand(g, alphabet, m) for _ in range(8)]
        queries = [substitute(g, base[i % 8], g.choice(m, i % 3, replace=False) if i % 3 else [], alphabet) for i in range(256 // nw)]
        targets = [substitute(g, base[i % 8], g.choice(m, i % 4, replace=False) if i % 4 else [], alphabet) for i in range(64)]
        for k in (2, 5):                                           # (at most 2 + 3 substitutions apart: at k = 5 every pair of one base hits)
            got, ran = emu(queries, targets, k, nw)
            want = join(queries, targets, k)
            assert np.array_equal(got, want) and ran.all() and (want != NONE).sum() >= (64 if k == 2 else 128)


# ---------------------------------------------------------------- the C ABI: argument errors come first, no CPU fallback
def _abi():
    from triple_accel_amd import _native as N
    return N


def _call(queries, nq, targets, nt, k=1, flags=0, hits=None, count=None, cap=0, nearest=None, per_query=None):
    return _abi().lib().ta_hamming_cross(queries, nq, targets, nt, k, flags, hits, count, cap, nearest, per_query, None)


def test_abi_symbol_is_declared_and_exported():
    N = _abi()
    assert "ta_hamming_cross" in N.ABI_SYMBOLS and hasattr(N.lib(), "ta_hamming_cross") and N.TA_CROSS_UPPER == 1
    header = open(os.path.join(os.path.dirname(HERE), "include", "triple_accel_amd.h")).read()
    assert "#define TA_CROSS_UPPER 1u" in header and "src/hamming.rs:390" in header


def test_abi_argument_errors_come_before_the_device():
    N = _abi()
    blob = (C.c_uint8 * 64)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 0, 8, 0)
    fake = C.c_void_p(0x1000)
    S = C.byref(s)
    assert _call(None, 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, None, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=None) == N.TA_ERR_ARG                               # count_dev is required ...
    assert _call(S, 0, S, 0, count=None) == N.TA_ERR_ARG                               # ... whatever the sizes
    for flags in (2, 3, 4, 0x80000000, 0xFFFFFFFF):                                    # any bit but TA_CROSS_UPPER
        assert _call(S, 1, S, 1, flags=flags, count=fake) == N.TA_ERR_ARG, flags
    noblob = N.StringsC(0, 0, 0, 8, 0)
    assert _call(C.byref(noblob), 1, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, C.byref(noblob), 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=fake, cap=4, hits=None) == N.TA_ERR_ARG
    assert _call(S, 1 << 32, S, 1, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1 << 32, count=fake) == N.TA_ERR_ARG
    assert _call(S, 1, S, 1, count=fake, cap=1 << 60, hits=fake) == N.TA_ERR_ARG       # cap * sizeof(ta_cross_hit) overflows
    # an argument error wins over an unsupported length
    long_query = N.StringsC(ptr, 0, 65, 65, 0)
    assert _call(C.byref(long_query), 1, S, 1, flags=2, count=fake) == N.TA_ERR_ARG


def test_abi_unsupported_lengths_come_before_the_device():
    N = _abi()
    blob = (C.c_uint8 * 128)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 0, 8, 0)
    S = C.byref(s)
    fake = C.c_void_p(0x1000)
    for flags in (0, N.TA_CROSS_UPPER):
        long_query = N.StringsC(ptr, 0, 65, 65, 0)
        assert _call(C.byref(long_query), 1, S, 1, flags=flags, count=fake) == N.TA_ERR_UNSUPPORTED
        long_csr_query = N.StringsC(ptr, 0x1000, 0, 0, 65)
        assert _call(C.byref(long_csr_query), 1, S, 1, flags=flags, count=fake) == N.TA_ERR_UNSUPPORTED
        huge_target = N.StringsC(ptr, 0, 1 << 32, 1 << 32, 0)
        assert _call(S, 1, C.byref(huge_target), 1, flags=flags, count=fake) == N.TA_ERR_UNSUPPORTED
        huge_csr_target = N.StringsC(ptr, 0x1000, 0, 0, 1 << 32)
        assert _call(S, 1, C.byref(huge_csr_target), 1, flags=flags, count=fake) == N.TA_ERR_UNSUPPORTED


def test_no_cpu_fallback():
    import torch
    N = _abi()
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    blob = (C.c_uint8 * 128)()
    ptr = C.cast(blob, C.c_void_p).value
    s = N.StringsC(ptr, 0, 0, 8, 0)
    long_target = N.StringsC(ptr, 0, 100, 100, 0)                                      # targets over 64 bytes are allowed: never hits
    count = (C.c_uint64 * 1)()
    cnt = C.cast(count, C.c_void_p)
    for flags in (0, N.TA_CROSS_UPPER):
        for k in (0, 1, 64, 0xFFFFFFFF):
            assert _call(C.byref(s), 1, C.byref(s), 1, k=k, flags=flags, count=cnt) == N.TA_ERR_HIP
    assert _call(C.byref(s), 1, C.byref(long_target), 1, count=cnt) == N.TA_ERR_HIP
    assert _call(C.byref(s), 0, C.byref(s), 4, count=cnt) == N.TA_ERR_HIP              # the count is zeroed on the device
