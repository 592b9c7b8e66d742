"""Re-hosts one side of a batch in a hostile arena (tests/test_gpu_layouts.py; verified byte for byte by tests/test_layout_arena_cpu.py).

include/triple_accel_amd.h promises more about memory layout than Strings.from_list / Strings.from_fixed ever produce: the strided form
has `stride` and `len` as separate fields, CSR offsets need not start at 0, a blob pointer may have any byte alignment and the bytes
around the strings (the 16 bytes of read slack included) may hold anything.  host_side() lays the strings of one side out under a Layout
in plain numpy -- so the result can be checked without a GPU -- and to_strings() uploads it and points a batch.Strings into it.

Every arena keeps MARGIN bytes of fill in front of its first byte and behind its last one (read slack included): a kernel that reads
further than the contract allows still stays inside memory the test owns.  These layouts expose wrong ANSWERS; they never invite a fault.

guarded() is the same idea for outputs: a view inside a larger tensor, guard bands on both sides, a pre-fill that shows unwritten slots."""
from dataclasses import dataclass

import numpy as np

SLACK = 16                    # TA_BLOB_SLACK
MARGIN = 256                  # fill in front of the blob pointer's allocation base and behind the slack
GUARD = 64                    # guard elements on each side of a guarded output
GUARD_BYTE = 0x5A             # every guard byte: 0x5A5A5A5A as int32
PREFILL_BYTE = 0xA7           # every byte of a guarded view before the call: 0xA7A7A7A7 (negative) as int32
PREFILL32 = np.frombuffer(bytes([PREFILL_BYTE] * 4), dtype=np.int32)[0]

FORMS = ("csr", "csr_view", "strided", "overlap", "shared")
SHIFTS = (0, 1, 3, 15, 16, 17, 63, 65, 127)
PADS = (0, 1, 3, 16, 61)
OVERLAP_STRIDES = (1, 7)
LEADS = (0, 5)
PLAIN_FILLS = {"00": 0x00, "ff": 0xFF, "0c": 0x0C}
FILLS = ("00", "ff", "0c", "echo", "continue", "nul")
BASE_OF_FILL = {"00": 0x00, "ff": 0xFF, "0c": 0x0C, "echo": 0xFF, "continue": 0xFF, "nul": 0xFF}
DECOYS = (3, 2)               # csr_view: decoy rows in front of and behind the batch's rows


@dataclass(frozen=True)
class Layout:
    """form: csr | csr_view | strided | overlap | shared (stride 0: one string for every pair).  shift: the blob pointer lies `shift` bytes
    behind a 256-byte aligned address.  pad: strided, stride = len + pad.  stride: overlap, the distance of two windows (< len).
    lead: csr, off[0].  fill: what the bytes that belong to no string hold (module docstring of tests/test_gpu_layouts.py)."""
    form: str = "csr"
    shift: int = 0
    pad: int = 0
    stride: int = 1
    lead: int = 0
    fill: str = "ff"

    def tag(self):
        extra = {"csr": "lead%d" % self.lead, "csr_view": "view", "strided": "pad%d" % self.pad, "overlap": "step%d" % self.stride,
                 "shared": "shared"}[self.form]
        return "%s-%s-shift%d-%s" % (self.form, extra, self.shift, self.fill)


class HostSide:
    """One side of a batch laid out in host memory.  buf: the whole allocation (uint8).  base: index in buf of the blob pointer.
    off: the int64 offsets tensor as uploaded (csr_view: the LARGER batch's) or None.  row0: index in off of the batch's first offset.
    n, stride, length: the C view's fields.  oracle: the strings the oracle must see.  Three masks over buf: owned = the byte
    belongs to a string of the batch; decoy = to a string of the larger batch (csr_view); special = written by the fills echo / continue
    / nul.  Every other byte holds BASE_OF_FILL[layout.fill]."""

    def __init__(self, layout, buf, base, off, row0, n, stride, length, oracle, owned, decoy, special):
        self.layout, self.buf, self.base, self.off, self.row0 = layout, buf, base, off, row0
        self.n, self.stride, self.length, self.oracle = n, stride, length, oracle
        self.owned, self.decoy, self.special = owned, decoy, special

    def spans(self):
        """(start, end) of every string of the batch as indices into buf, read the way the C ABI reads them"""
        if self.off is not None:
            o = self.off[self.row0:self.row0 + self.n + 1]
            return [(self.base + int(o[i]), self.base + int(o[i + 1])) for i in range(self.n)]
        return [(self.base + i * self.stride, self.base + i * self.stride + self.length) for i in range(self.n)]

    def extract(self):
        return [self.buf[s:e].tobytes() for s, e in self.spans()]

    def last_end(self):
        return max((e for _, e in self.spans()), default=self.base)

    def max_len(self):
        return max((e - s for s, e in self.spans()), default=0)


def _as_list(strings):
    if isinstance(strings, np.ndarray):
        assert strings.dtype == np.uint8 and strings.ndim == 2
        return [r.tobytes() for r in strings]
    return [bytes(s) for s in strings]


def _cyclic(src, start, count):
    """count bytes of src from position start on, wrapping round (src not empty)"""
    idx = (start + np.arange(count)) % len(src)
    return np.frombuffer(src, dtype=np.uint8)[idx]


def continuation(haystack, needle):
    """the bytes that, written behind `haystack`, complete an exact occurrence of `needle` that begins inside it (or right at its end):
    needle[j:] for the longest proper prefix needle[:j] the haystack ends with"""
    for j in range(min(len(needle) - 1, len(haystack)), -1, -1):
        if j == 0 or haystack.endswith(needle[:j]):
            return needle[j:]
    return needle


def _gap_bytes(layout, row, count, partner_row, needle, last):
    """what the `count` bytes right behind `row` hold under the special fills; None = the base fill.  last: nothing of the batch follows
    (the read slack and the margin)."""
    f = layout.fill
    if count <= 0:
        return None
    if f == "echo":
        if last and partner_row:
            return _cyclic(partner_row, len(row), count)          # the partner's bytes at the positions behind this string
        return _cyclic(row, 0, count) if row else None            # the row's own first bytes
    out = np.full(count, BASE_OF_FILL[f], dtype=np.uint8)
    if f == "continue" and needle:
        c = continuation(row, needle)[:count]
        out[:len(c)] = np.frombuffer(c, dtype=np.uint8)
        return out
    if f == "nul":
        out[0] = 0
        return out
    return None


def host_side(strings, layout, n=None, partner=None, needles=None, seed=0):
    """strings (list of bytes or an (n, len) uint8 array) under `layout` -> HostSide.  partner: the other side's strings (fill echo).
    needles: the needle of every row (fill continue; one bytes object = a shared needle).  n: the pair count of the shared form."""
    rows = _as_list(strings)
    L = layout
    base_fill = BASE_OF_FILL[L.fill]
    partner = _as_list(partner) if partner is not None else None
    if isinstance(needles, (bytes, bytearray)):
        needles = [bytes(needles)] * len(rows)
    g = np.random.Generator(np.random.PCG64(0xA7E4A + seed))
    off, row0 = None, 0
    # ---- the blob relative to the blob pointer: pieces = (position, bytes) of every string; extent = the last byte of any string + 1
    if L.form in ("csr", "csr_view"):
        before, after = ([], [])
        if L.form == "csr_view":
            lens = [len(r) for r in rows] or [8]
            mk = lambda: g.integers(1, 256, size=int(g.integers(1, max(lens) + 2)), dtype=np.uint8).tobytes()
            before, after = [mk() for _ in range(DECOYS[0])], [mk() for _ in range(DECOYS[1])]
        lead = L.lead if L.form == "csr" else 0
        allrows = before + rows + after
        off = np.zeros(len(allrows) + 1, dtype=np.int64)
        off[0] = lead
        np.cumsum([len(r) for r in allrows], out=off[1:])
        off[1:] += lead
        row0 = len(before)
        pos = [int(off[row0 + i]) for i in range(len(rows))]
        n_rows, stride, length = len(rows), 0, 0
        decoys = [(int(off[i]), allrows[i]) for i in range(len(allrows)) if i < row0 or i >= row0 + len(rows)]
        extent = int(off[-1])
    elif L.form == "strided":
        length = len(rows[0]) if rows else 0
        assert all(len(r) == length for r in rows), "the strided form needs strings of one length"
        stride, n_rows, decoys = length + L.pad, len(rows), []
        pos = [i * stride for i in range(n_rows)]
        extent = (n_rows - 1) * stride + length if n_rows else 0
    elif L.form == "overlap":
        length = len(rows[0]) if rows else 0
        assert all(len(r) == length for r in rows) and 0 < L.stride < max(length, 2)
        stride, n_rows, decoys = L.stride, len(rows), []
        seq = b"".join(r[:stride] for r in rows[:-1]) + (rows[-1] if rows else b"")     # rows become sliding windows over this sequence
        rows = [seq[i * stride:i * stride + length] for i in range(n_rows)]
        pos = [i * stride for i in range(n_rows)]
        extent = len(seq)
    elif L.form == "shared":
        assert len(rows) == 1 and n is not None
        length, stride, n_rows, decoys = len(rows[0]), 0, n, []
        rows = rows * n
        pos = [0] * n
        extent = length
    else:
        raise ValueError(L.form)
    base = MARGIN + L.shift
    total = base + extent + SLACK + MARGIN
    total += (-total) % 8
    buf = np.full(total, base_fill, dtype=np.uint8)
    owned, decoy, special = (np.zeros(total, dtype=bool) for _ in range(3))
    for p, d in decoys:                                            # other people's strings: neither owned nor fill
        buf[base + p:base + p + len(d)] = np.frombuffer(d, dtype=np.uint8)
        decoy[base + p:base + p + len(d)] = True
    order = list(range(n_rows)) if L.form != "shared" else [0]
    if L.form == "strided" and L.fill != "continue" and n_rows > 1 and length:
        # the rows (and the gaps behind all but the last one) as 2-D views of the buffer: the big batches in one step
        from numpy.lib.stride_tricks import as_strided
        arr = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(n_rows, length)
        vb, vo, vs = (as_strided(x[base:], (n_rows, stride), (stride, 1)) for x in (buf, owned, special))
        if L.pad and L.fill == "echo":
            vb[:-1, length:] = arr[:-1, np.arange(L.pad) % length]
            vs[:-1, length:] = True
        if L.pad and L.fill == "nul":
            vb[:-1, length] = 0
            vs[:-1, length:] = True
        vb[:, :length] = arr
        vo[:, :length] = True
        order = [n_rows - 1]                                       # what is left: the bytes behind the last string
    # the special fills first (a later string may overwrite the front of a gap: strings win), then the strings
    if L.fill in ("echo", "continue", "nul") and rows:
        batch_end = max(pos[i] + len(rows[i]) for i in order)
        for i in order:
            end = pos[i] + len(rows[i])
            last = end == batch_end
            if L.form in ("csr", "csr_view", "overlap") and not last:
                continue                                           # no gap behind this row: the next string starts there
            # behind the last string: the read slack and half the margin (csr_view: over the decoy rows that follow)
            count = (SLACK + MARGIN // 2) if last else (pos[i + 1] - end if i + 1 < n_rows else 0)
            gb = _gap_bytes(L, rows[i], count, partner[min(i, len(partner) - 1)] if partner else None,
                            needles[min(i, len(needles) - 1)] if needles else None, last)
            if gb is not None:
                buf[base + end:base + end + count] = gb
                special[base + end:base + end + count] = True
    for i in order:
        r = np.frombuffer(rows[i], dtype=np.uint8)
        buf[base + pos[i]:base + pos[i] + len(r)] = r
        owned[base + pos[i]:base + pos[i] + len(r)] = True
    special &= ~owned
    decoy &= ~special
    return HostSide(L, buf, base, off, row0, n_rows, stride, length, list(rows), owned, decoy, special)


def to_strings(side, device="cuda"):
    """upload a HostSide: -> batch.Strings whose blob / off pointers lie INSIDE the uploaded tensors (the tensors stay referenced)"""
    import torch
    from triple_accel_amd import batch as B
    t = torch.from_numpy(side.buf).to(device)
    assert t.data_ptr() % 256 == 0
    blob = t[side.base:]
    if side.off is not None:
        ot = torch.from_numpy(side.off).to(device)
        s = B.Strings(blob, ot[side.row0:side.row0 + side.n + 1], max_len=side.max_len())
        s._arena = (t, ot)
        return s
    s = B.Strings(blob, None, stride=side.stride, length=side.length, n=side.n)
    s._arena = (t,)
    return s


# ---------------------------------------------------------------- token sequences (CSR only: the binding has no element stride)
def host_tokens(seqs, shift_items=3, lead=5, sentinel=0x5A5A5A5A, margin=64):
    """-> (values int64 array of the whole allocation, base item index, off int64 array with off[0] = lead): the items of sequence i are
    values[base + off[i] .. base + off[i+1]); every other item holds `sentinel`."""
    lens = [len(s) for s in seqs]
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[0] = lead
    np.cumsum(lens, out=off[1:])
    off[1:] += lead
    base = margin + shift_items
    vals = np.full(base + int(off[-1]) + margin, sentinel, dtype=np.int64)
    for i, s in enumerate(seqs):
        vals[base + int(off[i]):base + int(off[i + 1])] = np.asarray(s, dtype=np.int64)
    return vals, base, off


def to_tokens(vals, base, off, device="cuda"):
    import torch
    from triple_accel_amd import batch as B
    v32 = vals.astype(np.uint32).view(np.int32)
    t = torch.from_numpy(v32).to(device)
    tok = B.Tokens(t[base:], torch.from_numpy(off).to(device), max_len=int(np.diff(off).max()) if len(off) > 1 else 0)
    tok._arena = t
    return tok


# ---------------------------------------------------------------- guarded outputs
class Guarded:
    """.view: a contiguous tensor of `shape` inside a larger one; GUARD elements of 0x5A bytes on each side; the view pre-filled with 0xA7
    bytes.  check() asserts both guard bands untouched (after a stream synchronisation)."""

    def __init__(self, shape, dtype, device="cuda"):
        import torch
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.count = int(np.prod(shape)) if shape else 1
        self.itemsize = torch.empty(0, dtype=dtype).element_size()
        self.full = torch.empty(self.count + 2 * GUARD, dtype=dtype, device=device)
        self._bytes = self.full.view(torch.uint8)
        self._bytes.fill_(GUARD_BYTE)
        self.view = self.full[GUARD:GUARD + self.count].view(shape)
        if self.count:
            self.view.view(torch.uint8).fill_(PREFILL_BYTE)

    def check(self):
        import torch
        torch.cuda.synchronize()
        g = GUARD * self.itemsize
        raw = self._bytes.cpu().numpy()
        lo, hi = raw[:g], raw[g + self.count * self.itemsize:]
        assert (lo == GUARD_BYTE).all(), "guard in front of the output touched at byte %d" % int(np.flatnonzero(lo != GUARD_BYTE)[-1] - g)
        assert (hi == GUARD_BYTE).all(), "guard behind the output touched at byte +%d" % int(np.flatnonzero(hi != GUARD_BYTE)[0])
        return self

    def numpy(self):
        return self.view.cpu().numpy()

    def unwritten(self):
        """bool array of the view's shape: the element still holds the pre-fill in every byte"""
        raw = self.view.cpu().numpy()
        b = raw.view(np.uint8).reshape(raw.shape + (self.itemsize,))
        return (b == PREFILL_BYTE).all(axis=-1)


def guarded(shape, dtype, device="cuda"):
    return Guarded(shape, dtype, device)
