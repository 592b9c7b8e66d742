"""Batch entry points on device-resident data (torch tensors carry the HBM buffers; the
arithmetic is the HIP kernels behind the C ABI).  New surface with no reference analogue:
N = 1 equals the single-call functions."""
import ctypes as _C

import torch

from . import _native as _n
from . import EditCosts, LEVENSHTEIN_COSTS, SearchType, _costs, _raise

SLACK = 16


class Strings:
    """A batch side: CSR (blob + n+1 int64 offsets) or strided (fixed length) uint8 data in HBM."""

    def __init__(self, blob, off=None, stride=0, length=0, max_len=0, n=None):
        assert blob.dtype == torch.uint8 and blob.is_cuda and blob.is_contiguous()
        self.blob, self.off, self.stride, self.length, self.max_len = blob, off, stride, length, max_len
        if off is not None:
            assert off.dtype == torch.int64 and off.is_cuda and off.is_contiguous()
            self.n = off.numel() - 1
        else:
            self.n = n if n is not None else (blob.numel() - SLACK) // max(stride, 1)

    def __setattr__(self, name, value):
        # the C view is built once per batch side (_c); changing a field drops it
        if name in ("blob", "off", "stride", "length", "max_len"):
            self.__dict__.pop("_cview", None)
            self.__dict__.pop("_cref", None)
        object.__setattr__(self, name, value)

    @classmethod
    def from_list(cls, strings, device="cuda"):
        import numpy as np
        lens = np.fromiter((len(s) for s in strings), dtype=np.int64, count=len(strings))
        off = np.zeros(len(strings) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        blob = np.zeros(int(off[-1]) + SLACK, dtype=np.uint8)
        if off[-1]:
            blob[:int(off[-1])] = np.frombuffer(b"".join(bytes(s) for s in strings), dtype=np.uint8)
        return cls(torch.from_numpy(blob).to(device), torch.from_numpy(off).to(device),
                   max_len=int(lens.max()) if len(strings) else 0)

    @classmethod
    def from_fixed(cls, array_2d, device="cuda"):
        """(n, len) uint8 array/tensor -> strided batch (stride == len) with read slack."""
        t = torch.as_tensor(array_2d, dtype=torch.uint8)
        n, length = t.shape
        blob = torch.zeros(n * length + SLACK, dtype=torch.uint8, device=device)
        blob[: n * length] = t.reshape(-1).to(device)
        return cls(blob, None, stride=length, length=length, n=n)

    @classmethod
    def shared(cls, needle, n, device="cuda"):
        """ONE needle for a batch of n pairs: the strided form with stride 0 (levenshtein_search_batch's shared needle -- an adapter,
        a primer -- the only needle form its scan route takes)"""
        needle = bytes(needle)
        blob = torch.zeros(len(needle) + SLACK, dtype=torch.uint8)
        if needle:
            blob[:len(needle)] = torch.frombuffer(bytearray(needle), dtype=torch.uint8)
        return cls(blob.to(device), None, stride=0, length=len(needle), n=n)

    def longest(self):
        """an upper bound on the length of any string of the side: `length` (strided), `max_len` when the caller gave it, else
        measured from the offsets (a CSR side built as Strings(blob, off) has max_len = 0 = "let the library measure it")"""
        if self.off is None:
            return int(self.length)
        if not self.max_len and self.n > 0:
            self.max_len = int((self.off[1:] - self.off[:-1]).max().item())
        return int(self.max_len)

    def _c(self):
        """the C view (built once: the tensors of a batch side do not change)"""
        c = self.__dict__.get("_cview")
        if c is None:
            c = self._cview = _n.StringsC(self.blob.data_ptr(), 0 if self.off is None else self.off.data_ptr(),
                                          self.stride, self.length, self.max_len)
            self._cref = _C.byref(c)
        return c

    def _ref(self):
        self._c()
        return self._cref


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """the current stream's handle (the raw getter skips building a torch.cuda.Stream object per call)"""
    if _raw_stream is not None:
        return _C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return _C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(n, device):
    return torch.empty(n, dtype=torch.int32, device=device)


def levenshtein_k_batch(a: Strings, b: Strings, k, costs=LEVENSHTEIN_COSTS, out=None, alphabet=None):
    """out[i] = levenshtein_simd_k_with_opts(a_i, b_i, k, false, costs) as int32 (-1 == None).
    alphabet: the byte values the strings are written in -- up to four (b"ACGT") or up to 32 (IUPAC codes, the amino acids'
    letters): the small-alphabet kernels (same answers; pairs with other bytes are still answered, by the general kernel)."""
    assert a.n == b.n
    out = _out(a.n, a.blob.device) if out is None else out
    cc = _costs(costs)._c()
    if alphabet is not None:
        alphabet = bytes(alphabet)
        rc = _n.lib().ta_levenshtein_k_batch_alphabet(a._ref(), b._ref(), a.n, k, _C.byref(cc), alphabet, len(alphabet), out.data_ptr(), _stream())
        if rc:
            _raise(rc)
        return out
    rc = _n.lib().ta_levenshtein_k_batch(a._ref(), b._ref(), a.n, k, _C.byref(cc), out.data_ptr(), _stream())
    if rc:
        _raise(rc)
    return out


def levenshtein_exp_batch(a: Strings, b: Strings, costs=LEVENSHTEIN_COSTS, out=None):
    assert a.n == b.n
    out = _out(a.n, a.blob.device) if out is None else out
    ca, cb, cc = a._c(), b._c(), _costs(costs)._c()
    _raise(_n.lib().ta_levenshtein_exp_batch(_C.byref(ca), _C.byref(cb), a.n, _C.byref(cc), out.data_ptr(), _stream()))
    return out


_EDIT_NAMES = ("Match", "Mismatch", "AGap", "BGap", "Transpose")


def levenshtein_trace_batch(a: Strings, b: Strings, k, costs=LEVENSHTEIN_COSTS, cap=None, out=None, edits=None, n_edits=None):
    """levenshtein_simd_k_with_opts(a_i, b_i, k, trace_on=True, costs) for every pair, on the device: -> (out, edits, n_edits) with
    out[i] = distance (int32, -1 == None), n_edits[i] = runs of pair i's script, edits[i, t] = (edit type, count) of run t (int64 pairs;
    edit types as triple_accel_amd.EditType).  cap = runs kept per pair (default 2 k + 1: every script of cost <= k fits)."""
    assert a.n == b.n
    n, dev = a.n, a.blob.device
    if cap is None:
        cap = min(2 * int(k) + 1, 2 * max(a.longest(), b.longest(), 1) + 1)
    out = _out(n, dev) if out is None else out
    edits = torch.empty((n, cap, 2), dtype=torch.int64, device=dev) if edits is None else edits
    n_edits = torch.empty(n, dtype=torch.int32, device=dev) if n_edits is None else n_edits
    cc = _costs(costs)._c()
    rc = _n.lib().ta_levenshtein_trace_batch(a._ref(), b._ref(), n, k, _C.byref(cc), out.data_ptr(), edits.data_ptr(), n_edits.data_ptr(),
                                              cap, _stream())
    if rc:
        _raise(rc)
    return out, edits, n_edits


def edits_to_lists(edits, n_edits, allow_cut=False):
    """the device result of levenshtein_trace_batch as Python lists [(name, count), ...] per pair (host copy).  A script that did
    not fit the `cap` records of its pair was cut on the device (n_edits says how long it is): that is an error here, not a
    silently shorter script, unless the caller asks for the cut scripts (allow_cut)."""
    e, ne = edits.cpu().numpy(), n_edits.cpu().numpy()
    cut = [i for i in range(len(ne)) if int(ne[i]) > e.shape[1]]
    if cut and not allow_cut:
        raise ValueError("levenshtein_trace_batch: %d script(s) longer than cap = %d runs (first: pair %d with %d runs); pass a larger cap"
                         % (len(cut), e.shape[1], cut[0], int(ne[cut[0]])))
    return [[(_EDIT_NAMES[int(e[i, t, 0]) & 0xFFFFFFFF], int(e[i, t, 1])) for t in range(min(int(ne[i]), e.shape[1]))] for i in range(len(ne))]


def levenshtein_trace_batch_packed(a: Strings, b: Strings, k, costs=LEVENSHTEIN_COSTS, cap=None, out=None, packed=None, n_edits=None):
    """levenshtein_trace_batch with PACKED records (ta_levenshtein_trace_batch_packed): -> (out, packed, n_edits); packed is (n, cap) int32,
    one word per run -- (edit type << 29) | count -- pair i's script the min(n_edits[i], cap) words at the END of row i, front to back (words in
    front of a script are not written).  A quarter of the bytes of the (n, cap, 2) int64 form; packed_to_lists expands it on the host."""
    assert a.n == b.n
    n, dev = a.n, a.blob.device
    if cap is None:
        cap = min(2 * int(k) + 1, 2 * max(a.longest(), b.longest(), 1) + 1)
    out = _out(n, dev) if out is None else out
    packed = torch.empty((n, cap), dtype=torch.int32, device=dev) if packed is None else packed
    n_edits = torch.empty(n, dtype=torch.int32, device=dev) if n_edits is None else n_edits
    cc = _costs(costs)._c()
    rc = _n.lib().ta_levenshtein_trace_batch_packed(a._ref(), b._ref(), n, k, _C.byref(cc), out.data_ptr(), packed.data_ptr(), n_edits.data_ptr(),
                                                     cap, _stream())
    if rc:
        _raise(rc)
    return out, packed, n_edits


def packed_to_lists(packed, n_edits, allow_cut=False):
    """the result of levenshtein_trace_batch_packed as Python lists [(name, count), ...] per pair (host copy); a script longer than the row
    is an error unless allow_cut (then its LAST cap runs are returned)."""
    import numpy as np
    p, ne = packed.cpu().numpy().view(np.uint32), n_edits.cpu().numpy()
    cap = p.shape[1]
    cut = [i for i in range(len(ne)) if int(ne[i]) > cap]
    if cut and not allow_cut:
        raise ValueError("levenshtein_trace_batch_packed: %d script(s) longer than cap = %d runs (first: pair %d with %d runs); pass a larger cap"
                         % (len(cut), cap, cut[0], int(ne[cut[0]])))
    return [[(_EDIT_NAMES[int(w) >> 29], int(w) & 0x1FFFFFFF) for w in p[i, cap - min(int(ne[i]), cap):]] for i in range(len(ne))]


# ---------------------------------------------------------------- sequences of 32-bit items (token ids) resident in HBM
def _token_values(t):
    """int32 (taken as its u32 bit pattern) or int64 (checked to lie in [0, 2^32)) -> a contiguous int32 tensor of the same bits"""
    if t.dtype == torch.int64:
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= 1 << 32):
            raise ValueError("token values must lie in [0, 2^32)")
        t = torch.where(t >= 1 << 31, t - (1 << 32), t).to(torch.int32)
    if t.dtype != torch.int32:
        raise TypeError("token values: int32 or int64, got %s" % t.dtype)
    return t.contiguous()


class Tokens:
    """A batch side of 32-bit item sequences in HBM (Strings for token ids): CSR (values + n+1 int64 element offsets) or a fixed
    (n, len) tensor.  No read slack is needed.  stride: the distance in items of two sequences of the strided form (default: length)."""

    def __init__(self, values, off=None, length=0, max_len=0, n=None, stride=None):
        values = _token_values(values)
        assert values.is_cuda
        self.values, self.off, self.max_len = values, off, max_len
        if off is not None:
            assert off.dtype == torch.int64 and off.is_cuda and off.is_contiguous()
            self.n, self.length, self.stride = off.numel() - 1, 0, 0
        else:
            self.n, self.length, self.stride = n, length, length if stride is None else stride

    def __setattr__(self, name, value):
        # the C view is built once per batch side (_ref); changing a field drops it
        if name in ("values", "off", "stride", "length", "max_len"):
            self.__dict__.pop("_cview", None)
            self.__dict__.pop("_cref", None)
        object.__setattr__(self, name, value)

    @classmethod
    def from_csr(cls, values, off, max_len=0):
        return cls(values, off, max_len=max_len)

    @classmethod
    def from_fixed(cls, array_2d, device="cuda"):
        """(n, len) int32 / int64 tensor or array -> strided side"""
        t = torch.as_tensor(array_2d)
        n, length = t.shape
        return cls(_token_values(t.to(device)).reshape(-1), None, length=length, n=n)

    @classmethod
    def from_list(cls, seqs, device="cuda"):
        """a list of int sequences (values in [0, 2^32)) -> CSR side"""
        import numpy as np
        lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=len(seqs))
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        vals = np.zeros(int(off[-1]), dtype=np.int64)
        if off[-1]:
            vals[:] = np.concatenate([np.asarray(s, dtype=np.int64).reshape(-1) for s in seqs if len(s)])
        return cls(torch.from_numpy(vals).to(device), torch.from_numpy(off).to(device), max_len=int(lens.max()) if len(seqs) else 0)

    def longest(self):
        if self.off is None:
            return int(self.length)
        if not self.max_len and self.n > 0:
            self.max_len = int((self.off[1:] - self.off[:-1]).max().item())
        return int(self.max_len)

    def _ref(self):
        c = self.__dict__.get("_cview")
        if c is None:
            # CSR: `len` carries the items the values hold (the bound of off[n]: the library then needs no synchronisation for it)
            c = self._cview = _n.TokensC(self.values.data_ptr(), 0 if self.off is None else self.off.data_ptr(), self.stride,
                                         self.length if self.off is None else self.values.numel(), self.max_len)
            self._cref = _C.byref(c)
        return self._cref


def levenshtein_k_batch_tokens(a: Tokens, b: Tokens, k, costs=LEVENSHTEIN_COSTS, out=None):
    """levenshtein_k_batch over token sequences: out[i] = the distance of pair i if <= k, else -1 (int32)."""
    assert a.n == b.n
    a.longest(), b.longest()
    out = _out(a.n, a.values.device) if out is None else out
    cc = _costs(costs)._c()
    rc = _n.lib().ta_levenshtein_k_batch_tokens(a._ref(), b._ref(), a.n, k, _C.byref(cc), out.data_ptr(), _stream())
    if rc:
        _raise(rc)
    return out


def levenshtein_exp_batch_tokens(a: Tokens, b: Tokens, costs=LEVENSHTEIN_COSTS, out=None):
    """levenshtein_exp_batch over token sequences (the distance of every pair)"""
    assert a.n == b.n
    a.longest(), b.longest()
    out = _out(a.n, a.values.device) if out is None else out
    cc = _costs(costs)._c()
    _raise(_n.lib().ta_levenshtein_exp_batch_tokens(a._ref(), b._ref(), a.n, _C.byref(cc), out.data_ptr(), _stream()))
    return out


def levenshtein_trace_batch_tokens(a: Tokens, b: Tokens, k, costs=LEVENSHTEIN_COSTS, cap=None, out=None, edits=None, n_edits=None):
    """levenshtein_trace_batch over token sequences: -> (out, edits, n_edits) as levenshtein_trace_batch returns them."""
    assert a.n == b.n
    n, dev = a.n, a.values.device
    if cap is None:
        cap = min(2 * int(k) + 1, 2 * max(a.longest(), b.longest(), 1) + 1)
    a.longest(), b.longest()
    out = _out(n, dev) if out is None else out
    edits = torch.empty((n, cap, 2), dtype=torch.int64, device=dev) if edits is None else edits
    n_edits = torch.empty(n, dtype=torch.int32, device=dev) if n_edits is None else n_edits
    cc = _costs(costs)._c()
    rc = _n.lib().ta_levenshtein_trace_batch_tokens(a._ref(), b._ref(), n, k, _C.byref(cc), out.data_ptr(), edits.data_ptr(),
                                                    n_edits.data_ptr(), cap, _stream())
    if rc:
        _raise(rc)
    return out, edits, n_edits


def hamming_batch(a: Strings, b: Strings, out=None):
    assert a.n == b.n
    out = _out(a.n, a.blob.device) if out is None else out
    rc = _n.lib().ta_hamming_batch(a._ref(), b._ref(), a.n, out.data_ptr(), _stream())
    if rc:
        _raise(rc)
    return out


def hamming_dev(a, b, out=None):
    """hamming(a, b) (src/hamming.rs:390) of ONE pair that lies in HBM (ta_hamming_dev): two 1-D contiguous torch.uint8 CUDA tensors of
    the same length -- views at any storage offset are fine, no read slack is needed -- -> a 1-element device tensor.  From 64 KiB on the
    pair is cut into slices spread over the whole chip.  Asynchronous on the current stream; capturable after one call outside the capture."""
    for t in (a, b):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.is_cuda and t.dim() == 1 and t.is_contiguous()):
            raise ValueError("hamming_dev: 1-D contiguous torch.uint8 CUDA tensors")
    if a.numel() != b.numel():
        _raise(_n.TA_ERR_LEN_MISMATCH)                          # assert!(a.len() == b.len()), src/hamming.rs:318
    out = _out(1, a.device) if out is None else out
    rc = _n.lib().ta_hamming_dev(a.data_ptr() if a.numel() else None, b.data_ptr() if b.numel() else None, a.numel(), out.data_ptr(), _stream())
    if rc:
        _raise(rc)
    return out


# ---------------------------------------------------------------- search on a haystack shard resident in HBM
def _hits_to_numpy(hits_t, count):
    """(start, end, k) rows sorted by end.  An end position is reported at most once per call, so `end` alone orders
    the hits; the sort runs on the device and one copy brings the rows to the host."""
    import numpy as np
    if count == 0:
        return np.empty((0, 3), dtype=np.int64)
    v = hits_t[: count * 3].view(-1, 3)                                # (start, end, k|pad) as int64 triples
    out = v[torch.argsort(v[:, 1])].cpu().numpy()
    out[:, 2] &= 0xFFFFFFFF
    return out


import threading as _threading

_hit_bufs = _threading.local()


def _hit_buffer(device, cap):
    """Reused device buffer for hit records (24 B each), one per calling thread (concurrent callers' kernels write their hits into it)."""
    key = (str(device), cap)
    bufs = _hit_bufs.__dict__.setdefault("bufs", {})
    if key not in bufs:
        bufs.clear()
        bufs[key] = torch.empty(cap * 3, dtype=torch.int64, device=device)
    return bufs[key]


def levenshtein_search_dev(needle, haystack, k, costs=LEVENSHTEIN_COSTS, anchored=False, base=0, emit_from=0, cap=None):
    """All-mode hits of levenshtein_search_simd_with_opts over a uint8 CUDA tensor (with >= 16 B of read slack
    after `length`): int64 array of rows (start, end, k) sorted by end.  `base` offsets the positions,
    hits with end <= emit_from are suppressed (left-halo positions of a sharded haystack)."""
    hay, length = haystack if isinstance(haystack, tuple) else (haystack, haystack.numel() - SLACK)
    assert hay.dtype == torch.uint8 and hay.is_cuda and hay.is_contiguous()
    needle = bytes(needle)
    cap = cap or min(length + 2, 1 << 22)
    hits = _hit_buffer(hay.device, cap)
    count = _C.c_uint64()
    cc = _costs(costs)._c()
    rc = _n.lib().ta_levenshtein_search_dev(needle, len(needle), hay.data_ptr(), length, k, _C.byref(cc), int(anchored),
                                            base, emit_from, hits.data_ptr(), cap, _C.byref(count), _stream())
    _raise(rc)
    return _hits_to_numpy(hits, int(count.value))


def levenshtein_search_best_dev(needle, haystack, k, costs=LEVENSHTEIN_COSTS, base=0, emit_from=0, cap=None):
    """The hits of levenshtein_search_dev that can survive the Best fold (those with the smallest k), selected on the
    device: int64 rows (start, end, k) sorted by end -- feed them to dist.fold_best.  Only these few records leave HBM."""
    import numpy as np
    hay, length = haystack if isinstance(haystack, tuple) else (haystack, haystack.numel() - SLACK)
    assert hay.dtype == torch.uint8 and hay.is_cuda and hay.is_contiguous()
    needle = bytes(needle)
    cap = cap or min(length + 2, 1 << 22)
    hits = _hit_buffer(hay.device, cap)
    count = _C.c_uint64()
    cc = _costs(costs)._c()
    out = _C.POINTER(_n.MatchC)()
    n_out = _C.c_size_t()
    rc = _n.lib().ta_levenshtein_search_best_dev(needle, len(needle), hay.data_ptr(), length, k, _C.byref(cc), base, emit_from,
                                                 hits.data_ptr(), cap, _C.byref(count), _C.byref(out), _C.byref(n_out), _stream())
    _raise(rc)
    rows = np.empty((n_out.value, 3), dtype=np.int64)
    for i in range(n_out.value):
        rows[i] = (out[i].start, out[i].end, out[i].k)
    _n.lib().ta_free(out)
    return rows


def levenshtein_search_first_dev(needle, haystack, k, costs=LEVENSHTEIN_COSTS, base=0):
    """The first All-mode hit (smallest end) of a resident haystack shard, or None: the shard is searched window by window and the
    scan stops at the first window that holds a hit (`.next()` on the reference's lazy iterator, src/levenshtein.rs:2282-2420)."""
    hay, length = haystack if isinstance(haystack, tuple) else (haystack, haystack.numel() - SLACK)
    assert hay.dtype == torch.uint8 and hay.is_cuda and hay.is_contiguous()
    needle = bytes(needle)
    m, found = _n.MatchC(), _C.c_int()
    cc = _costs(costs)._c()
    _raise(_n.lib().ta_levenshtein_search_first_dev(needle, len(needle), hay.data_ptr(), length, k, _C.byref(cc), base,
                                                    _C.byref(m), _C.byref(found), _stream()))
    return (int(m.start), int(m.end), int(m.k)) if found.value else None


def hamming_search_dev(needle, haystack, k, base=0, cap=None):
    hay, length = haystack if isinstance(haystack, tuple) else (haystack, haystack.numel() - SLACK)
    needle = bytes(needle)
    cap = cap or min(length + 2, 1 << 22)
    hits = _hit_buffer(hay.device, cap)
    # the hits on the host, sorted by end: the few hits of an ordinary search arrive through pinned memory with the call's one
    # stream synchronisation (ta_hamming_search_dev_sorted; the count + a device-side sort + a copy cost 0.11 ms per call)
    import numpy as np
    out = _C.POINTER(_n.MatchC)()
    n_out = _C.c_size_t()
    rc = _n.lib().ta_hamming_search_dev_sorted(needle, len(needle), hay.data_ptr(), length, k, base, hits.data_ptr(), cap,
                                               _C.byref(out), _C.byref(n_out), _stream())
    _raise(rc)
    n = n_out.value
    if n == 0:
        return np.empty((0, 3), dtype=np.int64)
    raw = np.ctypeslib.as_array(_C.cast(out, _C.POINTER(_C.c_uint64)), shape=(n, 3)).astype(np.int64)     # (start, end, k | pad << 32)
    _n.lib().ta_free(out)
    raw[:, 2] &= 0xFFFFFFFF
    return raw


def haystack_tensor(data, device="cuda"):
    """bytes / uint8 array -> (CUDA tensor with read slack, length)."""
    import numpy as np
    arr = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.asarray(data, dtype=np.uint8)
    t = torch.zeros(arr.size + SLACK, dtype=torch.uint8, device=device)
    t[: arr.size] = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
    return t, arr.size


def levenshtein_search_batch(needles: Strings, haystacks: Strings, k, search_type=SearchType.Best, costs=LEVENSHTEIN_COSTS, anchored=False, cap=None,
                             matches=None, counts=None):
    """levenshtein_search_simd_with_opts(needle_i, haystack_i, k, search_type, costs, anchored) for every pair, on the device:
    -> (matches, counts).  counts[i] (int32) = the length of pair i's result; matches[i, :min(counts[i], cap)] = its first `cap`
    matches as int64 (start, end, k) rows, positions relative to haystack i, in increasing end.  cap = 0: counts only.
    needles may be Strings.shared(needle, n): one needle for every pair.  Default cap: 8 (search_type Best) or 64 (All)."""
    st = search_type
    n, dev = haystacks.n, haystacks.blob.device
    assert needles.n == n
    if cap is None:
        cap = 8 if st == SearchType.Best else 64
    matches = torch.empty((n, cap, 3), dtype=torch.int64, device=dev) if matches is None else matches
    counts = torch.empty(n, dtype=torch.int32, device=dev) if counts is None else counts
    assert matches.dtype == torch.int64 and matches.is_contiguous() and matches.numel() >= n * cap * 3
    assert counts.dtype == torch.int32 and counts.numel() >= n
    cc = _costs(costs)._c()
    rc = _n.lib().ta_levenshtein_search_batch(needles._ref(), haystacks._ref(), n, int(k), int(st), _C.byref(cc), int(bool(anchored)),
                                              matches.data_ptr() if cap else None, counts.data_ptr(), cap, _stream())
    if rc:
        _raise(rc)
    return matches, counts


def hamming_search_batch(needles: Strings, haystacks: Strings, k, search_type=SearchType.Best, cap=None, matches=None, counts=None):
    """hamming_search_simd_with_opts(needle_i, haystack_i, k, search_type) for every pair, on the device: -> (matches, counts), shaped as
    levenshtein_search_batch's.  counts[i] (int32) = the length of pair i's result, or -1 where the single call panics (a NUL byte in
    the haystack): that pair has no matches, the others are unaffected.  matches[i, :min(counts[i], cap)] = its first `cap` matches as
    int64 (start, end, k) rows, positions relative to haystack i, in increasing start.  cap = 0: counts only.  needles may be
    Strings.shared(needle, n): one needle for every pair.  Default cap: 8 (search_type Best) or 64 (All)."""
    st = search_type
    n, dev = haystacks.n, haystacks.blob.device
    assert needles.n == n
    if cap is None:
        cap = 8 if st == SearchType.Best else 64
    matches = torch.empty((n, cap, 3), dtype=torch.int64, device=dev) if matches is None else matches
    counts = torch.empty(n, dtype=torch.int32, device=dev) if counts is None else counts
    assert matches.dtype == torch.int64 and matches.is_contiguous() and matches.numel() >= n * cap * 3
    assert counts.dtype == torch.int32 and counts.numel() >= n
    rc = _n.lib().ta_hamming_search_batch(needles._ref(), haystacks._ref(), n, int(k), int(st),
                                          matches.data_ptr() if cap else None, counts.data_ptr(), cap, _stream())
    if rc:
        _raise(rc)
    return matches, counts


def matches_to_lists(matches, counts, allow_cut=False):
    """the device result of levenshtein_search_batch / hamming_search_batch as Python lists of triple_accel_amd.Match per pair (host
    copy).  A result longer than the `cap` rows of its pair was cut on the device (counts says how long it is): that is an error here,
    not a silently shorter list, unless the caller asks for the cut lists (allow_cut).  A negative count is hamming_search_batch's NUL
    verdict: the reference's panic, raised here for the first such pair."""
    from . import Match, PanicError
    m, c = matches.cpu().numpy(), counts.cpu().numpy().astype("int64")
    cap = m.shape[1]
    nul = [i for i in range(len(c)) if int(c[i]) < 0]
    if nul:
        raise PanicError("No zero/null bytes allowed in the string! (pair %d)" % nul[0])
    cut = [i for i in range(len(c)) if int(c[i]) > cap]
    if cut and not allow_cut:
        raise ValueError("search batch: %d result(s) longer than cap = %d matches (first: pair %d with %d); pass a larger cap"
                         % (len(cut), cap, cut[0], int(c[cut[0]])))
    return [[Match(int(r[0]), int(r[1]), int(r[2]) & 0xFFFFFFFF) for r in m[i, :min(int(c[i]), cap)]] for i in range(len(c))]


def levenshtein_cross(queries: Strings, targets: Strings, k, costs=LEVENSHTEIN_COSTS, cap=None, hits=None, count=None, nearest=False):
    """Every query against every target within k, on the device (ta_levenshtein_cross): -> (hits, count, nearest).  The pair (q, t) is a
    hit with distance d exactly when levenshtein_simd_k_with_opts(query q, target t, k, false, costs) is Some(d).  count (int64, one
    element) = the number of hits whatever cap is; hits[:min(count, cap)] = that many distinct hits as int32 (query, target, d, 0) rows in
    no particular order (cross_to_arrays sorts them).  cap = 0: the count only.  nearest = True (or an int64 tensor of queries.n elements
    to reuse): nearest[q] = d << 32 | t of query q's nearest target -- the smallest distance, then the lowest index -- and -1 where q has
    no hit, whatever cap is; else None.  LEVENSHTEIN_COSTS, RDAMERAU_COSTS and their multiples (g, g, 0, None | g); queries of at most 64
    bytes (swap the sides when the short strings are the targets: the distance is symmetric).  Default cap: room for eight hits per
    string of the longer side (at least 1,024, at most every pair).  Nothing is synchronised: read count before trusting hits."""
    nq, nt, dev = queries.n, targets.n, targets.blob.device
    if cap is None:
        cap = hits.numel() // 4 if hits is not None else min(nq * nt, max(1024, 8 * max(nq, nt)))
    hits = torch.empty((cap, 4), dtype=torch.int32, device=dev) if hits is None else hits
    count = torch.empty(1, dtype=torch.int64, device=dev) if count is None else count
    if nearest is True:
        nearest = torch.empty(nq, dtype=torch.int64, device=dev)
    elif nearest is False:
        nearest = None
    assert hits.dtype == torch.int32 and hits.is_contiguous() and hits.numel() >= cap * 4
    assert count.dtype == torch.int64 and count.numel() >= 1
    assert nearest is None or (nearest.dtype == torch.int64 and nearest.is_contiguous() and nearest.numel() >= nq)
    cc = _costs(costs)._c()
    rc = _n.lib().ta_levenshtein_cross(queries._ref(), nq, targets._ref(), nt, int(k), _C.byref(cc), hits.data_ptr() if cap else None,
                                       count.data_ptr(), cap, None if nearest is None else nearest.data_ptr(), _stream())
    if rc:
        _raise(rc)
    return hits, count, nearest


def hamming_cross(queries: Strings, targets: Strings, k, cap=None, hits=None, count=None, nearest=False, per_query=False, upper=False):
    """Every query against every target within k mismatches, on the device (ta_hamming_cross): -> (hits, count, nearest, per_query).  The
    pair (q, t) is a hit with distance d exactly when both strings have the same length and hamming(query q, target t) = d <= k; strings
    of different lengths are never a hit.  hits, count, nearest and cap are levenshtein_cross's (cross_to_arrays reads them).
    per_query = True (or an int32 tensor of queries.n elements to reuse): per_query[q] = the number of hits of query q, whatever cap is;
    else None.  upper = True keeps only the pairs with target index > query index, in every output: a set against itself gives each
    unordered pair once.  Queries of at most 64 bytes.  Nothing is synchronised: read count before trusting hits."""
    nq, nt, dev = queries.n, targets.n, targets.blob.device
    if cap is None:
        cap = hits.numel() // 4 if hits is not None else min(nq * nt, max(1024, 8 * max(nq, nt)))
    hits = torch.empty((cap, 4), dtype=torch.int32, device=dev) if hits is None else hits
    count = torch.empty(1, dtype=torch.int64, device=dev) if count is None else count
    if nearest is True:
        nearest = torch.empty(nq, dtype=torch.int64, device=dev)
    elif nearest is False:
        nearest = None
    if per_query is True:
        per_query = torch.empty(nq, dtype=torch.int32, device=dev)
    elif per_query is False:
        per_query = None
    assert hits.dtype == torch.int32 and hits.is_contiguous() and hits.numel() >= cap * 4
    assert count.dtype == torch.int64 and count.numel() >= 1
    assert nearest is None or (nearest.dtype == torch.int64 and nearest.is_contiguous() and nearest.numel() >= nq)
    assert per_query is None or (per_query.dtype == torch.int32 and per_query.is_contiguous() and per_query.numel() >= nq)
    rc = _n.lib().ta_hamming_cross(queries._ref(), nq, targets._ref(), nt, int(k), _n.TA_CROSS_UPPER if upper else 0,
                                   hits.data_ptr() if cap else None, count.data_ptr(), cap,
                                   None if nearest is None else nearest.data_ptr(), None if per_query is None else per_query.data_ptr(), _stream())
    if rc:
        _raise(rc)
    return hits, count, nearest, per_query


def levenshtein_cross_with_opts(queries: Strings, targets: Strings, k, costs=LEVENSHTEIN_COSTS, cap=None, hits=None, count=None, nearest=False,
                                per_query=False, upper=False):
    """levenshtein_cross with queries of up to 256 bytes and hamming_cross's two further outputs, on the device
    (ta_levenshtein_cross_with_opts): -> (hits, count, nearest, per_query).  The hit rule, hits, count, nearest, cap and the costs are
    levenshtein_cross's; per_query = True (or an int32 tensor of queries.n elements to reuse): per_query[q] = the number of hits of query
    q, whatever cap is; else None.  upper = True keeps only the pairs with target index > query index, in every output: a set against
    itself gives each unordered pair once.  A query longer than 256 bytes raises NotImplementedError.  Nothing is synchronised: read
    count before trusting hits."""
    nq, nt, dev = queries.n, targets.n, targets.blob.device
    if cap is None:
        cap = hits.numel() // 4 if hits is not None else min(nq * nt, max(1024, 8 * max(nq, nt)))
    hits = torch.empty((cap, 4), dtype=torch.int32, device=dev) if hits is None else hits
    count = torch.empty(1, dtype=torch.int64, device=dev) if count is None else count
    if nearest is True:
        nearest = torch.empty(nq, dtype=torch.int64, device=dev)
    elif nearest is False:
        nearest = None
    if per_query is True:
        per_query = torch.empty(nq, dtype=torch.int32, device=dev)
    elif per_query is False:
        per_query = None
    assert hits.dtype == torch.int32 and hits.is_contiguous() and hits.numel() >= cap * 4
    assert count.dtype == torch.int64 and count.numel() >= 1
    assert nearest is None or (nearest.dtype == torch.int64 and nearest.is_contiguous() and nearest.numel() >= nq)
    assert per_query is None or (per_query.dtype == torch.int32 and per_query.is_contiguous() and per_query.numel() >= nq)
    cc = _costs(costs)._c()
    rc = _n.lib().ta_levenshtein_cross_with_opts(queries._ref(), nq, targets._ref(), nt, int(k), _C.byref(cc), _n.TA_CROSS_UPPER if upper else 0,
                                                 hits.data_ptr() if cap else None, count.data_ptr(), cap,
                                                 None if nearest is None else nearest.data_ptr(),
                                                 None if per_query is None else per_query.data_ptr(), _stream())
    if rc:
        _raise(rc)
    return hits, count, nearest, per_query


def levenshtein_cross_tokens(queries: Tokens, targets: Tokens, k, costs=LEVENSHTEIN_COSTS, cap=None, hits=None, count=None, nearest=False,
                             per_query=False, upper=False):
    """levenshtein_cross_with_opts over token sequences, on the device (ta_levenshtein_cross_tokens): -> (hits, count, nearest, per_query).
    The pair (q, t) is a hit with distance d exactly when levenshtein_k_batch_tokens answers d for it; hits, count, cap, nearest,
    per_query, upper and the costs are levenshtein_cross_with_opts's (cross_to_arrays reads the result).  Queries of at most 64 tokens
    (swap the sides when the short sequences are the targets: the distance is symmetric): a longer one raises NotImplementedError.  A
    CSR side with max_len = 0 is measured by the library (one synchronisation).  Nothing else is synchronised: read count before
    trusting hits."""
    nq, nt, dev = queries.n, targets.n, targets.values.device
    if cap is None:
        cap = hits.numel() // 4 if hits is not None else min(nq * nt, max(1024, 8 * max(nq, nt)))
    hits = torch.empty((cap, 4), dtype=torch.int32, device=dev) if hits is None else hits
    count = torch.empty(1, dtype=torch.int64, device=dev) if count is None else count
    if nearest is True:
        nearest = torch.empty(nq, dtype=torch.int64, device=dev)
    elif nearest is False:
        nearest = None
    if per_query is True:
        per_query = torch.empty(nq, dtype=torch.int32, device=dev)
    elif per_query is False:
        per_query = None
    assert hits.dtype == torch.int32 and hits.is_contiguous() and hits.numel() >= cap * 4
    assert count.dtype == torch.int64 and count.numel() >= 1
    assert nearest is None or (nearest.dtype == torch.int64 and nearest.is_contiguous() and nearest.numel() >= nq)
    assert per_query is None or (per_query.dtype == torch.int32 and per_query.is_contiguous() and per_query.numel() >= nq)
    cc = _costs(costs)._c()
    rc = _n.lib().ta_levenshtein_cross_tokens(queries._ref(), nq, targets._ref(), nt, int(k), _C.byref(cc), _n.TA_CROSS_UPPER if upper else 0,
                                              hits.data_ptr() if cap else None, count.data_ptr(), cap,
                                              None if nearest is None else nearest.data_ptr(),
                                              None if per_query is None else per_query.data_ptr(), _stream())
    if rc:
        _raise(rc)
    return hits, count, nearest, per_query


def cross_to_arrays(hits, count, allow_cut=False):
    """the device result of levenshtein_cross as numpy arrays (query, target, k), sorted by (query, target) (host copy).  More hits than
    the `cap` rows of `hits` were cut on the device (count says how many there are): that is an error here, not a silently shorter
    result, unless the caller asks for the cut one (allow_cut)."""
    import numpy as np
    n, cap = int(count.cpu()[0].item()), hits.shape[0]
    if n > cap and not allow_cut:
        raise ValueError("cross: %d hits for cap = %d records; pass a larger cap" % (n, cap))
    h = hits[:min(n, cap)].cpu().numpy().view(np.uint32).reshape(-1, 4)
    order = np.lexsort((h[:, 1], h[:, 0]))
    h = h[order]
    return h[:, 0].copy(), h[:, 1].copy(), h[:, 2].copy()


def _search_cross_call(entry, needles, haystacks, k, costs, anchored, cap, hits, count, nearest, best, per_haystack):
    """the buffers, the call and the status of both levenshtein_search_cross entries; entry(*leading, *trailing arguments) -> status"""
    nn, nh, dev = needles.n, haystacks.n, haystacks.blob.device
    if cap is None:
        cap = hits.numel() // 6 if hits is not None else min(nn * nh, max(1024, 8 * nh))
    hits = torch.empty((cap, 6), dtype=torch.int32, device=dev) if hits is None else hits
    count = torch.empty(1, dtype=torch.int64, device=dev) if count is None else count
    nearest = torch.empty(nh, dtype=torch.int64, device=dev) if nearest is True else None if nearest is False else nearest
    best = torch.empty((nh, 3), dtype=torch.int64, device=dev) if best is True else None if best is False else best
    per_haystack = torch.empty(nh, dtype=torch.int32, device=dev) if per_haystack is True else None if per_haystack is False else per_haystack
    assert hits.dtype == torch.int32 and hits.is_contiguous() and hits.numel() >= cap * 6
    assert count.dtype == torch.int64 and count.numel() >= 1
    assert nearest is None or (nearest.dtype == torch.int64 and nearest.is_contiguous() and nearest.numel() >= nh)
    assert best is None or (best.dtype == torch.int64 and best.is_contiguous() and best.numel() >= nh * 3)
    assert per_haystack is None or (per_haystack.dtype == torch.int32 and per_haystack.is_contiguous() and per_haystack.numel() >= nh)
    cc = _costs(costs)._c()
    rc = entry((needles._ref(), nn, haystacks._ref(), nh, int(k), _C.byref(cc), int(bool(anchored))),
               (hits.data_ptr() if cap else None, count.data_ptr(), cap,
                None if nearest is None else nearest.data_ptr(), None if best is None else best.data_ptr(),
                None if per_haystack is None else per_haystack.data_ptr(), _stream()))
    if rc:
        _raise(rc)
    return hits, count, nearest, best, per_haystack


def levenshtein_search_cross(needles: Strings, haystacks: Strings, k, costs=LEVENSHTEIN_COSTS, anchored=False, cap=None, hits=None, count=None,
                             nearest=False, best=False, per_haystack=False):
    """Every needle of a panel searched in every haystack within k, on the device (ta_levenshtein_search_cross): -> (hits, count, nearest,
    best, per_haystack).  For needle p and haystack i let R = levenshtein_search_simd_with_opts(needle p, haystack i, k, SearchType.Best,
    costs, anchored): the pair is a hit exactly when R is not empty.  count (int64, one element) = the number of hits whatever cap is;
    hits[:min(count, cap)] = that many distinct hits as int32 (haystack, needle, R[0].start, R[0].end, R[0].k, len(R)) rows in no
    particular order (search_cross_to_arrays sorts them).  cap = 0: the count only.  nearest = True (or an int64 tensor of haystacks.n
    elements to reuse): nearest[i] = R[0].k << 32 | p of haystack i's cheapest needle -- at equal cost the lowest index -- and -1 where no
    needle hits.  best = True (or an int64 (haystacks.n, 3) tensor): that needle's R[0] as a (start, end, k) row, (0, 0, 0xFFFFFFFF) where
    no needle hits; it does not need nearest.  per_haystack = True (or an int32 tensor): the number of needles that hit haystack i.  None
    of the three depends on cap; each is None when not asked for.  Needles of at most 32 bytes, at most 65,535 of them.  Default cap: room
    for eight hits per haystack (at least 1,024, at most every pair).  Nothing is synchronised: read count before trusting hits."""
    return _search_cross_call(lambda a, b: _n.lib().ta_levenshtein_search_cross(*a, *b), needles, haystacks, k, costs, anchored, cap, hits, count,
                              nearest, best, per_haystack)


def levenshtein_search_cross_with_opts(needles: Strings, haystacks: Strings, k, costs=LEVENSHTEIN_COSTS, anchored=False, cap=None, hits=None,
                                       count=None, nearest=False, best=False, per_haystack=False):
    """levenshtein_search_cross for needles of at most 64 bytes (ta_levenshtein_search_cross_with_opts, its flags word 0): the same
    arguments, the same five results, the same exceptions.  A panel whose longest needle is at most 32 bytes runs the same kernels as
    levenshtein_search_cross; a longer one takes the two-word route as a whole -- a few long adapters beside many short barcodes are
    better served by one call of each entry."""
    return _search_cross_call(lambda a, b: _n.lib().ta_levenshtein_search_cross_with_opts(*a, 0, *b), needles, haystacks, k, costs, anchored, cap,
                              hits, count, nearest, best, per_haystack)


def search_cross_to_arrays(hits, count, allow_cut=False):
    """the device result of levenshtein_search_cross as numpy arrays (haystack, needle, start, end, k, n_matches), sorted by (haystack,
    needle) (host copy).  More hits than the `cap` rows of `hits` were cut on the device (count says how many there are): that is an
    error here, not a silently shorter result, unless the caller asks for the cut one (allow_cut)."""
    import numpy as np
    n, cap = int(count.cpu()[0].item()), hits.shape[0]
    if n > cap and not allow_cut:
        raise ValueError("search cross: %d hits for cap = %d records; pass a larger cap" % (n, cap))
    h = hits[:min(n, cap)].cpu().numpy().view(np.uint32).reshape(-1, 6)
    h = h[np.lexsort((h[:, 1], h[:, 0]))]
    return tuple(h[:, c].copy() for c in range(6))


def _hamming_search_cross_call(entry, needles, haystacks, k, cap, hits, count, nearest, best, per_haystack):
    """hamming_search_cross and hamming_search_cross_with_opts: entry(a, b) calls the C function with a = (needles .. k), b = (hits ..)"""
    nn, nh, dev = needles.n, haystacks.n, haystacks.blob.device
    if cap is None:
        cap = hits.numel() // 6 if hits is not None else min(nn * nh, max(1024, 8 * nh))
    hits = torch.empty((cap, 6), dtype=torch.int32, device=dev) if hits is None else hits
    count = torch.empty(1, dtype=torch.int64, device=dev) if count is None else count
    nearest = torch.empty(nh, dtype=torch.int64, device=dev) if nearest is True else None if nearest is False else nearest
    best = torch.empty((nh, 3), dtype=torch.int64, device=dev) if best is True else None if best is False else best
    per_haystack = torch.empty(nh, dtype=torch.int32, device=dev) if per_haystack is True else None if per_haystack is False else per_haystack
    assert hits.dtype == torch.int32 and hits.is_contiguous() and hits.numel() >= cap * 6
    assert count.dtype == torch.int64 and count.numel() >= 1
    assert nearest is None or (nearest.dtype == torch.int64 and nearest.is_contiguous() and nearest.numel() >= nh)
    assert best is None or (best.dtype == torch.int64 and best.is_contiguous() and best.numel() >= nh * 3)
    assert per_haystack is None or (per_haystack.dtype == torch.int32 and per_haystack.is_contiguous() and per_haystack.numel() >= nh)
    rc = entry((needles._ref(), nn, haystacks._ref(), nh, int(k)),
               (hits.data_ptr() if cap else None, count.data_ptr(), cap, None if nearest is None else nearest.data_ptr(),
                None if best is None else best.data_ptr(), None if per_haystack is None else per_haystack.data_ptr(), _stream()))
    if rc:
        _raise(rc)
    return hits, count, nearest, best, per_haystack


def hamming_search_cross(needles: Strings, haystacks: Strings, k, cap=None, hits=None, count=None, nearest=False, best=False, per_haystack=False):
    """Every needle of a panel searched in every haystack within k MISMATCHES, on the device (ta_hamming_search_cross): -> (hits, count,
    nearest, best, per_haystack), shaped as levenshtein_search_cross's (search_cross_to_arrays reads hits and count).  For needle p and
    haystack i let R = hamming_search_simd_with_opts(needle p, haystack i, k, SearchType.Best): the pair is a hit exactly when R is not
    empty, its row is (haystack, needle, R[0].start, R[0].end, R[0].k, len(R)).  An empty needle never hits.  Where the single call
    panics -- a NUL byte in a haystack that is not shorter than the non-empty needle -- the pair has no row and touches neither nearest
    nor best, and per_haystack[i] = -1 for such a haystack: a caller who cannot rule out NUL bytes asks for per_haystack.  The other
    haystacks are unaffected.  Needles of at most 32 bytes, at most 65,535 of them.  Default cap: room for eight hits per haystack (at
    least 1,024, at most every pair).  Nothing is synchronised: read count before trusting hits."""
    return _hamming_search_cross_call(lambda a, b: _n.lib().ta_hamming_search_cross(*a, *b), needles, haystacks, k, cap, hits, count, nearest,
                                      best, per_haystack)


def hamming_search_cross_with_opts(needles: Strings, haystacks: Strings, k, cap=None, hits=None, count=None, nearest=False, best=False,
                                   per_haystack=False):
    """hamming_search_cross for needles of at most 64 bytes (ta_hamming_search_cross_with_opts, its flags word 0): the same arguments, the
    same five results, the same exceptions.  A panel whose longest needle is at most 32 bytes runs the same kernel as
    hamming_search_cross; a longer one takes the two-word route as a whole -- a few long adapters beside many short barcodes are better
    served by one call of each entry."""
    return _hamming_search_cross_call(lambda a, b: _n.lib().ta_hamming_search_cross_with_opts(*a, 0, *b), needles, haystacks, k, cap, hits,
                                      count, nearest, best, per_haystack)
