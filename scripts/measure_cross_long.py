"""Every query of up to 256 bytes against every target within k on one GPU: ta_levenshtein_cross_with_opts
  (a) as it routes itself: a window of the column, lev_cross_win_kernel<2 | 3 | 4, TRANS>;
  (b) against the route it replaces -- gather the pairs into two blobs in HBM (timed on its own), then ta_levenshtein_k_batch over the
      blobs (timed on its own), then filter the dense answer;
  (c) against itself forced to the whole column, lev_cross_win_kernel<8, TRANS> (TA_TUNING=1 TA_CROSS_FULL=1).
Workloads:
  reads_150       2,048 x 2,048 150-byte ACGT reads, 5 % of the queries a target with a few edits, k = 2, 8, 16 and 32: windows of 2, 2,
                  3 and 4 blocks ((b) gathers 1.3 GB);
  reads_150_16k   16,384 x 2,048 of the same at k = 2, 8, 16: (a) and (c) only; (b) still runs, 2,048 queries at a time, for the pair-for-pair check;
  set_100_upper   4,096 100-byte strings against themselves with TA_CROSS_UPPER, k = 3; (b) gathers the pairs i < j, 2,048 rows at a time
                  for the check, and is not timed.
Every row first checks (a) and (c) against the dense route, pair for pair (hits, distances, nearest words, per-query counts).  Times:
every route is warmed up, then timed in `--trials` windows of at least `--window-ms` each, the routes alternating inside a trial; a row
reports the median window and the fastest and slowest one.  One JSON line per row.  k = 32 is there beyond the three thresholds first asked
for because the routing keeps a window width only where it measured at least as fast as the whole column: without it the 4-block window
would have no figure."""
import argparse
import json
import os
import sys

os.environ.setdefault("TA_TUNING", "1")        # (TA_CROSS_FULL is honoured only under TA_TUNING; it is read at every call)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from triple_accel_amd import batch as B  # noqa: E402
from triple_accel_amd import _native as N  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fns, trials, window_ms):
    """{name: fn} -> {name: (median, fastest, slowest) ms per call}; the routes alternate inside every trial"""
    reps = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        once = max(window(fn, 2), 1e-3)
        reps[name] = max(2, int(window_ms / once) + 1)
    got = {name: [] for name in fns}
    for _ in range(trials):
        for name, fn in fns.items():
            got[name].append(window(fn, reps[name]))
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in got.items()}


def edit(rng, row, edits):
    """`edits` substitutions, insertions and deletions; the length is kept (cut or padded at the end)"""
    s = list(row)
    for _ in range(edits):
        kind, p = int(rng.integers(3)), int(rng.integers(len(s)))
        if kind == 0:
            s[p] = ACGT[rng.integers(4)]
        elif kind == 1:
            s.insert(p, ACGT[rng.integers(4)])
        else:
            del s[p]
    s = s[:len(row)] + [ACGT[rng.integers(4)] for _ in range(len(row) - len(s))]
    return np.array(s, np.uint8)


def reads(nq, nt, length, seed, max_edits, t=None):
    rng = np.random.default_rng(seed)
    t = ACGT[rng.integers(0, 4, (nt, length))] if t is None else t
    q = ACGT[rng.integers(0, 4, (nq, length))]
    for i in rng.choice(nq, nq // 20, replace=False):             # 5 % of the queries: a target with a few edits
        q[i] = edit(rng, t[rng.integers(nt)], int(rng.integers(0, max_edits + 1)))
    return q, t


def read_set(n, length, seed):
    rng = np.random.default_rng(seed)
    base = ACGT[rng.integers(0, 4, (n // 8, length))]             # eight reads per molecule, each with zero to two edits
    return np.stack([edit(rng, base[rng.integers(n // 8)], int(rng.integers(0, 3))) for _ in range(n)])


def gather(qs, ts, qi, ti):
    """the pairs (qi[p], ti[p]) materialised in HBM -> (a side, b side) for ta_levenshtein_k_batch"""
    n, ql, tl = qi.numel(), qs.length, ts.length
    a = torch.zeros(n * ql + 16, dtype=torch.uint8, device="cuda")
    b = torch.zeros(n * tl + 16, dtype=torch.uint8, device="cuda")
    a[: n * ql].view(n, ql).copy_(qs.blob[: qs.n * ql].view(qs.n, ql)[qi])
    b[: n * tl].view(n, tl).copy_(ts.blob[: ts.n * tl].view(ts.n, tl)[ti])
    return B.Strings(a, None, stride=ql, length=ql, n=n), B.Strings(b, None, stride=tl, length=tl, n=n)


def block_pairs(q0, q1, nt, upper):
    p = torch.arange((q1 - q0) * nt, device="cuda")
    qi, ti = q0 + p // nt, p % nt
    if upper:
        keep = ti > qi
        qi, ti = qi[keep], ti[keep]
    return qi, ti


def dense_hits(qs, ts, qi, ti, k):
    """the old route's answer: (q, t, d) rows of the pairs within k, sorted by (q, t)"""
    a, b = gather(qs, ts, qi, ti)
    d = B.levenshtein_k_batch(a, b, k)
    keep = torch.nonzero(d >= 0).flatten()
    rows = torch.stack([qi[keep], ti[keep], d[keep].long()], dim=1)
    return rows[torch.argsort(rows[:, 0] * ts.n + rows[:, 1])]


def agree(qs, want, out):
    """the cross outputs against the dense route's sorted rows, pair for pair (on the host)"""
    hits, count, nearest, per_query = out
    torch.cuda.synchronize()
    n = int(count.item())
    if n != want.shape[0]:
        return False
    got = hits[:n].cpu().numpy().astype(np.int64)
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    counts = np.bincount(want[:, 0], minlength=qs.n)
    words = np.full(qs.n, -1, dtype=np.int64).view(np.uint64)
    np.minimum.at(words, want[:, 0], ((want[:, 2] << 32) | want[:, 1]).astype(np.uint64))
    return bool((got[:, :3] == want).all()) and bool((per_query.cpu().numpy() == counts).all()) and \
        bool((nearest.cpu().numpy().view(np.uint64) == words).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=150.0)
    ap.add_argument("--scale", type=float, default=1.0, help="scales both sides of every workload (a quick run: 0.25)")
    ap.add_argument("--rows", default="reads_150,reads_150_16k,set_100_upper")
    ap.add_argument("--row-stride", type=int, default=9, help="recorded in every row as row_stride_dwords: the table's row stride the "
                    "library under test was built with (-DTA_WIN_ROW_DWORDS=8 | 9, lev_cross_win_body.h); the row-stride A/B of DESIGN 3.17 "
                    "is this script run once per build")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no other route"
    s = lambda n: max(64, int(n * args.scale))                                      # noqa: E731
    q150, t150 = reads(s(2048), s(2048), 150, 21, 16)
    q16k, _ = reads(s(16384), s(2048), 150, 22, 16, t150)
    set100 = read_set(s(4096), 100, 23)
    for name, q, t, upper, old_route, ks in (("reads_150", q150, t150, False, True, (2, 8, 16, 32)), ("reads_150_16k", q16k, t150, False, False, (2, 8, 16)),
                                             ("set_100_upper", set100, set100, True, False, (3,))):
        if name not in args.rows.split(","):
            continue
        qs, ts = B.Strings.from_fixed(q), B.Strings.from_fixed(t)
        nq, nt = qs.n, ts.n
        n_pairs = nq * (nt - 1) // 2 if upper else nq * nt
        count = torch.empty(1, dtype=torch.int64, device="cuda")
        nearest = torch.empty(nq, dtype=torch.int64, device="cuda")
        per_query = torch.empty(nq, dtype=torch.int32, device="cuda")
        for k in ks:
            os.environ.pop("TA_CROSS_FULL", None)
            B.levenshtein_cross_with_opts(qs, ts, k, cap=0, count=count, upper=upper)
            torch.cuda.synchronize()
            n_hits = int(count.item())
            hits = torch.empty((max(n_hits, 1), 4), dtype=torch.int32, device="cuda")

            def cross(full_column, **kw):
                if full_column:
                    os.environ["TA_CROSS_FULL"] = "1"
                else:
                    os.environ.pop("TA_CROSS_FULL", None)
                return B.levenshtein_cross_with_opts(qs, ts, k, upper=upper, **kw)

            outputs = dict(cap=n_hits, hits=hits, count=count, nearest=nearest, per_query=per_query)
            want = torch.cat([dense_hits(qs, ts, *block_pairs(q0, min(q0 + 2048, nq), nt, upper), k) for q0 in range(0, nq, 2048)]).cpu().numpy()
            same, kernels = {}, {}
            for route, full_column in (("window", False), ("full", True)):
                same[route] = agree(qs, want, cross(full_column, **outputs))
                kernels[route] = N.lib().ta_last_kernel_name().decode()
            del want
            fns = {"window": lambda: cross(False, **outputs), "full": lambda: cross(True, **outputs),
                   "window_count_only": lambda: cross(False, cap=0, count=count)}
            if old_route:
                pairs = block_pairs(0, nq, nt, upper)
                a, b = gather(qs, ts, *pairs)
                dense = torch.empty(n_pairs, dtype=torch.int32, device="cuda")
                fns["gather"] = lambda: gather(qs, ts, *pairs)
                fns["batch"] = lambda: B.levenshtein_k_batch(a, b, k, out=dense)
            ms = timed(fns, args.trials, args.window_ms)
            os.environ.pop("TA_CROSS_FULL", None)
            row = dict(row_stride_dwords=args.row_stride, row=name, nq=nq, nt=nt, length=int(qs.length), k=k, upper=upper, pairs=n_pairs, hits=n_hits,
                       window_agrees=same["window"], full_agrees=same["full"], window_kernel=kernels["window"], full_kernel=kernels["full"],
                       trials=args.trials, window_ms=args.window_ms,
                       window_route_ms=ms["window"][0], window_route_ms_range=ms["window"][1:],
                       full_route_ms=ms["full"][0], full_route_ms_range=ms["full"][1:], full_over_window=ms["full"][0] / ms["window"][0],
                       window_count_only_ms=ms["window_count_only"][0], cross_result_bytes=16 * n_hits + 12 * nq + 8,
                       pair_blob_bytes=n_pairs * int(qs.length + ts.length))
            if old_route:
                batch_kernel = N.lib().ta_last_kernel_name().decode()
                row.update(gather_ms=ms["gather"][0], gather_ms_range=ms["gather"][1:], batch_ms=ms["batch"][0], batch_ms_range=ms["batch"][1:],
                           batch_over_window=ms["batch"][0] / ms["window"][0],
                           gather_plus_batch_over_window=(ms["gather"][0] + ms["batch"][0]) / ms["window"][0], batch_kernel=batch_kernel)
                del a, b, dense, pairs
            else:
                row.update(old_route="not timed: its two pair blobs would be %.1f GB" % (n_pairs * int(qs.length + ts.length) / 1e9))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
