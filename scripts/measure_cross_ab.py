"""A/B of ta_levenshtein_cross between two builds: times the entry of the package found under --root (a checkout with
its library built) on 4,096 x 4,096 16-byte ACGT barcodes (lev_cross_kernel<1, TRANS>) and 2,048 x 2,048 ACGT strings of 33 - 64 bytes
(lev_cross_kernel<2, TRANS>), 1 % of the queries a target with one or two substitutions, at k = 1 and 2, both cost families, counting
and with records.  Run it once per build, alternating, on the same box; every run prints one JSON line per row with --label in it:
the median of --trials windows of at least --window-ms, and the fastest and slowest window."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ACGT = np.frombuffer(b"ACGT", np.uint8)


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn, trials, window_ms):
    fn()
    torch.cuda.synchronize()
    reps = max(3, int(window_ms / max(window(fn, 3), 1e-3)) + 1)
    v = [window(fn, reps) for _ in range(trials)]
    return float(np.median(v)), float(min(v)), float(max(v))


def batch(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    t = [ACGT[rng.integers(0, 4, int(rng.integers(lo, hi + 1)))] for _ in range(n)]
    q = [ACGT[rng.integers(0, 4, int(rng.integers(lo, hi + 1)))] for _ in range(n)]
    for i in rng.choice(n, n // 100, replace=False):
        q[i] = t[rng.integers(n)].copy()
        for _ in range(int(rng.integers(1, 3))):
            q[i][rng.integers(len(q[i]))] = ACGT[rng.integers(4)]
    return [x.tobytes() for x in q], [x.tobytes() for x in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    from triple_accel_amd import batch as B
    from triple_accel_amd import _native as N
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no other route"
    for name, n, lo, hi in (("barcodes_16", 4096, 16, 16), ("strings_33_64", 2048, 33, 64)):
        queries, targets = batch(n, lo, hi, 31)
        qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
        count = torch.empty(1, dtype=torch.int64, device="cuda")
        nearest = torch.empty(n, dtype=torch.int64, device="cuda")
        for costs in ((1, 1, 0, None), (1, 1, 0, 1)):
            for k in (1, 2):
                B.levenshtein_cross(qs, ts, k, costs, cap=0, count=count)
                torch.cuda.synchronize()
                n_hits = int(count.item())
                hits = torch.empty((max(n_hits, 1), 4), dtype=torch.int32, device="cuda")
                full = timed(lambda: B.levenshtein_cross(qs, ts, k, costs, cap=n_hits, hits=hits, count=count, nearest=nearest), args.trials, args.window_ms)
                kernel = N.lib().ta_last_kernel_name().decode()
                print(json.dumps(dict(label=args.label, row=name, n=n, k=k, kernel=kernel, hits=n_hits, cross_ms=full[0], cross_ms_range=full[1:],
                                      trials=args.trials, window_ms=args.window_ms)), flush=True)


if __name__ == "__main__":
    main()
