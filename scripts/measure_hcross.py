"""Every query against every target within k mismatches on one GPU: ta_hamming_cross against the route a caller had
before it -- gather the pairs into two blobs in HBM (timed on its own), then ta_hamming_batch over the blobs (timed on its own), then
filter the dense answer.  Workloads, each at k = 1 and k = 2:
  tags_16       4,096 x 4,096 random 16-byte ACGT tags, 1 % of the queries a target with one or two substitutions (strided blobs);
  tags_16_64k   65,536 x 4,096 of the same: the entry only -- the old route's two blobs would hold 65,536 x 4,096 x 16 bytes each, 8 GB
                together, so it is not timed; it is still run, 4,096 queries at a time, for the pair-for-pair check;
  umis_12_upper 4,096 12-byte UMIs against themselves with TA_CROSS_UPPER; the old route gathers the 4,096 x 4,095 / 2 pairs i < j.
Every row first checks the cross result against the dense one, pair for pair (hits, distances, nearest words, per-query counts).  Times:
every route is warmed up, then timed in `--trials` windows of at least `--window-ms` each, the routes alternating inside a trial; a row
reports the median window and the fastest and slowest one.  One JSON line per row."""
import argparse
import json
import os
import sys

os.environ.setdefault("TA_TUNING", "1")        # (TA_HCROSS_QTILE, the query tile's override, is honoured only under TA_TUNING)
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
        once = max(window(fn, 3), 1e-3)
        reps[name] = max(3, int(window_ms / once) + 1)
    got = {name: [] for name in fns}
    for _ in range(trials):
        for name, fn in fns.items():
            got[name].append(window(fn, reps[name]))
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in got.items()}


def tags(nq, nt, length, seed):
    rng = np.random.default_rng(seed)
    t = ACGT[rng.integers(0, 4, (nt, length))]
    q = ACGT[rng.integers(0, 4, (nq, length))]
    for i in rng.choice(nq, nq // 100, replace=False):            # 1 % of the queries: a target with one or two substitutions
        q[i] = t[rng.integers(nt)]
        for _ in range(int(rng.integers(1, 3))):
            q[i, rng.integers(length)] = ACGT[rng.integers(4)]
    return q, t


def umis(n, length, seed):
    rng = np.random.default_rng(seed)
    base = ACGT[rng.integers(0, 4, (n // 8, length))]             # eight reads per molecule, each with zero to two substitutions
    u = base[rng.integers(0, n // 8, n)].copy()
    for i in range(n):
        for _ in range(int(rng.integers(0, 3))):
            u[i, rng.integers(length)] = ACGT[rng.integers(4)]
    return u


def gather(qs, ts, qi, ti):
    """the pairs (qi[p], ti[p]) materialised in HBM -> (a side, b side) for ta_hamming_batch"""
    n, ql, tl = qi.numel(), qs.length, ts.length
    a = torch.zeros(n * ql + 16, dtype=torch.uint8, device="cuda")
    b = torch.zeros(n * tl + 16, dtype=torch.uint8, device="cuda")
    a[: n * ql].view(n, ql).copy_(qs.blob[: qs.n * ql].view(qs.n, ql)[qi])
    b[: n * tl].view(n, tl).copy_(ts.blob[: ts.n * tl].view(ts.n, tl)[ti])
    return B.Strings(a, None, stride=ql, length=ql, n=n), B.Strings(b, None, stride=tl, length=tl, n=n)


def all_pairs(q0, q1, nt):
    p = torch.arange((q1 - q0) * nt, device="cuda")
    return q0 + p // nt, p % nt


def dense_hits(qs, ts, qi, ti, k):
    """the old route's answer: (q, t, d) rows of the pairs within k, sorted by (q, t)"""
    a, b = gather(qs, ts, qi, ti)
    d = B.hamming_batch(a, b)
    keep = torch.nonzero((d >= 0) & (d <= k)).flatten()
    rows = torch.stack([qi[keep], ti[keep], d[keep].long()], dim=1)
    return rows[torch.argsort(rows[:, 0] * ts.n + rows[:, 1])]


def agree(qs, ts, want, out):
    """the cross outputs against the dense route's sorted rows, pair for pair (on the host)"""
    hits, count, nearest, per_query = out
    torch.cuda.synchronize()
    n = int(count.item())
    want = want.cpu().numpy()
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
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--scale", type=float, default=1.0, help="scales both sides of every workload (a quick run: 0.25)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no other route"
    s = lambda n: max(64, int(n * args.scale))                                      # noqa: E731
    q16, t16 = tags(s(4096), s(4096), 16, 11)
    q64k, _ = tags(s(65536), s(4096), 16, 12)
    u12 = umis(s(4096), 12, 13)
    for name, q, t, upper, old_route in (("tags_16", q16, t16, False, True), ("tags_16_64k", q64k, t16, False, False),
                                         ("umis_12_upper", u12, u12, True, True)):
        qs, ts = B.Strings.from_fixed(q), B.Strings.from_fixed(t)
        nq, nt = qs.n, ts.n
        if upper:
            iu = torch.triu_indices(nq, nt, offset=1, device="cuda")
            pairs = lambda: (iu[0], iu[1])                                          # noqa: E731
        else:
            pairs = lambda: all_pairs(0, nq, nt)                                    # noqa: E731
        n_pairs = int(pairs()[0].numel()) if old_route else nq * nt
        count = torch.empty(1, dtype=torch.int64, device="cuda")
        nearest = torch.empty(nq, dtype=torch.int64, device="cuda")
        per_query = torch.empty(nq, dtype=torch.int32, device="cuda")
        for k in (1, 2):
            B.hamming_cross(qs, ts, k, cap=0, count=count, upper=upper)
            torch.cuda.synchronize()
            n_hits = int(count.item())
            hits = torch.empty((max(n_hits, 1), 4), dtype=torch.int32, device="cuda")
            full = lambda: B.hamming_cross(qs, ts, k, cap=n_hits, hits=hits, count=count, nearest=nearest, per_query=per_query, upper=upper)   # noqa: E731
            out = full()
            kernel = N.lib().ta_last_kernel_name().decode()
            # the two routes agree pair for pair (the old one 4,096 queries at a time where its blobs would not fit)
            if old_route:
                want = dense_hits(qs, ts, *pairs(), k)
            else:
                want = torch.cat([dense_hits(qs, ts, *all_pairs(q0, min(q0 + 4096, nq), nt), k) for q0 in range(0, nq, 4096)])
            same = agree(qs, ts, want, out)
            del want
            fns = {"cross": full, "cross_count_only": lambda: B.hamming_cross(qs, ts, k, cap=0, count=count, upper=upper)}
            if old_route:
                a, b = gather(qs, ts, *pairs())
                dense = torch.empty(n_pairs, dtype=torch.int32, device="cuda")
                fns["gather"] = lambda: gather(qs, ts, *pairs())
                fns["batch"] = lambda: B.hamming_batch(a, b, out=dense)
            ms = timed(fns, args.trials, args.window_ms)
            row = dict(row=name, nq=nq, nt=nt, length=int(qs.length), k=k, upper=upper, pairs=n_pairs, hits=n_hits, routes_agree=same,
                       cross_kernel=kernel, trials=args.trials, window_ms=args.window_ms,
                       cross_ms=ms["cross"][0], cross_ms_range=ms["cross"][1:], cross_count_only_ms=ms["cross_count_only"][0],
                       cross_count_only_ms_range=ms["cross_count_only"][1:], cross_result_bytes=16 * n_hits + 12 * nq + 8,
                       pair_blob_bytes=n_pairs * int(qs.length + ts.length))
            if old_route:
                batch_kernel = N.lib().ta_last_kernel_name().decode()
                row.update(gather_ms=ms["gather"][0], gather_ms_range=ms["gather"][1:], batch_ms=ms["batch"][0], batch_ms_range=ms["batch"][1:],
                           batch_over_cross=ms["batch"][0] / ms["cross"][0],
                           gather_plus_batch_over_cross=(ms["gather"][0] + ms["batch"][0]) / ms["cross"][0], batch_kernel=batch_kernel)
                del a, b, dense
            else:
                row.update(old_route="not timed: its two pair blobs would be %.1f GB" % (n_pairs * int(qs.length + ts.length) / 1e9))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
