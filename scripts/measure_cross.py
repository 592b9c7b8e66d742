"""Every query against every target on one GPU: ta_levenshtein_cross against the route a caller had before it -- gather
the nq x nt pairs into two blobs in HBM (timed on its own), then ta_levenshtein_k_batch over the blobs (timed on its own), then filter
the dense answer.  Workloads: 4,096 x 4,096 random 16-byte ACGT barcodes, 1 % of the queries a mutation of a target (strided blobs);
2,048 x 2,048 words of 4..24 lower-case letters (CSR blobs).  Each at k = 1, k = 2 and the k at which about a third of the pairs hit
(found from the oracle on a sample of pairs).  Every row first checks the cross result against the dense one, pair for pair, and a
sample of pairs against the oracle.  One JSON line per row."""
import argparse
import json
import os
import sys

os.environ.setdefault("TA_TUNING", "1")        # (TA_CROSS_QTILE, the query tile's override, is honoured only under TA_TUNING)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
from triple_accel_amd import batch as B  # noqa: E402
from triple_accel_amd import _native as N  # noqa: E402

COSTS = (1, 1, 0, None)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def barcodes(nq, nt, seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    t = acgt[rng.integers(0, 4, (nt, 16))]
    q = acgt[rng.integers(0, 4, (nq, 16))]
    for i in rng.choice(nq, nq // 100, replace=False):            # 1 % of the queries: a target with one or two substitutions
        q[i] = t[rng.integers(nt)]
        for _ in range(int(rng.integers(1, 3))):
            q[i, rng.integers(16)] = acgt[rng.integers(4)]
    return [x.tobytes() for x in q], [x.tobytes() for x in t]


def words(nq, nt, seed):
    rng = np.random.default_rng(seed)
    mk = lambda n: [bytes(rng.integers(97, 123, int(rng.integers(4, 25)), dtype=np.uint8)) for _ in range(n)]   # noqa: E731
    return mk(nq), mk(nt)


def gather(qs, ts, fixed):
    """the nq x nt pairs materialised in HBM, pair p = (p // nt, p % nt): -> (a side, b side) for ta_levenshtein_k_batch"""
    nq, nt = qs.n, ts.n
    if fixed:
        ql, tl = qs.length, ts.length
        a = torch.zeros(nq * nt * ql + 16, dtype=torch.uint8, device="cuda")
        b = torch.zeros(nq * nt * tl + 16, dtype=torch.uint8, device="cuda")
        a[: nq * nt * ql].view(nq, nt, ql).copy_(qs.blob[: nq * ql].view(nq, 1, ql).expand(nq, nt, ql))
        b[: nq * nt * tl].view(nq, nt, tl).copy_(ts.blob[: nt * tl].view(1, nt, tl).expand(nq, nt, tl))
        return B.Strings(a, None, stride=ql, length=ql, n=nq * nt), B.Strings(b, None, stride=tl, length=tl, n=nq * nt)

    def side(s, idx):
        lens = (s.off[1:] - s.off[:-1])[idx]
        off = torch.zeros(idx.numel() + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(lens, 0, out=off[1:])
        total = int(off[-1].item())
        pair = torch.repeat_interleave(torch.arange(idx.numel(), device="cuda"), lens, output_size=total)
        src = s.off[:-1][idx][pair] + (torch.arange(total, device="cuda") - off[:-1][pair])
        blob = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
        blob[:total] = s.blob[src]
        return B.Strings(blob, off, max_len=s.max_len)

    p = torch.arange(nq * nt, device="cuda")
    return side(qs, p // nt), side(ts, p % nt)


def third_k(queries, targets, seed, sample=20000):
    """the k at which the share of hitting pairs is closest to a third, from the oracle on a sample of pairs"""
    rng = np.random.default_rng(seed)
    qi, ti = rng.integers(len(queries), size=sample), rng.integers(len(targets), size=sample)
    d = O.levenshtein_k_batch(O.csr_from_list([queries[i] for i in qi]), O.csr_from_list([targets[i] for i in ti]), 64, COSTS)
    shares = [(abs(float((d <= k).mean()) - 1 / 3), k) for k in range(0, 40)]
    return min(shares)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0, help="scales both sides of both workloads (a quick run: 0.25)")
    args = ap.parse_args()
    for name, make, n, fixed in (("barcodes_16", barcodes, int(4096 * args.scale), True), ("words_4_24", words, int(2048 * args.scale), False)):
        queries, targets = make(n, n, 11)
        if fixed:
            arr = lambda s: np.frombuffer(b"".join(s), np.uint8).reshape(len(s), -1)   # noqa: E731
            qs, ts = B.Strings.from_fixed(arr(queries)), B.Strings.from_fixed(arr(targets))
        else:
            qs, ts = B.Strings.from_list(queries), B.Strings.from_list(targets)
        gather_ms = timed(lambda: gather(qs, ts, fixed), max(2, args.reps // 3))
        a, b = gather(qs, ts, fixed)
        pair_bytes = int(a.blob.numel() + b.blob.numel() + (0 if fixed else 16 * (n * n + 1)))
        dense = torch.empty(n * n, dtype=torch.int32, device="cuda")
        count = torch.empty(1, dtype=torch.int64, device="cuda")
        nearest = torch.empty(n, dtype=torch.int64, device="cuda")
        rng = np.random.default_rng(12)
        for k in (1, 2, third_k(queries, targets, 13)):
            B.levenshtein_k_batch(a, b, k, COSTS, out=dense)
            batch_kernel = N.lib().ta_last_kernel_name().decode()
            B.levenshtein_cross(qs, ts, k, COSTS, cap=0, count=count)
            torch.cuda.synchronize()
            n_hits = int(count.item())
            hits = torch.empty((max(n_hits, 1), 4), dtype=torch.int32, device="cuda")
            B.levenshtein_cross(qs, ts, k, COSTS, cap=n_hits, hits=hits, count=count, nearest=nearest)
            cross_kernel = N.lib().ta_last_kernel_name().decode()
            torch.cuda.synchronize()
            # the two routes agree pair for pair, and a sample of pairs agrees with the oracle
            want = torch.nonzero(dense.view(n, n) >= 0)
            order = torch.argsort(hits[:n_hits, 0].long() * n + hits[:n_hits, 1].long())
            got = hits[:n_hits][order]
            same = n_hits == want.shape[0] and bool((got[:, :2].long() == want).all()) and \
                bool((got[:, 2] == dense.view(n, n)[want[:, 0], want[:, 1]]).all())
            qi, ti = rng.integers(n, size=2000), rng.integers(n, size=2000)
            od = O.levenshtein_k_batch(O.csr_from_list([queries[i] for i in qi]), O.csr_from_list([targets[i] for i in ti]), k, COSTS)
            oracle_ok = bool((dense.view(n, n).cpu().numpy().view(np.uint32)[qi, ti] == od).all())
            batch_ms = timed(lambda: B.levenshtein_k_batch(a, b, k, COSTS, out=dense), args.reps)
            cross_ms = timed(lambda: B.levenshtein_cross(qs, ts, k, COSTS, cap=n_hits, hits=hits, count=count, nearest=nearest), args.reps)
            count_ms = timed(lambda: B.levenshtein_cross(qs, ts, k, COSTS, cap=0, count=count), args.reps)
            print(json.dumps(dict(row=name, nq=n, nt=n, k=k, hits=n_hits, hit_share=n_hits / (n * n), gather_ms=gather_ms, batch_ms=batch_ms,
                                  cross_ms=cross_ms, cross_count_only_ms=count_ms, batch_over_cross=batch_ms / cross_ms,
                                  gather_plus_batch_over_cross=(gather_ms + batch_ms) / cross_ms, pair_blob_bytes=pair_bytes,
                                  cross_result_bytes=16 * n_hits + 8 * n + 8, routes_agree=same, oracle_sample_ok=oracle_ok,
                                  cross_kernel=cross_kernel, batch_kernel=batch_kernel)), flush=True)
        del a, b, dense


if __name__ == "__main__":
    main()
