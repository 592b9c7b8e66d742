"""Every token query against every target on one GPU: ta_levenshtein_cross_tokens against the route a caller had before
it -- gather the nq x nt pairs of int32 sequences into two blobs in HBM (timed on its own), then ta_levenshtein_k_batch_tokens over the
blobs (timed on its own), then filter the dense answer -- and, where the tokens are byte-valued, against ta_levenshtein_cross_with_opts
on the same data as bytes: that ratio is the price of the hash table against the 256-row table.
Workloads: 4,096 x 4,096 sequences of 16 byte-valued tokens (four values, 1 % of the queries a mutation of a target; strided);
2,048 x 2,048 sequences of 33..64 tokens over a vocabulary of 32K, half of the queries a target after a few edits (CSR).  Each at
k = 1, k = 2 and the k at which about a third of the pairs hit (from the oracle on a sample of pairs).  Every row first checks the
cross result against the dense one, pair for pair, and a sample of pairs against the oracle.  Timing: five windows of `reps` calls per
route, the routes taking turns window by window; the median window and the spread (max - min) / median are reported.  One JSON line per row."""
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
import tokens_ref as R  # noqa: E402
from triple_accel_amd import batch as B  # noqa: E402
from triple_accel_amd import _native as N  # noqa: E402

COSTS = (1, 1, 0, None)
WINDOWS = 5


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed_in_turns(routes, reps):
    """routes: {name: fn} -> {name: (median ms, spread)}; one warm-up call each, then WINDOWS rounds in which every route gets a window"""
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in routes}
    for _ in range(WINDOWS):
        for name, fn in routes.items():
            ms[name].append(window(fn, reps))
    return {name: (float(np.median(v)), float((max(v) - min(v)) / np.median(v))) for name, v in ms.items()}


def barcodes(nq, nt, seed):
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, (nt, 16)).astype(np.int64) + 65
    q = rng.integers(0, 4, (nq, 16)).astype(np.int64) + 65
    for i in rng.choice(nq, max(nq // 100, 1), replace=False):     # 1 % of the queries: a target with one or two substitutions
        q[i] = t[rng.integers(nt)]
        for _ in range(int(rng.integers(1, 3))):
            q[i, rng.integers(16)] = 65 + rng.integers(4)
    return [tuple(x.tolist()) for x in q], [tuple(x.tolist()) for x in t]


def phrases(nq, nt, seed):
    rng = np.random.default_rng(seed)
    voc = rng.choice(1 << 32, 32768, replace=False)
    t = [tuple(int(x) for x in voc[rng.integers(0, 32768, int(rng.integers(33, 65)))]) for _ in range(nt)]
    q = []
    for i in range(nq):
        if i % 2:
            q.append(tuple(int(x) for x in voc[rng.integers(0, 32768, int(rng.integers(33, 65)))]))
            continue
        s = list(t[int(rng.integers(nt))])                         # a target after 0 .. 8 substitutions / deletions
        for _ in range(int(rng.integers(0, 9))):
            p = int(rng.integers(len(s)))
            if rng.integers(2) and len(s) > 33:
                del s[p]
            else:
                s[p] = int(voc[rng.integers(32768)])
        q.append(tuple(s))
    return q, t


def gather(qs, ts):
    """the nq x nt pairs materialised in HBM, pair p = (p // nt, p % nt): -> (a side, b side) for ta_levenshtein_k_batch_tokens"""
    nq, nt = qs.n, ts.n
    if qs.off is None:
        ql, tl = qs.length, ts.length
        a = qs.values.view(nq, 1, ql).expand(nq, nt, ql).contiguous().view(-1)
        b = ts.values.view(1, nt, tl).expand(nq, nt, tl).contiguous().view(-1)
        return B.Tokens(a, None, length=ql, n=nq * nt), B.Tokens(b, None, length=tl, n=nq * nt)

    def side(s, idx):
        lens = (s.off[1:] - s.off[:-1])[idx]
        off = torch.zeros(idx.numel() + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(lens, 0, out=off[1:])
        total = int(off[-1].item())
        pair = torch.repeat_interleave(torch.arange(idx.numel(), device="cuda"), lens, output_size=total)
        src = s.off[:-1][idx][pair] + (torch.arange(total, device="cuda") - off[:-1][pair])
        return B.Tokens(s.values[src], off, max_len=s.max_len)

    p = torch.arange(nq * nt, device="cuda")
    return side(qs, p // nt), side(ts, p % nt)


def oracle_pairs(queries, targets, qi, ti, k):
    coded = [R.codes(queries[i], targets[j]) for i, j in zip(qi, ti)]
    return O.levenshtein_k_batch(O.csr_from_list([c[0] for c in coded]), O.csr_from_list([c[1] for c in coded]), k, COSTS)


def third_k(queries, targets, seed, sample=5000):
    """the k at which the share of hitting pairs is closest to a third, from the oracle on a sample of pairs"""
    rng = np.random.default_rng(seed)
    qi, ti = rng.integers(len(queries), size=sample), rng.integers(len(targets), size=sample)
    d = oracle_pairs(queries, targets, qi, ti, 128)
    return min((abs(float((d <= k).mean()) - 1 / 3), k) for k in range(0, 70))[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="scales both sides of both workloads (a quick run: 0.25)")
    args = ap.parse_args()
    for name, make, n, fixed in (("tokens_16_bytes", barcodes, int(4096 * args.scale), True), ("tokens_33_64_vocab32k", phrases, int(2048 * args.scale), False)):
        queries, targets = make(n, n, 11)
        if fixed:
            qs, ts = B.Tokens.from_fixed(np.array(queries, dtype=np.int64)), B.Tokens.from_fixed(np.array(targets, dtype=np.int64))
            qb = B.Strings.from_fixed(np.array(queries, dtype=np.uint8))
            tb = B.Strings.from_fixed(np.array(targets, dtype=np.uint8))
        else:
            qs, ts = B.Tokens.from_list(queries), B.Tokens.from_list(targets)
        a, b = gather(qs, ts)
        pair_bytes = 4 * int(a.values.numel() + b.values.numel()) + (0 if fixed else 16 * (n * n + 1))
        dense = torch.empty(n * n, dtype=torch.int32, device="cuda")
        count = torch.empty(1, dtype=torch.int64, device="cuda")
        nearest = torch.empty(n, dtype=torch.int64, device="cuda")
        rng = np.random.default_rng(12)
        for k in (1, 2, third_k(queries, targets, 13)):
            B.levenshtein_k_batch_tokens(a, b, k, COSTS, out=dense)
            batch_kernel = N.lib().ta_last_kernel_name().decode()
            B.levenshtein_cross_tokens(qs, ts, k, COSTS, cap=0, count=count)
            torch.cuda.synchronize()
            n_hits = int(count.item())
            hits = torch.empty((max(n_hits, 1), 4), dtype=torch.int32, device="cuda")
            B.levenshtein_cross_tokens(qs, ts, k, COSTS, cap=n_hits, hits=hits, count=count, nearest=nearest)
            cross_kernel = N.lib().ta_last_kernel_name().decode()
            torch.cuda.synchronize()
            # the routes agree pair for pair, and a sample of pairs agrees with the oracle
            want = torch.nonzero(dense.view(n, n) >= 0)
            order = torch.argsort(hits[:n_hits, 0].long() * n + hits[:n_hits, 1].long())
            got = hits[:n_hits][order]
            same = n_hits == want.shape[0] and bool((got[:, :2].long() == want).all()) and \
                bool((got[:, 2] == dense.view(n, n)[want[:, 0], want[:, 1]]).all())
            qi, ti = rng.integers(n, size=2000), rng.integers(n, size=2000)
            oracle_ok = bool((dense.view(n, n).cpu().numpy().view(np.uint32)[qi, ti] == oracle_pairs(queries, targets, qi, ti, k)).all())
            routes = {"cross_tokens": lambda: B.levenshtein_cross_tokens(qs, ts, k, COSTS, cap=n_hits, hits=hits, count=count, nearest=nearest),
                      "gather": lambda: gather(qs, ts),
                      "batch_tokens": lambda: B.levenshtein_k_batch_tokens(a, b, k, COSTS, out=dense)}
            bytes_agree = None
            if fixed:
                bhits = torch.empty((max(n_hits, 1), 4), dtype=torch.int32, device="cuda")
                bcount = torch.empty(1, dtype=torch.int64, device="cuda")
                B.levenshtein_cross_with_opts(qb, tb, k, COSTS, cap=n_hits, hits=bhits, count=bcount, nearest=nearest)
                torch.cuda.synchronize()
                border = torch.argsort(bhits[:n_hits, 0].long() * n + bhits[:n_hits, 1].long())
                bytes_agree = int(bcount.item()) == n_hits and bool((bhits[:n_hits][border][:, :3] == got[:, :3]).all())
                routes["cross_bytes"] = lambda: B.levenshtein_cross_with_opts(qb, tb, k, COSTS, cap=n_hits, hits=bhits, count=bcount, nearest=nearest)
            t = timed_in_turns(routes, args.reps)
            row = dict(row=name, nq=n, nt=n, k=k, hits=n_hits, hit_share=n_hits / (n * n), routes_agree=same, oracle_sample_ok=oracle_ok,
                       bytes_route_agrees=bytes_agree, cross_kernel=cross_kernel, batch_kernel=batch_kernel, pair_blob_bytes=pair_bytes,
                       cross_result_bytes=16 * n_hits + 8 * n + 8, windows=WINDOWS, reps=args.reps)
            for route, (ms, spread) in t.items():
                row[route + "_ms"], row[route + "_spread"] = ms, spread
            row["gather_plus_batch_over_cross"] = (t["gather"][0] + t["batch_tokens"][0]) / t["cross_tokens"][0]
            row["batch_over_cross"] = t["batch_tokens"][0] / t["cross_tokens"][0]
            if fixed:
                row["cross_tokens_over_cross_bytes"] = t["cross_tokens"][0] / t["cross_bytes"][0]
            print(json.dumps(row), flush=True)
        del a, b, dense


if __name__ == "__main__":
    main()
