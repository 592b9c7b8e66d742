"""levenshtein_search over a batch of reads on one GPU: 1,048,576 haystacks of 100-250 bytes over ACGT, a shared 24-byte
needle planted with 0-2 substitutions in half of them.  Rows: Best at k = 3 (unit costs), All, EditCosts(2, 3, 1, None) at k = 6, the exact
route alone (TA_SEARCH_BATCH_NO_SCAN=1), per-pair CSR needles of 16-32 bytes, and the single-call host path over the first 1,000 pairs.
Every row checks a sample of pairs against the scalar oracle before it is timed.  One JSON line per row."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("TA_TUNING", "1")        # (the A/B switch of the exact-route row is honoured only under TA_TUNING)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import triple_accel_amd as T  # noqa: E402
from triple_accel_amd import batch as B  # noqa: E402
from triple_accel_amd import _native as N  # noqa: E402


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


def reads(n, seed):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    lens = rng.integers(100, 251, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    blob = np.zeros(int(off[-1]) + 16, np.uint8)
    blob[: off[-1]] = acgt[rng.integers(0, 4, int(off[-1]))]
    needle = acgt[rng.integers(0, 4, 24)]
    planted = np.arange(1, n, 2)
    pos = off[planted] + (rng.random(planted.size) * (lens[planted] - 24 + 1)).astype(np.int64)
    idx = pos[:, None] + np.arange(24)[None, :]
    blob[idx] = needle[None, :]
    for _ in range(2):                                          # 0-2 substitutions per planted copy
        hit = rng.random(planted.size) < 0.5
        blob[pos[hit] + rng.integers(0, 24, int(hit.sum()))] = acgt[rng.integers(0, 4, int(hit.sum()))]
    return needle.tobytes(), blob, off, lens


def hay_list(blob, off, idx):
    return [blob[off[i]:off[i + 1]].tobytes() for i in idx]


def verify(m, c, needles, hays, idx, k, st, costs):
    got = B.matches_to_lists(m[idx], c[idx])
    want = [O.levenshtein_search_naive_with_opts(nd, h, k, st, costs, False) for nd, h in zip(needles, hays)]
    return [[tuple(x) for x in r] for r in got] == want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sample", type=int, default=300)
    args = ap.parse_args()
    n = args.pairs
    needle, blob, off, lens = reads(n, 1)
    hs = B.Strings(torch.from_numpy(blob).cuda(), torch.from_numpy(off).cuda(), max_len=int(lens.max()))
    side = B.Strings.shared(needle, n)
    sample = np.linspace(0, n - 1, args.sample).astype(np.int64)
    shays = hay_list(blob, off, sample)
    base = {"pairs": n, "bytes": int(off[-1]), "needle": len(needle)}
    rows = [("reads_best_k3", 3, O.BEST, (1, 1, 0, None), False),
            ("reads_all_k3", 3, O.ALL, (1, 1, 0, None), False),
            ("reads_best_weighted_2_3_1_k6", 6, O.BEST, (2, 3, 1, None), False),
            ("reads_best_k3_exact_route", 3, O.BEST, (1, 1, 0, None), True)]
    for name, k, st, costs, no_scan in rows:
        if no_scan:
            os.environ["TA_SEARCH_BATCH_NO_SCAN"] = "1"
        cap = 8 if st == O.BEST else 32
        m = torch.empty((n, cap, 3), dtype=torch.int64, device="cuda")
        c = torch.empty(n, dtype=torch.int32, device="cuda")
        B.levenshtein_search_batch(side, hs, k, st, costs, cap=cap, matches=m, counts=c)
        torch.cuda.synchronize()
        ok = verify(m, c, [needle] * len(sample), shays, sample, k, st, costs)
        kern = N.lib().ta_last_kernel_name().decode()
        ms = timed(lambda: B.levenshtein_search_batch(side, hs, k, st, costs, cap=cap, matches=m, counts=c), args.reps)
        os.environ.pop("TA_SEARCH_BATCH_NO_SCAN", None)
        print(json.dumps(dict(base, row=name, k=k, costs=list(costs), ms=ms, verified=ok, kernel=kern,
                              with_hits=int((c > 0).sum().item()))), flush=True)
    # per-pair CSR needles of 16-32 bytes (the exact route)
    rng = np.random.default_rng(2)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    nl = rng.integers(16, 33, n)
    noff = np.zeros(n + 1, np.int64)
    np.cumsum(nl, out=noff[1:])
    nblob = np.zeros(int(noff[-1]) + 16, np.uint8)
    nblob[: noff[-1]] = acgt[rng.integers(0, 4, int(noff[-1]))]
    nside = B.Strings(torch.from_numpy(nblob).cuda(), torch.from_numpy(noff).cuda(), max_len=32)
    m = torch.empty((n, 8, 3), dtype=torch.int64, device="cuda")
    c = torch.empty(n, dtype=torch.int32, device="cuda")
    B.levenshtein_search_batch(nside, hs, 3, O.BEST, (1, 1, 0, None), cap=8, matches=m, counts=c)
    torch.cuda.synchronize()
    ok = verify(m, c, hay_list(nblob, noff, sample), shays, sample, 3, O.BEST, (1, 1, 0, None))
    kern = N.lib().ta_last_kernel_name().decode()
    ms = timed(lambda: B.levenshtein_search_batch(nside, hs, 3, O.BEST, (1, 1, 0, None), cap=8, matches=m, counts=c), args.reps)
    print(json.dumps(dict(base, row="per_pair_needles_16_32_best_k3", k=3, ms=ms, verified=ok, kernel=kern)), flush=True)
    # the single-call host path, first 1,000 pairs
    first = hay_list(blob, off, range(min(1000, n)))
    got = [list(T.levenshtein_search_simd_with_opts(needle, h, 3, T.SearchType.Best, T.LEVENSHTEIN_COSTS, False)) for h in first[:50]]
    ok = got == [[T.Match(*x) for x in O.levenshtein_search_naive_with_opts(needle, h, 3, O.BEST)] for h in first[:50]]
    t0 = time.perf_counter()
    for h in first:
        list(T.levenshtein_search_simd_with_opts(needle, h, 3, T.SearchType.Best, T.LEVENSHTEIN_COSTS, False))
    us = (time.perf_counter() - t0) * 1e6 / len(first)
    print(json.dumps(dict(base, row="single_call_host_path", k=3, us_per_pair=us, pairs_timed=len(first), verified=ok,
                          est_ms_for_batch=us * n / 1e3)), flush=True)


if __name__ == "__main__":
    main()
