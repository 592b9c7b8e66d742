"""Token batches on one GPU: 1M pairs x 32-64 int32 tokens, vocabulary 32K, unit costs -- the compaction kernel alone,
the whole levenshtein_k_batch_tokens call at k = 8 and unbounded, the byte pass on the compacted strings, the compaction's bytes moved as a
fraction of 8 TB/s; then the overflow route (1,000 pairs of 400 distinct tokens).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from triple_accel_amd import batch as B  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    n = args.pairs
    g = torch.Generator(device="cuda").manual_seed(1)
    la = torch.randint(32, 65, (n,), device="cuda", generator=g)
    lb = torch.randint(32, 65, (n,), device="cuda", generator=g)
    offa = torch.zeros(n + 1, dtype=torch.int64, device="cuda"); offa[1:] = torch.cumsum(la, 0)
    offb = torch.zeros(n + 1, dtype=torch.int64, device="cuda"); offb[1:] = torch.cumsum(lb, 0)
    va = torch.randint(0, 32768, (int(offa[-1]),), dtype=torch.int32, device="cuda", generator=g)
    vb = torch.randint(0, 32768, (int(offb[-1]),), dtype=torch.int32, device="cuda", generator=g)
    # b = a with a few substitutions where the lengths allow: near pairs, the usual error-rate workload
    m = torch.minimum(la, lb)
    idx = torch.arange(int(offb[-1]), device="cuda")
    pair_b = torch.repeat_interleave(torch.arange(n, device="cuda"), lb)
    pos = idx - offb[pair_b]
    keep = (pos < m[pair_b]) & (torch.rand(idx.shape, device="cuda", generator=g) > 0.1)
    vb[keep] = va[offa[pair_b[keep]] + pos[keep]]
    ta, tb = B.Tokens.from_csr(va, offa, max_len=64), B.Tokens.from_csr(vb, offb, max_len=64)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    res = {"pairs": n, "tokens": int(offa[-1] + offb[-1])}
    res["k8_ms"] = timed(lambda: B.levenshtein_k_batch_tokens(ta, tb, 8, out=out), args.reps)
    res["unbounded_ms"] = timed(lambda: B.levenshtein_k_batch_tokens(ta, tb, 0xFFFFFFFF, out=out), args.reps)
    # the byte pass alone on a byte batch of the same shape (the tokens folded into bytes); the compaction is the call minus it
    from triple_accel_amd import _native as N
    sa = B.Strings(torch.zeros(int(offa[-1]) + 16, dtype=torch.uint8, device="cuda"), offa, max_len=64)
    sb = B.Strings(torch.zeros(int(offb[-1]) + 16, dtype=torch.uint8, device="cuda"), offb, max_len=64)
    ca = torch.remainder(va, 251).to(torch.uint8); cb = torch.remainder(vb, 251).to(torch.uint8)
    sa.blob[: ca.numel()] = ca; sb.blob[: cb.numel()] = cb
    res["byte_pass_k8_ms"] = timed(lambda: B.levenshtein_k_batch(sa, sb, 8, out=out), args.reps)
    res["byte_pass_unbounded_ms"] = timed(lambda: B.levenshtein_k_batch(sa, sb, 0xFFFFFFFF, out=out), args.reps)
    res["compaction_ms_est"] = res["k8_ms"] - res["byte_pass_k8_ms"]
    moved = res["tokens"] * 5
    res["compaction_bytes"] = moved
    res["compaction_frac_8TBs"] = moved / (res["compaction_ms_est"] * 1e-3) / 8e12 if res["compaction_ms_est"] > 0 else None
    res["kernel"] = N.lib().ta_last_kernel_name().decode()
    # overflow route: 1,000 pairs of 400 distinct tokens (permutations with a few swaps)
    rng = np.random.default_rng(2)
    xs = np.stack([rng.permutation(1 << 20)[:400] for _ in range(1000)])
    ys = xs.copy()
    for r in range(1000):
        p = rng.integers(0, 400, 8)
        ys[r, p] = ys[r, p[::-1]]
    ox, oy = B.Tokens.from_fixed(torch.from_numpy(xs)), B.Tokens.from_fixed(torch.from_numpy(ys))
    o2 = torch.empty(1000, dtype=torch.int32, device="cuda")
    res["overflow_1000x400_k8_ms"] = timed(lambda: B.levenshtein_k_batch_tokens(ox, oy, 8, out=o2), 3)
    res["overflow_1000x400_unbounded_ms"] = timed(lambda: B.levenshtein_k_batch_tokens(ox, oy, 0xFFFFFFFF, out=o2), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
