"""hamming_search_cross on one GPU on 3.15's workload: 1,048,576 haystacks of 100-250 bytes over ACGT and a panel of 96
random 24-byte needles (strided), one needle of the panel planted with 0-2 substitutions in every haystack; k = 2, every output asked
for.  For panels of 96, 24 and 12 needles: the single pass against (a) the route it replaces -- one shared-needle hamming_search_batch
call per needle, Best, cap = 1 -- and (b) levenshtein_search_cross on the same batch at k = 2, all three timed with device events over
`--reps` calls after a warm-up, in the same session.  Before anything is timed a sample of haystacks is checked against the oracle
hamming_search_simd_with_opts over every needle: records, nearest, best and per-haystack counts.  One JSON line per row; run it twice
and keep both runs."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import triple_accel_amd as T  # noqa: E402
from triple_accel_amd import batch as B  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
NL = 24
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


def reads(n, panel, seed):
    """-> (blob with read slack, offsets, lengths): every haystack holds one needle of `panel` ((nn, 24) uint8) with 0-2 substitutions"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(100, 251, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    blob = np.zeros(int(off[-1]) + 16, np.uint8)
    blob[: off[-1]] = ACGT[rng.integers(0, 4, int(off[-1]))]
    which = rng.integers(0, panel.shape[0], n)
    pos = off[:-1] + (rng.random(n) * (lens - NL + 1)).astype(np.int64)
    blob[pos[:, None] + np.arange(NL)[None, :]] = panel[which]
    for _ in range(2):
        hit = rng.random(n) < 0.5
        blob[pos[hit] + rng.integers(0, NL, int(hit.sum()))] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    return blob, off, lens


def verify(out, needles, blob, off, sample, k):
    hits, count, nearest, best, per = out
    torch.cuda.synchronize()
    cols = B.search_cross_to_arrays(hits, count)
    got = {}
    for i, p, s, e, d, m in zip(*cols):
        got.setdefault(int(i), []).append((int(p), int(s), int(e), int(d), int(m)))
    near, rows, cnt = nearest.cpu().numpy().view(np.uint64), best.cpu().numpy(), per.cpu().numpy()
    for i in sample:
        h = blob[off[i]:off[i + 1]].tobytes()
        want = []
        for p, nd in enumerate(needles):
            r = O.hamming_search_simd_with_opts(nd, h, k, O.BEST)
            if r:
                want.append((p, r[0][0], r[0][1], r[0][2], len(r)))
        if got.get(int(i), []) != want or int(cnt[i]) != len(want):
            return False
        w = min((x[3] << 32 | x[0] for x in want), default=0xFFFFFFFFFFFFFFFF)
        b = next(((x[1], x[2], x[3]) for x in want if x[0] == (w & 0xFFFFFFFF)), (0, 0, 0xFFFFFFFF))
        if int(near[i]) != w or (int(rows[i, 0]), int(rows[i, 1]), int(rows[i, 2]) & 0xFFFFFFFF) != b:
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--haystacks", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sample", type=int, default=300)
    ap.add_argument("--panels", type=int, nargs="*", default=[96, 24, 12])
    ap.add_argument("--only-cross", action="store_true", help="time the single pass alone (a kernel trace of its own)")
    args = ap.parse_args()
    n, k = args.haystacks, 2
    panel = ACGT[np.random.default_rng(7).integers(0, 4, (max(args.panels), NL))]
    blob, off, lens = reads(n, panel, 1)
    hs = B.Strings(torch.from_numpy(blob).cuda(), torch.from_numpy(off).cuda(), max_len=int(lens.max()))
    sample = np.linspace(0, n - 1, args.sample).astype(np.int64)
    base = {"haystacks": n, "bytes": int(off[-1]), "needle": NL, "k": k}
    for nn in args.panels:
        needles = [panel[p].tobytes() for p in range(nn)]
        nd = B.Strings.from_fixed(panel[:nn].copy())
        cap = 2 * n
        bufs = dict(hits=torch.empty((cap, 6), dtype=torch.int32, device="cuda"), count=torch.empty(1, dtype=torch.int64, device="cuda"),
                    nearest=torch.empty(n, dtype=torch.int64, device="cuda"), best=torch.empty((n, 3), dtype=torch.int64, device="cuda"),
                    per_haystack=torch.empty(n, dtype=torch.int32, device="cuda"))
        cross = lambda: B.hamming_search_cross(nd, hs, k, cap=cap, **bufs)                               # noqa: E731
        out = cross()
        ok = verify(out, needles, blob, off, sample, k)
        kern = T.last_kernel_name()
        n_hits = int(out[1].item())
        ms_cross = timed(cross, args.reps)
        row = dict(base, row="panel_%d" % nn, needles=nn, ms_cross=ms_cross, hits=n_hits, verified=ok, kernel=kern)
        if not args.only_cross:
            sides = [B.Strings.shared(nd_, n) for nd_ in needles]
            m = torch.empty((n, 1, 3), dtype=torch.int64, device="cuda")
            c = torch.empty(n, dtype=torch.int32, device="cuda")

            def loop():
                for s in sides:
                    B.hamming_search_batch(s, hs, k, T.SearchType.Best, cap=1, matches=m, counts=c)

            ms_loop = timed(loop, args.reps)
            loop_kernel = T.last_kernel_name()
            lev = lambda: B.levenshtein_search_cross(nd, hs, k, COSTS, cap=cap, **bufs)                  # noqa: E731
            ms_lev = timed(lev, args.reps)
            row.update(ms_loop=ms_loop, loop_over_cross=ms_loop / ms_cross, loop_kernel=loop_kernel,
                       ms_lev_cross=ms_lev, lev_over_cross=ms_lev / ms_cross, lev_kernel=T.last_kernel_name())
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
