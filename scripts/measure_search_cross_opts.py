"""levenshtein_search_cross_with_opts' two-word route on one GPU on 3.15's batch: 1,048,576 haystacks of 100-250 bytes
over ACGT, one needle of the panel planted with 0-2 substitutions in every haystack; k = 3, LEVENSHTEIN_COSTS, every output asked for.
Rows: panels of 12 x 34-byte and 96 x 40-byte needles (strided) -- the single pass against the route it replaces, one shared-needle
levenshtein_search_batch call per needle, Best, cap = 1 (that route has a two-word scan of its own) -- and, as a control, 96 x 24-byte
needles through the new entry and through levenshtein_search_cross: the same kernels, so any difference beyond the spread is a routing
bug.  Both routes of a row are timed with device events in alternating windows of `--reps` calls in the same session: the medians of
`--windows` windows and their spread (max - min over the median) are reported.  Before anything is timed a sample of haystacks is
checked against the scalar oracle over every needle: records, nearest, best and per-haystack counts.  One JSON line per row, appended to
`--out` when given.  `--anchored-row` adds one small anchored row (the memory-backed recurrence on every pair's prefix).
The scan / exact / finish split comes from a kernel trace taken in a run of its own (`--trace-row`: one row, few calls, no loop)."""
import argparse
import json
import os
import statistics
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
COSTS = (1, 1, 0, None)
ROWS = {"panel_12x34": (12, 34), "panel_96x40": (96, 40), "control_96x24": (96, 24)}


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternating(fa, fb, reps, windows):
    """-> (median a, spread a, median b, spread b): the two routes in turn, one warm-up call each first"""
    fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(windows):
        ta.append(window(fa, reps))
        tb.append(window(fb, reps))
    med = statistics.median
    return med(ta), (max(ta) - min(ta)) / med(ta), med(tb), (max(tb) - min(tb)) / med(tb)


def reads(n, panel, seed):
    """-> (blob with read slack, offsets, lengths): every haystack holds one needle of `panel` ((nn, nl) uint8) with 0-2 substitutions"""
    nl = panel.shape[1]
    rng = np.random.default_rng(seed)
    lens = rng.integers(100, 251, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    blob = np.zeros(int(off[-1]) + 16, np.uint8)
    blob[: off[-1]] = ACGT[rng.integers(0, 4, int(off[-1]))]
    which = rng.integers(0, panel.shape[0], n)
    pos = off[:-1] + (rng.random(n) * (lens - nl + 1)).astype(np.int64)
    blob[pos[:, None] + np.arange(nl)[None, :]] = panel[which]
    for _ in range(2):
        hit = rng.random(n) < 0.5
        blob[pos[hit] + rng.integers(0, nl, int(hit.sum()))] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    return blob, off, lens


def verify(out, needles, blob, off, sample, k, anchored=False):
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
            r = O.levenshtein_search_naive_with_opts(nd, h, k, O.BEST, COSTS, anchored)
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--sample", type=int, default=300)
    ap.add_argument("--rows", nargs="*", default=list(ROWS))
    ap.add_argument("--anchored-row", action="store_true")
    ap.add_argument("--trace-row", default=None, help="one row, three calls of the single pass, nothing else: for a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n, k = args.haystacks, 3
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for row in ([args.trace_row] if args.trace_row else args.rows):
        nn, nl = ROWS[row]
        panel = ACGT[np.random.default_rng(7 + nl).integers(0, 4, (nn, nl))]
        blob, off, lens = reads(n, panel, 1)
        hs = B.Strings(torch.from_numpy(blob).cuda(), torch.from_numpy(off).cuda(), max_len=int(lens.max()))
        sample = np.linspace(0, n - 1, args.sample).astype(np.int64)
        needles = [panel[p].tobytes() for p in range(nn)]
        nd = B.Strings.from_fixed(panel.copy())
        cap = 2 * n
        bufs = dict(hits=torch.empty((cap, 6), dtype=torch.int32, device="cuda"), count=torch.empty(1, dtype=torch.int64, device="cuda"),
                    nearest=torch.empty(n, dtype=torch.int64, device="cuda"), best=torch.empty((n, 3), dtype=torch.int64, device="cuda"),
                    per_haystack=torch.empty(n, dtype=torch.int32, device="cuda"))
        cross = lambda: B.levenshtein_search_cross_with_opts(nd, hs, k, COSTS, cap=cap, **bufs)          # noqa: E731
        if args.trace_row:
            for _ in range(3):
                cross()
            torch.cuda.synchronize()
            emit(dict(row=row, traced_calls=3, kernel=T.last_kernel_name()))
            continue
        out = cross()
        ok = verify(out, needles, blob, off, sample, k)
        kern = T.last_kernel_name()
        n_hits = int(out[1].item())
        base = {"row": row, "haystacks": n, "bytes": int(off[-1]), "needles": nn, "needle": nl, "k": k, "reps": args.reps, "windows": args.windows,
                "hits": n_hits, "verified": ok, "kernel": kern}
        if nl <= 32:                                               # the control: the 32-byte entry runs the same kernels
            old = lambda: B.levenshtein_search_cross(nd, hs, k, COSTS, cap=cap, **bufs)                  # noqa: E731
            old()
            same = T.last_kernel_name() == kern
            a, sa, b, sb = alternating(cross, old, args.reps, args.windows)
            emit(dict(base, ms_with_opts=a, spread_with_opts=sa, ms_search_cross=b, spread_search_cross=sb, same_kernel=same))
            continue
        sides = [B.Strings.shared(nd_, n) for nd_ in needles]
        m = torch.empty((n, 1, 3), dtype=torch.int64, device="cuda")
        c = torch.empty(n, dtype=torch.int32, device="cuda")

        def loop():
            for s in sides:
                B.levenshtein_search_batch(s, hs, k, T.SearchType.Best, COSTS, cap=1, matches=m, counts=c)

        a, sa, b, sb = alternating(cross, loop, args.reps, args.windows)
        emit(dict(base, ms_cross=a, spread_cross=sa, ms_loop=b, spread_loop=sb, loop_over_cross=b / a, loop_kernel=T.last_kernel_name()))
        if args.anchored_row and row == "panel_12x34":            # the anchored route on one small row: 65,536 haystacks
            small = 1 << 16
            hs2 = B.Strings(hs.blob, hs.off[:small + 1].contiguous(), max_len=int(lens.max()))
            anch = lambda: B.levenshtein_search_cross_with_opts(nd, hs2, k, COSTS, True, cap=cap, **bufs)      # noqa: E731
            out = anch()
            ok2 = verify(out, needles, blob, off, sample[sample < small][:100], k, True)
            anch()
            torch.cuda.synchronize()
            ts = [window(anch, args.reps) for _ in range(args.windows)]
            emit(dict(row="anchored_12x34", haystacks=small, needles=nn, needle=nl, k=k, ms_cross=statistics.median(ts),
                      spread_cross=(max(ts) - min(ts)) / statistics.median(ts), verified=ok2, kernel=T.last_kernel_name()))
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
