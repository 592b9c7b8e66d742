"""hamming_search over a batch of reads on one GPU: 1,048,576 haystacks of 100-250 bytes over ACGT, a shared 24-byte
needle planted with 0-2 substitutions in half of them.  Rows: Best and All at k = 2 (the shared-needle route), Best forced onto the
general route (TA_HSEARCH_BATCH_GENERAL=1), per-pair CSR needles of 16-32 bytes, an 8-byte shared needle at k = 1 (both routes) and
at k = 4, a 64-byte shared needle at k = 8; comparators of the same run: ta_levenshtein_search_batch Best at k = 2 on the same batch
(its scan route) and a loop of single hamming_search_simd_with_opts calls over the first 1,000 pairs.  Every row checks a sample of
pairs against the oracle before it is timed, and reports its algorithmic bytes (haystacks + offsets + counts) per second as a fraction
of 8 TB/s.  One JSON line per row."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("TA_TUNING", "1")        # (the A/B switch of the general-route row is honoured only under TA_TUNING)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import triple_accel_amd as T  # noqa: E402
from triple_accel_amd import batch as B  # noqa: E402
from triple_accel_amd import _native as N  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
PEAK = 8e12


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


def reads(n, seed, nl):
    """-> (needle, blob, off, lens): a copy of the nl-byte needle with 0-2 substitutions in every other haystack"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(100, 251, n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    blob = np.zeros(int(off[-1]) + 16, np.uint8)
    blob[: off[-1]] = ACGT[rng.integers(0, 4, int(off[-1]))]
    needle = ACGT[rng.integers(0, 4, nl)]
    planted = np.arange(1, n, 2)
    pos = off[planted] + (rng.random(planted.size) * (lens[planted] - nl + 1)).astype(np.int64)
    blob[pos[:, None] + np.arange(nl)[None, :]] = needle[None, :]
    for _ in range(2):
        hit = rng.random(planted.size) < 0.5
        blob[pos[hit] + rng.integers(0, nl, int(hit.sum()))] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    return needle.tobytes(), blob, off, lens


def hay_list(blob, off, idx):
    return [blob[off[i]:off[i + 1]].tobytes() for i in idx]


def verify(m, c, needles, hays, idx, k, st):
    got = B.matches_to_lists(m[idx], c[idx], allow_cut=True)
    cap = m.shape[1]
    want = [O.hamming_search_simd_with_opts(nd, h, k, st) for nd, h in zip(needles, hays)]
    counts_ok = c[idx].cpu().tolist() == [len(w) for w in want]
    return counts_ok and [[tuple(x) for x in r] for r in got] == [w[:cap] for w in want]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sample", type=int, default=300)
    args = ap.parse_args()
    n = args.pairs
    sample = np.linspace(0, n - 1, args.sample).astype(np.int64)

    def batch(nl, seed):
        needle, blob, off, lens = reads(n, seed, nl)
        hs = B.Strings(torch.from_numpy(blob).cuda(), torch.from_numpy(off).cuda(), max_len=int(lens.max()))
        return needle, blob, off, hs

    def row(name, side, needles_s, hs, shays, k, st, nbytes, general=False, extra=None):
        if general:
            os.environ["TA_HSEARCH_BATCH_GENERAL"] = "1"
        cap = 8 if st == O.BEST else 32
        m = torch.empty((n, cap, 3), dtype=torch.int64, device="cuda")
        c = torch.empty(n, dtype=torch.int32, device="cuda")
        B.hamming_search_batch(side, hs, k, st, cap=cap, matches=m, counts=c)
        torch.cuda.synchronize()
        ok = verify(m, c, needles_s, shays, sample, k, st)
        kern = N.lib().ta_last_kernel_name().decode()
        ms = timed(lambda: B.hamming_search_batch(side, hs, k, st, cap=cap, matches=m, counts=c), args.reps)
        os.environ.pop("TA_HSEARCH_BATCH_GENERAL", None)
        algo = nbytes + 8 * (n + 1) + 4 * n                      # haystacks once, their offsets, the counts
        print(json.dumps(dict(row=name, pairs=n, bytes=nbytes, k=k, ms=ms, verified=ok, kernel=kern, algo_bytes=algo,
                              frac_of_8TBs=algo / (ms * 1e-3) / PEAK, with_hits=int((c > 0).sum().item()), **(extra or {}))), flush=True)
        return ms

    needle, blob, off, hs = batch(24, 1)
    nbytes = int(off[-1])
    shays = hay_list(blob, off, sample)
    side = B.Strings.shared(needle, n)
    shared_s = [needle] * len(sample)
    best_ms = row("reads_best_k2", side, shared_s, hs, shays, 2, O.BEST, nbytes)
    row("reads_all_k2", side, shared_s, hs, shays, 2, O.ALL, nbytes)
    row("reads_best_k2_general_route", side, shared_s, hs, shays, 2, O.BEST, nbytes, general=True)
    # per-pair CSR needles of 16-32 bytes
    rng = np.random.default_rng(2)
    nl = rng.integers(16, 33, n)
    noff = np.zeros(n + 1, np.int64)
    np.cumsum(nl, out=noff[1:])
    nblob = np.zeros(int(noff[-1]) + 16, np.uint8)
    nblob[: noff[-1]] = ACGT[rng.integers(0, 4, int(noff[-1]))]
    nside = B.Strings(torch.from_numpy(nblob).cuda(), torch.from_numpy(noff).cuda(), max_len=32)
    row("per_pair_needles_16_32_best_k2", nside, hay_list(nblob, noff, sample), hs, shays, 2, O.BEST, nbytes)
    # the comparator on the same batch: ta_levenshtein_search_batch, Best, k = 2 (its scan route)
    m = torch.empty((n, 8, 3), dtype=torch.int64, device="cuda")
    c = torch.empty(n, dtype=torch.int32, device="cuda")
    lev = lambda: B.levenshtein_search_batch(side, hs, 2, O.BEST, (1, 1, 0, None), cap=8, matches=m, counts=c)    # noqa: E731
    lev()
    torch.cuda.synchronize()
    got = B.matches_to_lists(m[sample], c[sample])
    ok = [[tuple(x) for x in r] for r in got] == [O.levenshtein_search_naive_with_opts(needle, h, 2, O.BEST, (1, 1, 0, None), False) for h in shays]
    kern = N.lib().ta_last_kernel_name().decode()
    lev_ms = timed(lev, args.reps)
    print(json.dumps(dict(row="comparator_levenshtein_search_batch_best_k2", pairs=n, bytes=nbytes, k=2, ms=lev_ms, verified=ok, kernel=kern,
                          hamming_best_ms=best_ms, hamming_no_slower=bool(best_ms <= lev_ms))), flush=True)
    # the comparator: a loop of single calls over the first 1,000 pairs
    first = hay_list(blob, off, range(min(1000, n)))
    got = [list(T.hamming_search_simd_with_opts(needle, h, 2, T.SearchType.Best)) for h in first[:50]]
    ok = got == [[T.Match(*x) for x in O.hamming_search_simd_with_opts(needle, h, 2, O.BEST)] for h in first[:50]]
    t0 = time.perf_counter()
    for h in first:
        list(T.hamming_search_simd_with_opts(needle, h, 2, T.SearchType.Best))
    us = (time.perf_counter() - t0) * 1e6 / len(first)
    print(json.dumps(dict(row="comparator_single_call_loop", k=2, us_per_pair=us, pairs_timed=len(first), verified=ok,
                          est_ms_for_batch=us * n / 1e3)), flush=True)
    del hs, side, nside
    # an 8-byte shared needle at k = 1 (both routes) and at k = 4 (hit-dense: the rule sends it to the general route), a 64-byte one at k = 8
    for nl8, seed, cases in ((8, 3, ((1, False), (1, True), (4, False))), (64, 4, ((8, False),))):
        needle, blob, off, hs = batch(nl8, seed)
        shays = hay_list(blob, off, sample)
        for k, general in cases:
            row("shared_needle_%d_best_k%d%s" % (nl8, k, "_general_route" if general else ""), B.Strings.shared(needle, n),
                [needle] * len(sample), hs, shays, k, O.BEST, int(off[-1]), general=general, extra={"needle": nl8})
        del hs


if __name__ == "__main__":
    main()
