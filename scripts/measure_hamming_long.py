"""Hamming distance of long strings on one GPU: the sliced form (ham_long_kernel) against the one-wavefront-per-pair
kernel it routes around (hamming_batch_kernel, pinned with TA_FORCE_HAM_SLICED=0), on inputs resident in HBM.  Rows:
  a  1 pair x 1 GiB                      (the old route on 64 MiB of it: one wavefront at a fraction of a GB/s)
  b  16 x 64 MiB
  c  2,000 x 64 KiB
  d  CSR, 4,096 pairs of 1 KiB / 16 KiB / 256 KiB / 4 MiB
  e  1,000,000 x 1 KiB                   (2 GB: past the Infinity Cache; the unchanged kernel's HBM-side figure)
  f  10,000 x 1 KiB                      (bench.py's cfg1: 20 MB, inside the Infinity Cache; the unchanged kernel)
then a sweep of the slice length and the grid cap on rows a and c, the crossover of the two routes over (pairs, length), and ta_hamming
on a 1 GiB pair in HOST memory (staged 64 MiB at a time: bound by the copies).  Every row first checks that the two routes give the
same answers.  bytes = both strings; fractions are of 8 TB/s (the data sheet) and of 6.29 TB/s (a device-to-device copy's measured rate).
Times: every route is warmed up, then timed in `--trials` windows of at least `--window-ms` each with device events, the routes
alternating inside a trial; a row reports the median window and the fastest and slowest one.  One JSON line per row."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("TA_TUNING", "1")        # (the route and slice switches are honoured only under TA_TUNING)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import triple_accel_amd as T  # noqa: E402
from triple_accel_amd import batch as B  # noqa: E402

PEAK, COPY = 8.0e12, 6.29e12
SWITCHES = ("TA_FORCE_HAM_SLICED", "TA_HAM_SLICE", "TA_HAM_GRID")


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
        once = max(window(fn, 1), 1e-3)
        reps[name] = max(1, int(window_ms / once) + 1)
    got = {name: [] for name in fns}
    for _ in range(trials):
        for name, fn in fns.items():
            got[name].append(window(fn, reps[name]))
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in got.items()}


def route(a, b, out, **env):
    """a call of hamming_batch under the given switches (set around the call: the library reads them at every call)"""
    def fn():
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k, v in env.items():
            os.environ[k] = str(v)
        B.hamming_batch(a, b, out=out)
    return fn


def rates(ms, nbytes):
    return dict(ms=ms[0], ms_range=ms[1:], tb_per_s=nbytes / ms[0] / 1e9, of_8_tb=nbytes / (ms[0] * 1e-3) / PEAK, of_copy_rate=nbytes / (ms[0] * 1e-3) / COPY)


def random_bytes(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (n + 16,), dtype=torch.uint8, device="cuda", generator=g)


def strided(n, length, seed):
    a = random_bytes(n * length, seed)
    b = a.clone()
    b[::97] ^= 0x0C
    return B.Strings(a, None, stride=length, length=length, n=n), B.Strings(b, None, stride=length, length=length, n=n)


def ragged(n, lens, seed):
    rng = np.random.default_rng(seed)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(rng.choice(lens, n), out=off[1:])
    a = random_bytes(int(off[-1]), seed)
    b = a.clone()
    b[::97] ^= 0x0C
    o = torch.from_numpy(off).cuda()
    return B.Strings(a, o, max_len=max(lens)), B.Strings(b, o, max_len=max(lens)), int(off[-1])


def kernel_of(fn):
    fn()
    torch.cuda.synchronize()
    return T.last_kernel_name()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--sweep-window-ms", type=float, default=30.0)
    ap.add_argument("--scale", type=float, default=1.0, help="scales every row's bytes (a quick run: 0.01)")
    ap.add_argument("--host-gib", type=float, default=1.0, help="the host pair of the last row, 0: skip it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "measure_hamming_long.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no other route"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    sink = open(args.out, "w")

    def emit(**row):
        line = json.dumps(row)
        print(line, flush=True)
        sink.write(line + "\n")
        sink.flush()

    sc = lambda x: max(1, int(x * args.scale))                                      # noqa: E731
    GiB, MiB, KiB = 1 << 30, 1 << 20, 1 << 10
    # ---- rows a .. f
    keep = {}
    for name, n, length, old_len in (("a", 1, sc(GiB), sc(64 * MiB)), ("b", 16, sc(64 * MiB), None), ("c", sc(2000), 64 * KiB, None),
                                     ("d", sc(4096), None, None), ("e", sc(1000000), KiB, None), ("f", 10000, KiB, None)):
        if name == "d":
            a, b, total = ragged(n, [KiB, 16 * KiB, 256 * KiB, 4 * MiB], 4)
        else:
            a, b = strided(n, length, ord(name))
            total = n * length
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        natural = route(a, b, out)
        kernel = kernel_of(natural)
        answers = out.clone()
        row = dict(row=name, pairs=n, length=length, bytes=2 * total, kernel=kernel, trials=args.trials, window_ms=args.window_ms)
        if name in "abcd":
            if old_len:                                                             # the old route on a shorter piece of the same pair
                ao, bo = (B.Strings(s.blob, None, stride=old_len, length=old_len, n=1) for s in (a, b))
                out_o = torch.empty(1, dtype=torch.int32, device="cuda")
                old = route(ao, bo, out_o, TA_FORCE_HAM_SLICED=0)
                check = route(ao, bo, out_o, TA_FORCE_HAM_SLICED=1)
                check(); torch.cuda.synchronize(); new_answer = out_o.clone()
                old_kernel = kernel_of(old)
                same, old_bytes = bool((out_o == new_answer).all()), 2 * old_len
            else:
                old = route(a, b, out, TA_FORCE_HAM_SLICED=0)
                old_kernel = kernel_of(old)
                same, old_bytes = bool((out == answers).all()), 2 * total
            ms = timed({"new": natural, "old": old}, args.trials, args.window_ms)
            row.update(rates(ms["new"], 2 * total), routes_agree=same, old_kernel=old_kernel, old_bytes=old_bytes,
                       old={k: v for k, v in rates(ms["old"], old_bytes).items()},
                       new_over_old_rate=(2 * total / ms["new"][0]) / (old_bytes / ms["old"][0]))
        else:
            ms = timed({"new": natural}, args.trials, args.window_ms)
            row.update(rates(ms["new"], 2 * total))
        emit(**row)
        if name in "ac":
            keep[name] = (a, b, out, 2 * total, answers)
        else:
            del a, b, out
            torch.cuda.empty_cache()
    # ---- the slice length and the grid cap, rows a and c
    for name, (a, b, out, nbytes, answers) in keep.items():
        for S in (4 * KiB, 16 * KiB, 64 * KiB):
            for grid in (2048, 4096, 8192, 16384, 32768):
                fn = route(a, b, out, TA_FORCE_HAM_SLICED=1, TA_HAM_SLICE=S, TA_HAM_GRID=grid)
                kernel = kernel_of(fn)
                ok = bool((out == answers).all())
                ms = timed({"new": fn}, args.trials, args.sweep_window_ms)
                emit(row="sweep_" + name, slice=S, grid_waves=grid, kernel=kernel, answers_agree=ok, **rates(ms["new"], nbytes))
    keep.clear()
    torch.cuda.empty_cache()
    # ---- the crossover of the two routes
    for n in (1, 64, 1024, 8192):
        for length in (512, 1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072):
            if n * length * args.scale < 1:
                continue
            a, b = strided(n, length, 1000 + n)
            out = torch.empty(n, dtype=torch.int32, device="cuda")
            new, old = route(a, b, out, TA_FORCE_HAM_SLICED=1), route(a, b, out, TA_FORCE_HAM_SLICED=0)
            new(); torch.cuda.synchronize(); want = out.clone()
            old(); torch.cuda.synchronize()
            same = bool((out == want).all())
            ms = timed({"new": new, "old": old}, args.trials, args.sweep_window_ms)
            for k in SWITCHES:
                os.environ.pop(k, None)
            emit(row="crossover", pairs=n, length=length, routes_agree=same, new_ms=ms["new"][0], new_ms_range=ms["new"][1:], old_ms=ms["old"][0],
                 old_ms_range=ms["old"][1:], old_over_new=ms["old"][0] / ms["new"][0], rule_slices=kernel_of(route(a, b, out)) == "ham_long_kernel")
            del a, b, out
    # ---- ta_hamming on a pair in host memory: copies, 64 MiB at a time
    if args.host_gib > 0:
        for k in SWITCHES:
            os.environ.pop(k, None)
        n = sc(int(args.host_gib * GiB))
        rng = np.random.default_rng(7)
        a = rng.integers(0, 256, n, dtype=np.uint8)
        b = a.copy()
        b[::97] ^= 0x0C
        ab, bb = a.tobytes(), b.tobytes()
        want = int((a != b).sum())
        del a, b
        got, secs = None, []
        for _ in range(3):
            t0 = time.perf_counter()
            got = T.hamming(ab, bb)
            secs.append(time.perf_counter() - t0)
        emit(row="host", length=n, bytes=2 * n, answer_agrees=got == want, kernel=T.last_kernel_name(), seconds=secs,
             gb_per_s_best=2 * n / min(secs) / 1e9, note="host clock around the whole call: two pageable host-to-device copies per 64 MiB chunk, then the kernel")
    sink.close()


if __name__ == "__main__":
    main()
