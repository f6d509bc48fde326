#!/usr/bin/env python3
"""FIR filter timings: one JSON line per measurement.

  timeout 600 python3 profiles/fir_bench.py [--log2n 30] [--reps 5] [--quick] [--only filter,decim,slice]

  filter   bbb_fir_filter over n = 2^30 int16 samples to int16 at 4, 64 and 256 taps, decim 1; GB/s counts the bytes read
           and written (4 per sample), the yardstick being profiles/sinc_bench.py --only interp, run in the same session
  decim    64 taps at decim 8, and at decim 8 from an input 2 bytes off a 16-byte boundary (the narrow loads)
  slice    bbb_fir_slice at 7 and 64 taps, stride 8, against bbb_fir_filter followed by bbb_rx_slice at stride 8 over the
           same record (the two calls the slicer replaces); the slicer must be the faster
Medians of `reps` calls (hipEvents on the stream) after a warm-up call.  --quick: n = 2^26, 2 repetitions (profiler runs)."""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402

DEV = torch.device("cuda", 0)


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def line(**kw):
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in kw.items()}), flush=True)


def taps(n):
    """n taps of both signs, sum |h| = 65535 - (65535 mod n)."""
    return [(65535 // n) * (1 if i % 3 else -1) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated subset of filter,decim,slice")
    args = ap.parse_args()
    n, reps = (1 << 26, 2) if args.quick else (1 << args.log2n, args.reps)
    only = set(args.only.split(",")) if args.only else {"filter", "decim", "slice"}
    x = torch.empty(n + 8, dtype=torch.int16, device=DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    step = 1 << 26
    for a in range(0, n + 8, step):
        b = min(n + 8, a + step)
        x[a:b] = torch.randint(-2048, 2048, (b - a,), dtype=torch.int16, device=DEV, generator=g)
    xa = x[:n]
    if "filter" in only:
        out = torch.empty(n, dtype=torch.int16, device=DEV)
        for nt in (4, 64, 256):
            f = bbb.FIR(taps(nt), shift=12)
            med, lo, hi = timed(lambda: f.filter(xa, out=out), reps)
            line(case="filter", ntaps=nt, decim=1, n=n, ms=med, ms_min=lo, ms_max=hi, gbps=4 * n / med / 1e6,
                 gmac_per_s=n * nt / med / 1e6)
        del out
    if "decim" in only:
        f = bbb.FIR(taps(64), shift=12)
        out = torch.empty(n // 8, dtype=torch.int16, device=DEV)
        med, lo, hi = timed(lambda: f.filter(xa, decim=8, out=out), reps)
        line(case="filter", ntaps=64, decim=8, n=n, ms=med, ms_min=lo, ms_max=hi, gbps_read=2 * n / med / 1e6)
        xo = x[1:n + 1]
        med, lo, hi = timed(lambda: f.filter(xo, decim=8, out=out), reps)
        line(case="filter_narrow_loads", ntaps=64, decim=8, n=n, ms=med, ms_min=lo, ms_max=hi, gbps_read=2 * n / med / 1e6)
        del out
    if "slice" in only:
        rx = bbb.RX(31, 8, 0)
        tmp = torch.empty(n, dtype=torch.int16, device=DEV)
        for nt in (7, 64):
            f = bbb.FIR(taps(nt))
            med, lo, hi = timed(lambda: f.slice(xa, stride=8), reps)
            line(case="slice", ntaps=nt, stride=8, n=n, ms=med, ms_min=lo, ms_max=hi, gbps_read=2 * n / med / 1e6)

            def two_calls():
                f.filter(xa, out=tmp)
                rx.slice(tmp)
            med2, lo2, hi2 = timed(two_calls, reps)
            line(case="filter_then_rx_slice", ntaps=nt, stride=8, n=n, ms=med2, ms_min=lo2, ms_max=hi2, slice_is_faster=med < med2)
        med, lo, hi = timed(lambda: rx.slice(xa), reps)
        line(case="rx_slice_alone", stride=8, n=n, ms=med, ms_min=lo, ms_max=hi)


if __name__ == "__main__":
    main()
