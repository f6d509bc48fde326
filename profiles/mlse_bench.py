#!/usr/bin/env python3
"""Viterbi sequence detector timings: one JSON line per measurement.

  timeout 900 python3 profiles/mlse_bench.py [--log2n 30] [--reps 5] [--quick]

The record is dfe_bench.py's: n = 2^30 resident int16 samples at 8 samples per bit, random +-400 data through an echo of 0.7
one bit late plus Gaussian noise of sigma 150.  Feed-forward of 8 taps (integrate and dump, shift 2: y = 800 d + 560 d') and
of 64 (the same eight and 56 zeros), targets of memory 1 and 4 under the default geometry (B, W, D = 192, 32, 32).  In the
same session bbb_dfe_run at nfb = mem and bbb_fir_slice at the same taps and stride are timed; every line of the detector
carries the ratios to both and the lane-instruction estimate of DESIGN.md 23 (20 NS (1 + (W + D) / B) per symbol at 39 T/s).
A last group varies the geometry at memory 1.
Medians of `reps` calls (hipEvents on the stream) after a warm-up call.  --quick: n = 2^26, 2 repetitions."""
import argparse
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import basebandboard_amd as bbb  # noqa: E402
from dfe_bench import line, record, timed  # noqa: E402

LANE_RATE = 39e12          # lane instructions per second
G = {1: [800, 560], 4: [800, 560, 15, -8, 3]}
FB = {1: [2240], 4: [2240, 60, -30, 10]}


def estimate_ms(nsym, mem, B=192, W=32, D=32):
    return 20 * (1 << mem) * (1 + (W + D) / B) * nsym / LANE_RATE * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    n, reps = (1 << 26, 2) if args.quick else (1 << args.log2n, args.reps)
    x = record(n)
    for nt in (8, 64):
        taps = [1] * 8 + [0] * (nt - 8)
        f = bbb.FIR(taps, shift=2)
        ref, lo, hi = timed(lambda: f.slice(x, stride=8, phase=7), reps)
        line(case="fir_slice", ntaps=nt, stride=8, n=n, ms=ref, ms_min=lo, ms_max=hi, gbps_read=2 * n / ref / 1e6)
        for mem in (1, 4):
            d = bbb.DFE(f, FB[mem], 8, phase=7)
            dfe, lo, hi = timed(lambda: d.slice(x), reps)
            line(case="dfe", ntaps=nt, nfb=mem, n=n, ms=dfe, ms_min=lo, ms_max=hi, ratio_to_fir_slice=dfe / ref)
            m = bbb.MLSE(f, G[mem], 8, phase=7)
            med, lo, hi = timed(lambda: m.slice(x), reps)
            est = estimate_ms(n // 8, mem)
            line(case="mlse", ntaps=nt, mem=mem, n=n, ms=med, ms_min=lo, ms_max=hi, ratio_to_fir_slice=med / ref, ratio_to_dfe=med / dfe,
                 estimate_ms=est, measured_over_estimate=med / est, gsym_per_s=n / 8 / med / 1e6)
    f = bbb.FIR([1] * 8, shift=2)
    for B, W, D in ((64, 32, 32), (192, 16, 16), (384, 64, 64), (448, 32, 32)):
        m = bbb.MLSE(f, G[1], 8, phase=7, block_symbols=B, warmup_symbols=W, lookahead_symbols=D)
        med, lo, hi = timed(lambda: m.slice(x), reps)
        est = estimate_ms(n // 8, 1, B, W, D)
        line(case="mlse_geometry", ntaps=8, mem=1, B=B, W=W, D=D, n=n, ms=med, ms_min=lo, ms_max=hi, estimate_ms=est, measured_over_estimate=med / est)


if __name__ == "__main__":
    main()
