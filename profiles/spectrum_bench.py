#!/usr/bin/env python3
"""Autocorrelation timings: one JSON line per measurement.

  python3 profiles/spectrum_bench.py [--n 1e9] [--reps 5] [--quick]

  capture12    bbb_acf_accumulate_i16 over n 12-bit samples in HBM (random in [-2048, 2048)), 256 and 4096 lags
  capture16    the same over full-range int16 samples (the nine-MFMA form), 256 lags
  fill         a bare bbb_tx_fill_i16 of n samples into HBM (noise on), the yardstick of the transmitter side
  eye_bathtub  one bathtub-only bbb_tx_eye_run over n samples at the default chunk
  tx256        bbb_tx_acf_run over n first elements, 256 lags, default chunk (2^26)
Multiply-adds per second count n * nlags; the i8 MFMA peak is 1024 SIMDs x 16384 multiply-adds per 16 cycles at 2.4 GHz.
Medians of `reps` calls (hipEvents on the stream) after ramp fills.  --quick: n = 2^28, 2 repetitions (profiler runs)."""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402
from basebandboard_amd.eye import BIT_SAMPLE0, EyeConfig, TxEye  # noqa: E402
from basebandboard_amd.spectrum import TxAcf, capture_acf  # noqa: E402

DEV = torch.device("cuda", 0)
PEAK_MAC_PER_S = 1024 * 16384 / 16 * 2.4e9


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    n, reps = (1 << 28, 2) if args.quick else (int(args.n), args.reps)
    ramp = bbb.TX(31, 1, 0, 16, 1, 8, device=0)
    buf = torch.empty(1 << 28, dtype=torch.int16, device=DEV)
    for _ in range(20):
        ramp.generate(1 << 28, out=buf, stream_on=False)
    torch.cuda.synchronize()
    del buf

    x = torch.randint(-2048, 2048, (n,), dtype=torch.int16, device=DEV)
    for nlags in (256, 4096):
        acf = torch.zeros(nlags + 1, dtype=torch.int64, device=DEV)
        med, lo, hi = timed(lambda: capture_acf(x, nlags, acf=acf), reps)
        line(what="capture12", n=n, nlags=nlags, ms=med, ms_min=lo, ms_max=hi, tmac_per_s=n * nlags / med / 1e9,
             share_of_i8_peak=n * nlags / (med / 1e3) / PEAK_MAC_PER_S)
    x = torch.randint(-32768, 32768, (n,), dtype=torch.int16, device=DEV)
    acf = torch.zeros(257, dtype=torch.int64, device=DEV)
    med, lo, hi = timed(lambda: capture_acf(x, 256, acf=acf), reps)
    line(what="capture16", n=n, nlags=256, ms=med, ms_min=lo, ms_max=hi, tmac_per_s=n * 256 / med / 1e9,
         share_of_i8_peak=n * 256 / (med / 1e3) / PEAK_MAC_PER_S)

    tx = bbb.TX(31, 1, 0, 16, 1, 8, device=0)
    out = x                                                            # reuse the buffer: n int16
    med_fill, lo, hi = timed(lambda: tx.generate(n, out=out, stream_on=False), reps)
    line(what="fill", n=n, ms=med_fill, ms_min=lo, ms_max=hi)
    del x, out
    tub = torch.zeros((8, 2), dtype=torch.uint64, device=DEV)
    with TxEye(tx, EyeConfig(col_origin=BIT_SAMPLE0), chunk_samples=1 << 26) as e:
        med_eye, lo, hi = timed(lambda: e.run(n, 0, None, tub, want_hist=False), reps)
    line(what="eye_bathtub", n=n, ms=med_eye, ms_min=lo, ms_max=hi)
    with TxAcf(tx, 256) as a:
        acf = a.run(1 << 20)
        med, lo, hi = timed(lambda: a.run(n, 0, acf), reps)
    line(what="tx256", n=n, nlags=256, chunk=1 << 26, ms=med, ms_min=lo, ms_max=hi, ratio_to_fill=med / med_fill,
         ratio_to_eye_bathtub=med / med_eye)


if __name__ == "__main__":
    main()
