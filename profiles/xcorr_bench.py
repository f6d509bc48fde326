#!/usr/bin/env python3
"""Pulse-response counter timings: one JSON line per measurement, all in one session.

  python3 profiles/xcorr_bench.py [--n 1e9] [--reps 10] [--quick]

Over n resident int16 samples (the transmitter's waveform at noise_var 8, generated once) and the PRBS-31 bits behind them
  xcorr_64, xcorr_256   bbb_xcorr_accumulate_i16 at spb 8, origin 17, 64 and 256 lags
  acf_256               bbb_acf_accumulate_i16 at 256 lags over the same samples: the yardstick that already exists
and over the transmitter's own stream, never materialised
  tx_xcorr_64           bbb_tx_xcorr_run at 64 lags (fill, data bits and correlation chunk by chunk)
  tx_acf_256            bbb_tx_acf_run at 256 lags
Medians of `reps` calls (hipEvents on the stream) after two warm-up calls.  --quick: 2^26 samples, 3 calls each (kernel-trace
runs)."""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402

DEV = torch.device("cuda", 0)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def line(what, n, t, **kw):
    med, lo, hi = t
    print(json.dumps({"what": what, "samples": n, "ms": med, "ms_min": lo, "ms_max": hi, "Gsamples_per_s": n / med / 1e6, **kw}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    n = (1 << 26) if a.quick else int(a.n) // 64 * 64
    reps = 3 if a.quick else a.reps
    tx = bbb.TX(31, 1, 0, 16, 1, 8, device=0)
    x = torch.empty(n, dtype=torch.int16, device=DEV)
    step = 1 << 26
    for off in range(0, n, step):
        tx.generate(min(step, n - off), first_sample=off, out=x[off:])
    bits = bbb.PRBS(31, device=0).generate(n // 8 + 64)
    for nlags in (64, 256):
        xc = torch.zeros(nlags, dtype=torch.int64, device=DEV)
        line(f"xcorr_{nlags}", n, timed(lambda: bbb.capture_xcorr(x, bits, 8, bbb.TX_BIT_ORIGIN, nlags, xcorr=xc), reps), nlags=nlags)
    acf = torch.zeros(257, dtype=torch.int64, device=DEV)
    line("acf_256", n, timed(lambda: bbb.capture_acf(x, 256, acf=acf), reps), nlags=256)
    del x, bits
    with bbb.TxXcorr(tx, nlags=64) as t:
        xc = torch.zeros(64, dtype=torch.int64, device=DEV)
        line("tx_xcorr_64", n, timed(lambda: t.run(n, xcorr=xc), reps), nlags=64)
    with bbb.TxAcf(tx, nlags=256) as t:
        line("tx_acf_256", n, timed(lambda: t.run(n, acf=acf), reps), nlags=256)


if __name__ == "__main__":
    main()
