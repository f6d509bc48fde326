#!/usr/bin/env python3
"""BER sweep timings: one JSON line per measurement.

  python3 profiles/tx_sweep_bench.py [--n 1e9] [--reps 5] [--quick]

  eye_bathtub   one bathtub-only bbb_tx_eye_run over n samples (the cost of ONE setting the old way), chunk 2^26
  sweep16       bbb_tx_ber_sweep_run, 16 noise_var settings of one shape (threshold 0), chunk 2^26 and 2^28
  sweep16_thr   the same with a nonzero threshold (the kernel's threshold step)
  grid512       the 32 x 16 shape_sel x noise_var grid, chunk 2^26; against 512 bathtub-only eye runs, extrapolated from
                `eye_bathtub` (not run)
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
from basebandboard_amd.txsweep import TxBerSweep, TxSetting  # noqa: E402

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

    tx = bbb.TX(31, 1, 0, 16, 1, 8, device=0)
    tub = torch.zeros((8, 2), dtype=torch.uint64, device=DEV)
    with TxEye(tx, EyeConfig(col_origin=BIT_SAMPLE0), chunk_samples=1 << 26) as e:
        med_eye, lo, hi = timed(lambda: e.run(n, 0, None, tub, want_hist=False), reps)
    line(what="eye_bathtub", n=n, settings=1, ms=med_eye, ms_min=lo, ms_max=hi)

    for chunk in (1 << 26, 1 << 28):
        for name, thr in (("sweep16", 0), ("sweep16_thr", 40)):
            if thr and chunk != 1 << 26:
                continue
            with TxBerSweep(tx, [TxSetting(noise_var=v, threshold=thr) for v in range(16)], chunk_samples=chunk) as s:
                cnt = s.run(1 << 20)
                med, lo, hi = timed(lambda: s.run(n, 0, cnt), reps)
            line(what=name, chunk=chunk, n=n, settings=16, ms=med, ms_min=lo, ms_max=hi, ratio_to_one_eye=med / med_eye,
                 gsetting_samples_per_s=16 * n / med / 1e6)

    grid = [TxSetting(shape_sel=sh, noise_var=v) for sh in range(32) for v in range(16)]
    with TxBerSweep(tx, grid, chunk_samples=1 << 26) as s:
        cnt = s.run(1 << 20)
        med, lo, hi = timed(lambda: s.run(n, 0, cnt), max(2, reps // 2))
    line(what="grid512", chunk=1 << 26, n=n, settings=512, ms=med, ms_min=lo, ms_max=hi,
         eye_runs_512_ms_extrapolated=512 * med_eye, speedup=512 * med_eye / med, gsetting_samples_per_s=512 * n / med / 1e6)


if __name__ == "__main__":
    main()
