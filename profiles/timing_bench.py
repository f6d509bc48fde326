#!/usr/bin/env python3
"""Symbol timing recovery timings: one JSON line per measurement.

  timeout 900 python3 profiles/timing_bench.py [--log2n 30] [--reps 5] [--quick]

The record is n = 2^30 resident int16 samples at 8 samples per bit: random +-400 data plus Gaussian noise of sigma 150
(torch's generator).  bbb_timing_run at P 8, L 64, 8 taps (integrate and dump), bits only and with soft values and phases; the
yardstick is bbb_fir_slice at the same taps and stride 8 in the same session.  Then chunk_blocks 64, 256, 1024 (the default)
and 4096, which moves work between the chunk walks and the one-workgroup chain.  The kernels' shares of a call come from a
kernel trace of this script (profiles/README.md has the command).
Medians of `reps` calls (hipEvents on the stream) after a warm-up call; a call ends with the one read of nbits_dev.
--quick: n = 2^26, 2 repetitions."""
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


def record(n):
    """+-400 data at 8 samples per bit, noise of sigma 150."""
    x = torch.empty(n, dtype=torch.int16, device=DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    step = 1 << 24
    for a in range(0, n, step):
        b = min(n, a + step)
        bits = torch.randint(0, 2, ((b - a + 7) // 8,), dtype=torch.int16, device=DEV, generator=g) * 800 - 400
        noise = (torch.randn(b - a, device=DEV, generator=g) * 150).to(torch.int16)
        x[a:b] = bits.repeat_interleave(8)[:b - a] + noise
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    n, reps = (1 << 26, 2) if args.quick else (1 << args.log2n, args.reps)
    x = record(n)
    f = bbb.FIR([1] * 8, shift=2)
    ref, lo, hi = timed(lambda: f.slice(x, stride=8, phase=7), reps)
    line(case="fir_slice", ntaps=8, stride=8, n=n, ms=ref, ms_min=lo, ms_max=hi, gbps_read=2 * n / ref / 1e6)
    for soft in (False, True):
        tr = bbb.TimingRecovery(8, f)
        fn = (lambda: tr.recover(x)) if soft else (lambda: tr.slice(x))
        med, lo, hi = timed(fn, reps)
        st = tr.stats()
        line(case="timing", ntaps=8, spb=8, block_symbols=64, soft=soft, n=n, ms=med, ms_min=lo, ms_max=hi, ratio_to_fir_slice=med / ref,
             gbps_read=2 * n / med / 1e6, blocks=st["blocks"] // (reps + 1), moves_share=st["moves"] / st["blocks"],
             wraps=(st["wraps_up"] + st["wraps_down"]) // (reps + 1))
    for chunk in (64, 256, 1024, 4096):
        tr = bbb.TimingRecovery(8, f, chunk_blocks=chunk)
        med, lo, hi = timed(lambda: tr.slice(x), reps)
        line(case="timing_chunk", chunk_blocks=chunk, n=n, ms=med, ms_min=lo, ms_max=hi, ratio_to_fir_slice=med / ref)


if __name__ == "__main__":
    main()
