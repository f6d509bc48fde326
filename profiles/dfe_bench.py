#!/usr/bin/env python3
"""Decision-feedback equalizer timings: one JSON line per measurement.

  timeout 900 python3 profiles/dfe_bench.py [--log2n 30] [--reps 5] [--quick]

The record is n = 2^30 resident int16 samples at 8 samples per bit: random +-400 data through an echo of 0.7 one bit late
plus Gaussian noise of sigma 150 (torch's generator), so that about half of the symbols are ambiguous without the feedback
and the regions' warm-ups have something to prove.  Feed-forward of 8 taps (integrate and dump) and of 64 (the same eight
and 56 zeros: the same decisions at eight times the filter), nfb 1 and 4, with and without soft values; the yardstick is
bbb_fir_slice at the same taps and stride in the same session.  Every line carries the ratio to its yardstick and the
call's share of regions that were not proven and that were repaired; a last group shortens the warm-up (default 64 symbols)
to show what it buys.
Medians of `reps` calls (hipEvents on the stream) after a warm-up call.  --quick: n = 2^26, 2 repetitions."""
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
    """+-400 data at 8 samples per bit, an echo of 0.7 one bit late, noise of sigma 150."""
    x = torch.empty(n, dtype=torch.int16, device=DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    step = 1 << 24
    last = torch.zeros(1, dtype=torch.int16, device=DEV)
    for a in range(0, n, step):
        b = min(n, a + step)
        bits = torch.randint(0, 2, ((b - a + 7) // 8,), dtype=torch.int16, device=DEV, generator=g) * 800 - 400
        echo = torch.cat([last, bits[:-1]]) * 7 // 10
        last = bits[-1:]
        noise = (torch.randn(b - a, device=DEV, generator=g) * 150).to(torch.int16)
        x[a:b] = (bits + echo).repeat_interleave(8)[:b - a] + noise
    return x


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
        for fb in ([2240], [2240, 60, -30, 10]):
            for soft in (False, True):
                d = bbb.DFE(f, fb, 8, phase=7)
                fn = (lambda: d.equalize(x)) if soft else (lambda: d.slice(x))
                med, lo, hi = timed(fn, reps)
                st = d.stats()
                line(case="dfe", ntaps=nt, nfb=len(fb), soft=soft, n=n, ms=med, ms_min=lo, ms_max=hi, ratio_to_fir_slice=med / ref,
                     gbps_read=2 * n / med / 1e6, regions=st["regions"] // (reps + 1), not_proven_share=st["not_proven"] / st["regions"],
                     repaired_share=st["repaired"] / st["regions"])
        if nt == 8:
            # what the warm-up buys: shorter ones leave starts unproven, and some of those wrong
            for w in (1, 2, 4, 8, 16):
                d = bbb.DFE(f, [2240, 60, -30, 10], 8, phase=7, warmup_symbols=w)
                med, lo, hi = timed(lambda: d.slice(x), reps)
                st = d.stats()
                line(case="dfe_warmup", ntaps=nt, nfb=4, warmup_symbols=w, n=n, ms=med, ms_min=lo, ms_max=hi, ratio_to_fir_slice=med / ref,
                     not_proven_share=st["not_proven"] / st["regions"], repaired_share=st["repaired"] / st["regions"])


if __name__ == "__main__":
    main()
