#!/usr/bin/env python3
"""NCO timings: one JSON line per measurement.

  python3 profiles/nco_bench.py [--n 1e9] [--reps 5] [--quick]

  const        bbb_nco_run with constant inputs over n samples, at fcw = 2^20 (NCOTest) and, for the fcw sensitivity,
               2^10, 2^14, 2^16, 2^17, 2^23 + 1 and 0x5A5A5A
  fm           an fm buffer (random full-range int32), am and pm constant
  all          fm, am and pm buffers (random)
GB/s counts the bytes the call must move: 2 per sample written, 4 per fm value, 2 per am or pm value read.
Medians of `reps` calls (hipEvents on the stream) after a warm-up call.  --quick: n = 2^28, 2 repetitions (profiler runs)."""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402

DEV = torch.device("cuda", 0)
FCWS = {"2^10": 1 << 10, "2^14": 1 << 14, "2^16": 1 << 16, "2^17": 1 << 17, "2^20": 1 << 20, "2^23+1": (1 << 23) + 1,
        "0x5A5A5A": 0x5A5A5A}


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
    ap.add_argument("--only", default="", help="comma-separated subset of const,fm,all")
    args = ap.parse_args()
    n, reps = (1 << 28, 2) if args.quick else (int(args.n), args.reps)
    only = set(args.only.split(",")) if args.only else {"const", "fm", "all"}
    x = torch.empty(n, dtype=torch.int16, device=DEV)
    if "const" in only:
        for name, fcw in FCWS.items():
            o = bbb.NCO(fcw, 1 << 14)
            med, lo, hi = timed(lambda: o.generate(n, out=x), reps)
            line(case="const", fcw=name, n=n, ms=med, ms_min=lo, ms_max=hi, gbps=2 * n / med / 1e6)
            o.close()
    if only & {"fm", "all"}:
        g = torch.Generator(device=DEV)
        g.manual_seed(1)
        fm = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int32, device=DEV, generator=g)
        o = bbb.NCO(1 << 20, 1 << 14)
        if "fm" in only:
            med, lo, hi = timed(lambda: o.generate(n, fm=fm, out=x), reps)
            line(case="fm", fcw="2^20", n=n, ms=med, ms_min=lo, ms_max=hi, gbps=6 * n / med / 1e6)
        if "all" in only:
            am = torch.randint(-2 ** 15, 2 ** 15, (n,), dtype=torch.int16, device=DEV, generator=g).view(torch.uint16)
            pm = torch.randint(-512, 512, (n,), dtype=torch.int16, device=DEV, generator=g)
            med, lo, hi = timed(lambda: o.generate(n, fm=fm, am=am, pm=pm, out=x), reps)
            line(case="all", fcw="2^20", n=n, ms=med, ms_min=lo, ms_max=hi, gbps=10 * n / med / 1e6)
        o.close()


if __name__ == "__main__":
    main()
