#!/usr/bin/env python3
"""Sinc interpolator timings: one JSON line per measurement.

  python3 profiles/sinc_bench.py [--log2n 26] [--reps 5] [--quick] [--only interp,eye,phase]

  interp   bbb_sinc_interpolate over n = 2^26 inputs (2^30 outputs) for the four type combinations; GB/s counts the bytes
           written (16 or 32 per input sample), the yardstick being the NCO's constant kernel (profiles/nco_bench.py
           --only const, run in the same session), which writes with the same 16-byte stores
  eye      bbb_sinc_eye_run over the same int16 record with chunks of 2^20, 2^22 and 2^24 inputs, against
           bbb_eye_accumulate_i16 alone over the 2^30 resident interpolated samples (a bound the composite cannot beat) and
           against the two calls made separately without chunking
  phase    RX.phase_search(interpolate=True) over a 2^24-sample capture at 4 samples per bit: the whole call (host time,
           it returns counters), the interpolation alone, and the 64 slice-and-detect passes alone
Medians of `reps` calls (hipEvents on the stream) after a warm-up call.  --quick: n = 2^24, 2 repetitions (profiler runs)."""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402
from basebandboard_amd import _lib  # noqa: E402
from basebandboard_amd.eye import EyeConfig, capture_eye  # noqa: E402

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


def wall(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def line(**kw):
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in kw.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated subset of interp,eye,phase")
    args = ap.parse_args()
    n, reps = (1 << 24, 2) if args.quick else (1 << args.log2n, args.reps)
    only = set(args.only.split(",")) if args.only else {"interp", "eye", "phase"}
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    s = bbb.SincInterpolator()
    x16 = torch.randint(-2048, 2048, (n,), dtype=torch.int16, device=DEV, generator=g)
    if "interp" in only:
        x8 = (x16 >> 4).to(torch.int8)
        for xin, shift in ((x8, 0), (x16, 4)):
            for odt in (torch.int8, torch.int16):
                out = torch.empty(16 * n, dtype=odt, device=DEV)
                med, lo, hi = timed(lambda: s.interpolate(xin, shift=shift, out=out), reps)
                line(case="interp", inp=str(xin.dtype)[6:], out=str(odt)[6:], n=n, ms=med, ms_min=lo, ms_max=hi,
                     gbps_written=16 * n * out.element_size() / med / 1e6)
                del out
    if "eye" in only:
        eye = EyeConfig(ncols=64, shift=0)
        y = s.interpolate(x16, shift=4, out_dtype=torch.int16)
        hist = torch.zeros(256, 64, dtype=torch.uint64, device=DEV)
        med, lo, hi = timed(lambda: capture_eye(y, 0, eye, hist), reps)
        line(case="eye_alone", samples=16 * n, ms=med, ms_min=lo, ms_max=hi, gbps_read=32 * n / med / 1e6)

        def separate():
            s.interpolate(x16, shift=4, out=y)
            capture_eye(y, 0, eye, hist)
        med, lo, hi = timed(separate, reps)
        line(case="eye_two_calls", n=n, ms=med, ms_min=lo, ms_max=hi)
        del y
        lib = _lib.lib()
        cfg, ec = _lib.SincCfg(2, 2, 4), eye._c()
        st = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
        for lg in (20, 22, 24):
            e = C.c_void_p()
            _lib.check(lib.bbb_sinc_eye_open(C.byref(cfg), C.byref(ec), 1 << lg, 0, st, C.byref(e)), "bbb_sinc_eye_open")
            med, lo, hi = timed(lambda: _lib.check(lib.bbb_sinc_eye_run(e, C.c_void_p(x16.data_ptr()), n, 0, 0,
                                                                         C.c_void_p(hist.data_ptr())), "bbb_sinc_eye_run"), reps)
            line(case="sinc_eye", chunk_in=f"2^{lg}", n=n, ms=med, ms_min=lo, ms_max=hi)
            _lib.check(lib.bbb_sinc_eye_close(e), "bbb_sinc_eye_close")
    if "phase" in only:
        m = min(n, 1 << 24)
        cap = bbb.TX(31, 1, 0, 16, 1, 6, device=0).generate(2 * m)[::2].contiguous()     # 4 samples per bit
        rx = bbb.RX(31, 4, 0)
        med, lo, hi = wall(lambda: rx.phase_search(cap, interpolate=True, shift=1), reps)
        line(case="phase_search_interpolated", samples=m, phases=64, ms=med, ms_min=lo, ms_max=hi)
        med, lo, hi = timed(lambda: rx.interpolate(cap, shift=1), reps)
        line(case="phase_interpolation_alone", samples=m, ms=med, ms_min=lo, ms_max=hi)
        y = rx.interpolate(cap, shift=1)
        wide = bbb.RX(31, 64, 0)
        med, lo, hi = wall(lambda: wide.phase_search(y), reps)
        line(case="phase_64_passes_alone", samples=16 * m, ms=med, ms_min=lo, ms_max=hi)
        stats, best = rx.phase_search(cap, interpolate=True, shift=1)
        line(case="phase_result", best=best, errors=stats[best]["errors"], bits=stats[best]["bits"])


if __name__ == "__main__":
    main()
