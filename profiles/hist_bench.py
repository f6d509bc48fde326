#!/usr/bin/env python3
"""Sample histogram timings: one JSON line per measurement.

  python3 profiles/hist_bench.py [--n 1000000000] [--reps 5] [--calls 4] [--quick] [--only hist,baseline,stream,eval]
                                 [--eval 1e12] [--log profiles/hist_bench.log]

  hist      bbb_awgn_hist over n samples of the shipped n256 generator, `calls` calls back to back at consecutive stream
            positions between two events: milliseconds per call and samples per second; then ONE call over 4, 32 and 256
            chunks of 2^30 samples (the library's own chunks, every next one announced), per 10^9 samples: the ends of a call
            against its steady state
  stream    bbb_awgn_stream_next of n int8 samples alone, the same way: the bare stream step the histogram is held against
  baseline  the same count the way a caller gets it without bbb_awgn_hist: bbb_awgn_stream_next of n int8 samples followed by
            torch.bincount of the bytes (and, once, torch.histc of them as floats: the faster of the two is the baseline)
  eval      grngstats.evaluate over --eval samples: wall time, and the evaluation as text (stderr: it is no JSON)
Medians of `reps` timings (hipEvents on the stream) after a warm-up.  --quick: n = 2^27, 2 repetitions (profiler runs).
All in ONE process and session, so that the ratios are of one box."""
import argparse
import json
import pathlib
import statistics
import sys
import time

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402
from basebandboard_amd import grngstats  # noqa: E402

DEV = torch.device("cuda", 0)
LOG = None


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
    text = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in kw.items()})
    print(text, flush=True)
    if LOG:
        LOG.write(text + "\n")
        LOG.flush()


def main():
    global LOG
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--only", default="", help="comma-separated subset of hist,stream,baseline,eval")
    ap.add_argument("--eval", type=float, default=1e12)
    ap.add_argument("--log", default="")
    args = ap.parse_args()
    n, reps = (1 << 27, 2) if args.quick else (int(args.n), args.reps)
    calls = args.calls
    only = set(args.only.split(",")) if args.only else {"hist", "stream", "baseline", "eval"}
    if args.log:
        LOG = open(args.log, "a")
    prop = torch.cuda.get_device_properties(0)
    line(case="setup", device=torch.cuda.get_device_name(0), arch=getattr(prop, "gcnArchName", "?"), cus=prop.multi_processor_count,
         hbm_gib=round(prop.total_memory / 2 ** 30), torch=torch.__version__, hip=torch.version.hip, n=n, reps=reps, calls=calls)
    res = {}
    if "hist" in only:
        g = bbb.CLTGRNG(bbb.LUTOPT.shipped(256))
        out = torch.zeros(256, dtype=torch.uint64, device=DEV)
        pos = [16]

        def run():
            for _ in range(calls):
                g.histogram(n, first_step=pos[0], out=out)
                pos[0] += n
        med, lo, hi = timed(run, reps)
        res["hist"] = med / calls
        line(case="hist_calls", n=n, calls=calls, ms_per_call=med / calls, ms_min=lo / calls, ms_max=hi / calls,
             gsamples_per_s=n / (med / calls) / 1e6)
        # ONE call over ever longer ranges (the library's own chunks of 2^30, every next one announced): what a call costs at
        # its ends -- the first chunk's start states derived in line, the last mover alone on the machine -- against the steady state
        for chunks in ((4,) if args.quick else (4, 32, 256)):
            big = chunks << 30
            med, lo, hi = timed(lambda: g.histogram(big, first_step=16, out=out), max(2, reps // 2))
            res["hist_one_call"] = med / (big / 1e9)
            line(case="hist_one_call", chunks_of_2p30=chunks, n=big, ms=med, ms_per_1e9=med / (big / 1e9), ms_per_1e9_min=lo / (big / 1e9),
                 ms_per_1e9_max=hi / (big / 1e9), gsamples_per_s=big / med / 1e6)
        del g
    if "stream" in only or "baseline" in only:
        buf = torch.empty(n, dtype=torch.int8, device=DEV)
        with bbb.CLTGRNG(bbb.LUTOPT.shipped(256)).stream(n, first_step=16) as st:
            def reads():
                for _ in range(calls):
                    st.next(out=buf)
            if "stream" in only:
                med, lo, hi = timed(reads, reps)
                res["stream"] = med / calls
                line(case="stream_next", n=n, calls=calls, ms_per_call=med / calls, ms_min=lo / calls, ms_max=hi / calls,
                     gsamples_per_s=n / (med / calls) / 1e6)
            if "baseline" in only:
                u8 = buf.view(torch.uint8)
                med, lo, hi = timed(lambda: torch.bincount(u8, minlength=256), reps)
                res["bincount"] = med
                line(case="bincount_alone", n=n, ms=med, ms_min=lo, ms_max=hi)
                try:
                    med, lo, hi = timed(lambda: torch.histc(buf.float(), bins=256, min=-128, max=127), 2)
                    res["histc"] = med
                    line(case="histc_alone", n=n, ms=med, ms_min=lo, ms_max=hi)
                except RuntimeError as e:          # (the float copy of 10^9 samples takes 4 GB)
                    line(case="histc_alone", n=n, error=str(e)[:120])
                count = "bincount" if res.get("histc", float("inf")) >= res["bincount"] else "histc"

                def both():
                    for _ in range(calls):
                        st.next(out=buf)
                        if count == "bincount":
                            torch.bincount(u8, minlength=256)
                        else:
                            torch.histc(buf.float(), bins=256, min=-128, max=127)
                med, lo, hi = timed(both, reps)
                res["baseline"] = med / calls
                line(case="stream_next_then_count", count=count, n=n, calls=calls, ms_per_call=med / calls, ms_min=lo / calls,
                     ms_max=hi / calls)
        del buf
    if "hist" in res and "baseline" in res:
        line(case="condition", what="hist faster than stream_next + count", hist_ms=res["hist"], baseline_ms=res["baseline"],
             speedup=res["baseline"] / res["hist"], verdict="met" if res["hist"] < res["baseline"] else "missed")
    if "hist" in res and "stream" in res:
        r = res["hist"] / res["stream"]
        line(case="estimate", what="hist within 1.3x of the bare stream step", ratio=r, ratio_longest_call=res["hist_one_call"] / res["stream"],
             verdict="met" if r <= 1.3 else "missed")
    if "eval" in only:
        ne = (1 << 28) if args.quick else int(args.eval)
        u = bbb.LUTOPT.shipped(256)
        grngstats.evaluate(u, 1 << 26)          # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = grngstats.evaluate(u, ne, first_step=16)
        wall = time.perf_counter() - t0
        line(case="evaluate", nsamples=ne, wall_s=wall, ms_per_1e9=wall * 1e3 / (ne / 1e9), chi2=ev.chi2.statistic, dof=ev.chi2.dof, p=ev.chi2.p_value, method=ev.chi2.method,
             mean=ev.moments.mean, variance=ev.moments.variance, skewness=ev.moments.skewness, excess_kurtosis=ev.moments.excess_kurtosis,
             min_sample=min(b for b, v in enumerate(ev.hist) if v) - 128, max_sample=max(b for b, v in enumerate(ev.hist) if v) - 128)
        print(str(ev), file=sys.stderr, flush=True)
        if LOG:
            LOG.write(str(ev) + "\n")
    if LOG:
        LOG.close()


if __name__ == "__main__":
    main()
