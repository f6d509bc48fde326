#!/usr/bin/env python3
"""Filtered-link timings: one JSON line per measurement, all in one session.

  python3 profiles/link_bench.py [--n 1e9] [--reps 5] [--quick]

  eye_bathtub    one bathtub-only bbb_tx_eye_run over n samples: the UNFILTERED bathtub of one setting, chunk 2^26
  composition    the materialising road to a filtered eye: TX.generate of a 2^26 chunk (with the filter's history in front)
                 -> FIR.filter -> capture_eye, chunk by chunk over n samples.  It gives the histogram only: the capture side
                 has no bathtub
  link_tub       bbb_link_sweep_run, one setting, taps {1, 1, 1, 1}, bathtub only
  link_hist      the same with the histogram (64 columns)
  link_tub_64    bathtub only behind a 64-tap matched filter
  link16         16 noise_var settings behind the moving average, bathtub only: the noise stream is generated once
Medians of `reps` calls (hipEvents on the stream) after ramp fills.  --quick: n = 2^28, 2 repetitions (profiler runs)."""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402
from basebandboard_amd.eye import BIT_SAMPLE0, EyeConfig, TxEye, capture_eye  # noqa: E402
from basebandboard_amd.txsweep import TxSetting  # noqa: E402

DEV = torch.device("cuda", 0)
CHUNK = 1 << 26


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
    eye = EyeConfig(col_origin=BIT_SAMPLE0)
    ma = bbb.FIR.moving_average()
    tub = torch.zeros((8, 2), dtype=torch.uint64, device=DEV)
    with TxEye(tx, eye, chunk_samples=CHUNK) as e:
        med_eye, lo, hi = timed(lambda: e.run(n, 0, None, tub, want_hist=False), reps)
    line(what="eye_bathtub", n=n, settings=1, ms=med_eye, ms_min=lo, ms_max=hi)

    delay = 2
    wave = torch.empty(CHUNK + 16, dtype=torch.int16, device=DEV)
    z = torch.empty(CHUNK + 16, dtype=torch.int16, device=DEV)
    hist = torch.zeros((256, 64), dtype=torch.uint64, device=DEV)

    def composition():
        # eight samples of history in front of every chunk keep the filter's input 16-byte aligned (its wide loads); the
        # first chunk starts at sample 0 and is filtered from there
        for off in range(0, n, CHUNK):
            m = min(CHUNK, n - off)
            lo_s = max(0, off + delay - 8)
            before = off + delay - lo_s
            tx.generate(m + before, first_sample=lo_s, out=wave)
            if before == 8:
                zz = ma.filter(wave[:m + 8], nbefore=8, out=z[:m])
            else:
                zz = ma.filter(wave[:m + before], out=z[:m + before])[before:]
            capture_eye(zz, first_sample=off, eye=eye, hist=hist)

    med_comp, lo, hi = timed(composition, reps)
    line(what="composition", chunk=CHUNK, n=n, settings=1, ms=med_comp, ms_min=lo, ms_max=hi, ratio_to_one_eye=med_comp / med_eye)

    own = [TxSetting(noise_var=8)]
    with bbb.LinkSweep(tx, own, ma, delay, chunk_samples=CHUNK) as s:
        cnt = s.run(1 << 20)
        med, lo, hi = timed(lambda: s.run(n, 0, cnt), reps)
    line(what="link_tub", chunk=CHUNK, n=n, settings=1, taps=4, ms=med, ms_min=lo, ms_max=hi, ratio_to_one_eye=med / med_eye,
         speedup_over_composition=med_comp / med)
    with bbb.LinkSweep(tx, own, ma, delay, eye, chunk_samples=CHUNK) as s:
        cnt, h = s.run(1 << 20)
        med, lo, hi = timed(lambda: s.run(n, 0, cnt, h), reps)
    line(what="link_hist", chunk=CHUNK, n=n, settings=1, taps=4, ms=med, ms_min=lo, ms_max=hi, ratio_to_one_eye=med / med_eye,
         speedup_over_composition=med_comp / med)
    sh = tx.prbs_shaper
    with bbb.LinkSweep(tx, own, bbb.FIR.matched(sh.coefficients[sh.setsel]), chunk_samples=CHUNK) as s:
        cnt = s.run(1 << 20)
        med, lo, hi = timed(lambda: s.run(n, 0, cnt), reps)
    line(what="link_tub_64", chunk=CHUNK, n=n, settings=1, taps=64, ms=med, ms_min=lo, ms_max=hi, ratio_to_one_eye=med / med_eye)
    with bbb.LinkSweep(tx, [TxSetting(noise_var=v) for v in range(16)], ma, delay, chunk_samples=CHUNK) as s:
        cnt = s.run(1 << 20)
        med, lo, hi = timed(lambda: s.run(n, 0, cnt), max(2, reps // 2))
    line(what="link16", chunk=CHUNK, n=n, settings=16, taps=4, ms=med, ms_min=lo, ms_max=hi, ratio_to_one_eye=med / med_eye,
         gsetting_samples_per_s=16 * n / med / 1e6)


if __name__ == "__main__":
    main()
