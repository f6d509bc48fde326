#!/usr/bin/env python3
"""Eye diagram and bathtub timings: one JSON line per measurement.

  python3 profiles/eye_bench.py [--n 1e9] [--reps 10] [--quick]

  capture   bbb_eye_accumulate_i16 over an int16 buffer of n samples in HBM (noisy eye, noise-free eye, constant buffer):
            median ms of `reps` calls (hipEvents on the stream) and the read rate 2 n B / time
  tx        bbb_tx_eye_run over n samples (one object, chunk 2^24 / 2^26 / 2^28) against a bare bbb_tx_fill_i16 of the same
            range (TX.generate into a preallocated buffer) and against the manual path it replaces: fill + 8 x
            (bbb_rx_slice + bbb_prbs_check) + torch.bincount
--quick: n = 2^28 and 3 repetitions (for the profiler runs)."""
import argparse
import json
import statistics
import sys
import pathlib

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402
from basebandboard_amd.eye import BIT_SAMPLE0, EyeConfig, TxEye  # noqa: E402

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
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    n, reps = (1 << 28, 3) if args.quick else (int(args.n), args.reps)
    n -= n % 8
    # ramp the clock out of its idle state (profiles/README.md, round 3)
    ramp = bbb.TX(31, 1, 0, 16, 1, 8, device=0)
    buf = torch.empty(n, dtype=torch.int16, device=DEV)
    for _ in range(20):
        ramp.generate(n, out=buf, stream_on=False)
    torch.cuda.synchronize()

    eye = EyeConfig(ncols=64, shift=4, col_origin=BIT_SAMPLE0)
    rx = bbb.RX(31, 8, 0)
    hist = torch.zeros((256, 64), dtype=torch.uint64, device=DEV)
    cases = {
        "noisy": lambda: bbb.TX(31, 1, 0, 16, 1, 8, device=0).generate(n, out=buf, stream_on=False),
        "noise_free": lambda: bbb.TX(31, 1, 0, 16, 0, 0, device=0).generate(n, out=buf, stream_on=False),
        "constant": lambda: buf.fill_(77),
    }
    for name, make in cases.items():
        make()
        torch.cuda.synchronize()
        med, lo, hi = timed(lambda: rx.eye(buf, eye=eye, hist=hist), reps)
        print(json.dumps(dict(what="capture_eye", case=name, n=n, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                              read_tb_s=round(2 * n / med / 1e9, 3))), flush=True)

    # the transmitter side against a bare fill and against the manual path
    tx = bbb.TX(31, 1, 0, 16, 1, 8, device=0)
    med_fill, lo, hi = timed(lambda: tx.generate(n, out=buf, stream_on=False), reps)
    print(json.dumps(dict(what="tx_fill_bare", n=n, ms=round(med_fill, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))), flush=True)
    tub = torch.zeros((8, 2), dtype=torch.uint64, device=DEV)
    best = None
    for chunk in (1 << 24, 1 << 26, 1 << 28):
        with TxEye(tx, eye, chunk_samples=chunk) as e:
            med, lo, hi = timed(lambda: e.run(n, 0, hist, tub), reps)
            med_h, _, _ = timed(lambda: e.run(n, 0, hist, None, want_bathtub=False), reps)
            med_t, _, _ = timed(lambda: e.run(n, 0, None, tub, want_hist=False), reps)
        print(json.dumps(dict(what="tx_eye_run", chunk=chunk, n=n, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                              ratio_to_fill=round(med / med_fill, 3), hist_only_ms=round(med_h, 4), bathtub_only_ms=round(med_t, 4))),
              flush=True)
        if chunk == 1 << 26:
            best = med

    def manual():
        x = tx.generate(n, out=buf, stream_on=False)
        out = []
        for p in range(8):
            out.append(rx.count_errors(x, first_sample=BIT_SAMPLE0 + p, stride=8))
        xi = x.to(torch.int32)
        rows = 127 - torch.clamp(xi >> 4, -128, 127)
        cols = (torch.arange(n, device=DEV, dtype=torch.int64) - BIT_SAMPLE0) % 64
        return out, torch.bincount(rows.to(torch.int64) * 64 + cols, minlength=256 * 64)
    med_m, lo, hi = timed(manual, max(2, reps // 3), warm=1)
    print(json.dumps(dict(what="manual_path", n=n, ms=round(med_m, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                          tx_eye_speedup=round(med_m / best, 2))), flush=True)


if __name__ == "__main__":
    main()
