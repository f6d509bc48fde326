#!/usr/bin/env python3
"""Digital down-converter timings: one JSON line per measurement.

  timeout 900 python3 profiles/ddc_bench.py [--log2n 28] [--reps 5] [--quick]

n = 2^28 resident int16 samples at fcw = 0x5A5A5A, for (64 taps, decim 16), (256 taps, decim 64) and (64 taps, decim 1):
  ddc          bbb_ddc_run to IQ16 and to POLAR
  fir          baseline (a): ONE bbb_fir_filter with the same taps and decim to int16.  The converter does two filters'
               arithmetic on one read; `ratio_to_fir` is its time over this one's, the estimate being "at most about 2"
  composition  baseline (b), what a user writes without the converter: the oscillator's ROM gathered in torch, multiply,
               shift, two FIR.filter calls.  `fused_is_faster` must be true in every case
The composition's I and Q are compared with the fused call's at the timed size before anything is timed.  Medians of `reps`
calls (hipEvents on the stream) after a warm-up call.  --quick: n = 2^24, 2 repetitions (profiler runs)."""
import argparse
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402

DEV = torch.device("cuda", 0)
FCW, PA0, SHIFT = 0x5A5A5A, 0xABCDEF, 12
MASK = (1 << 24) - 1


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


def taps(n):
    """n taps of both signs, sum |h| = 65535 - (65535 mod n)."""
    return [(65535 // n) * (1 if i % 3 else -1) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    n, reps = (1 << 24, 2) if args.quick else (1 << args.log2n, args.reps)
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    x = torch.randint(-2048, 2048, (n,), dtype=torch.int16, device=DEV, generator=g)
    rom = torch.from_numpy(bbb.NCO.rom_table()).to(DEV).to(torch.int32)
    mi, mq = torch.empty(n, dtype=torch.int16, device=DEV), torch.empty(n, dtype=torch.int16, device=DEV)

    def mix():
        # int32 products wrap modulo 2^32, which leaves the low 24 bits exact
        adr = ((torch.arange(n, dtype=torch.int32, device=DEV) * FCW + PA0) & MASK) >> 14
        xi = x.to(torch.int32)
        mi.copy_((xi * rom[(adr + 256) & 1023]) >> 15)
        mq.copy_((xi * -rom[adr]) >> 15)

    for ntaps, decim in ((64, 16), (256, 64), (64, 1)):
        f = bbb.FIR(taps(ntaps), shift=SHIFT)
        d = bbb.DDC(FCW, f, decim=decim, pa0=PA0)
        nout = (n + decim - 1) // decim
        out = torch.empty((nout, 2), dtype=torch.int16, device=DEV)
        yi, yq = torch.empty(nout, dtype=torch.int16, device=DEV), torch.empty(nout, dtype=torch.int16, device=DEV)

        def composition():
            mix()
            f.filter(mi, decim=decim, out=yi)
            f.filter(mq, decim=decim, out=yq)

        composition()
        d.iq(x, out=out)
        assert torch.equal(out[:, 0], yi) and torch.equal(out[:, 1], yq), "the fused call and the composition differ"
        fir_ms, lo, hi = timed(lambda: f.filter(x, decim=decim, out=yi), reps)
        line(case="fir", ntaps=ntaps, decim=decim, n=n, ms=fir_ms, ms_min=lo, ms_max=hi)
        comp_ms, lo, hi = timed(composition, reps)
        line(case="composition", ntaps=ntaps, decim=decim, n=n, ms=comp_ms, ms_min=lo, ms_max=hi)
        for name, fn in (("iq16", lambda: d.iq(x, out=out)), ("polar", lambda: d.polar(x, out=out))):
            med, lo, hi = timed(fn, reps)
            line(case="ddc", mode=name, ntaps=ntaps, decim=decim, n=n, ms=med, ms_min=lo, ms_max=hi, gbps_read=2 * n / med / 1e6,
                 gmac_per_s=2 * nout * ntaps / med / 1e6, ratio_to_fir=med / fir_ms, within_2x_of_fir=med <= 2 * fir_ms,
                 fused_is_faster=med < comp_ms)
        del out, yi, yq


if __name__ == "__main__":
    main()
