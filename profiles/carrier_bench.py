#!/usr/bin/env python3
"""Carrier recovery timings: one JSON line per measurement.

  timeout -k 10 900 python3 profiles/carrier_bench.py [--log2n 28] [--reps 5] [--quick]

The record is n = 2^28 resident (I, Q) pairs of int16: a BPSK vector of length 8000 that turns once per 2^15 pairs, one data
bit per pair, plus Gaussian noise of sigma 2000 on either axis (torch's generator).  bbb_carrier_run at L 32: the pairs turned
back (CarrierRecovery.derotate), the decisions alone (slice) and every output (recover).  Measured against, in the same
process:
  (a) bbb_ddc_run, IQ16, one tap, decim 1 over 2^28 samples: the stage in front, a reference point only;
  (b) the same result through torch: block sums by reshape, the CORDIC's integer steps in place of atan2, the unwrap as a
      cumulative sum of the flags, a gather from the ROM and a multiply.  Its pairs are compared with the fused call's first.
Then chunk_blocks 64, 256, 1024 (the default) and 4096.  The kernels' shares of a call come from a kernel trace of this script
(profiles/README.md has the command).  Medians of `reps` calls (hipEvents on the stream) after a warm-up call.
--quick: n = 2^24, 2 repetitions."""
import argparse
import ctypes as C
import json
import math
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402
from basebandboard_amd import _lib  # noqa: E402

DEV = torch.device("cuda", 0)
ANGLES = [536870912, 316933406, 167458907, 85004756, 42667331, 21354465, 10679838, 5340245, 2670163, 1335087, 667544, 333772, 166886, 83443,
          41722, 20861]


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
    x = torch.empty((n, 2), dtype=torch.int16, device=DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(1)
    step = 1 << 24
    for a in range(0, n, step):
        b = min(n, a + step)
        k = torch.arange(a, b, device=DEV, dtype=torch.float64)
        ang = (k * (2 * math.pi / 32768) + 0.3).to(torch.float32)
        d = (torch.randint(0, 2, (b - a,), device=DEV, generator=g) * 2 - 1).to(torch.float32) * 8000
        x[a:b, 0] = (d * torch.cos(ang) + torch.randn(b - a, device=DEV, generator=g) * 2000).round().clamp(-32768, 32767).to(torch.int16)
        x[a:b, 1] = (d * torch.sin(ang) + torch.randn(b - a, device=DEV, generator=g) * 2000).round().clamp(-32768, 32767).to(torch.int16)
    return x


def torch_carrier(pairs, L, init, rom):
    """bbb_carrier_run's pairs through torch, whole blocks only, out of reset."""
    nb = pairs.shape[0] // L
    x = pairs[:nb * L].to(torch.int64).view(nb, L, 2)
    i, q = x[:, :, 0], x[:, :, 1]
    sr, si = (i * i - q * q).sum(1), 2 * (i * q).sum(1)
    m = torch.maximum(sr.abs(), si.abs())
    bl = torch.zeros_like(m)
    for k in (32, 16, 8, 4, 2, 1):                       # the bit length by halving
        big = (m >> (bl + k - 1)) != 0
        bl = torch.where(big, bl + k, bl)
    s = (bl - 15).clamp(min=0)
    a, b = sr >> s, si >> s
    neg = a < 0
    X, Y = torch.where(neg, -a, a) << 14, torch.where(neg, -b, b) << 14
    Z = torch.where(neg, 1 << 31, 0)
    for k in range(16):
        d = Y >= 0
        X, Y = torch.where(d, X + (Y >> k), X - (Y >> k)), torch.where(d, Y - (X >> k), Y + (X >> k))
        Z = (Z + torch.where(d, ANGLES[k], -ANGLES[k])) & 0xFFFFFFFF
    th = torch.where((a == 0) & (b == 0), 0, ((Z + (1 << 15)) >> 16) & 0xFFFF)
    h = th >> 1
    hp = torch.cat([torch.tensor([init & 0x7FFF], device=h.device), h[:-1]])
    dd = (h - hp) & 0xFFFF
    f = ((dd >= 16384) & (dd < 49152)).to(torch.int64)
    est = h + 32768 * ((init >> 15) ^ (torch.cumsum(f, 0) & 1))
    adr = est >> 6
    c, sn = rom[(adr + 256) & 1023][:, None], rom[adr][:, None]
    io = ((i * c + q * sn) >> 15).clamp(-32768, 32767)
    qo = ((q * c - i * sn) >> 15).clamp(-32768, 32767)
    return torch.stack([io, qo], dim=2).view(nb * L, 2).to(torch.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    n, reps = (1 << 24, 2) if args.quick else (1 << args.log2n, args.reps)
    L, init = 32, 16384
    x = record(n)
    r16 = (C.c_int16 * 1024)()
    _lib.check(_lib.lib().bbb_nco_rom(r16), "bbb_nco_rom")
    rom = torch.tensor(list(r16), dtype=torch.int64, device=DEV)
    # (a) the stage in front
    ddc = bbb.DDC(1 << 20, [1])
    ref, lo, hi = timed(lambda: ddc.iq(x.view(-1)[:n]), reps)
    line(case="ddc_iq16", decim=1, ntaps=1, n=n, ms=ref, ms_min=lo, ms_max=hi, gbytes_per_s=6 * n / ref / 1e6)
    # the fused call; bytes: the pairs read twice and what the outputs take
    cr = bbb.CarrierRecovery(L, init)
    fused = None
    for case, fn, nbytes in (("derotate", lambda: cr.derotate(x), 12), ("slice", lambda: cr.slice(x), 8.125), ("recover", lambda: cr.recover(x), 14.125)):
        med, lo, hi = timed(fn, reps)
        line(case="carrier_" + case, block_pairs=L, n=n, ms=med, ms_min=lo, ms_max=hi, ratio_to_ddc=med / ref, gbytes_per_s=nbytes * n / med / 1e6)
        fused = med if case == "derotate" else fused
    st = cr.stats()
    line(case="carrier_stats", blocks_per_call=st["blocks"] // (3 * (reps + 1)), flips_share=st["flips"] / st["blocks"], carrier_offset_ppm=cr.carrier_offset() * 1e6,
         ideal_offset_ppm=1e6 / 32768)
    # (b) the same pairs through torch
    same = bool(torch.equal(torch_carrier(x, L, init, rom), bbb.CarrierRecovery(L, init).derotate(x)))
    med, lo, hi = timed(lambda: torch_carrier(x, L, init, rom), max(2, reps // 2))
    line(case="torch_carrier", n=n, ms=med, ms_min=lo, ms_max=hi, equal_to_fused=same, fused_speedup=med / fused)
    missed = not same or med <= fused
    for chunk in (64, 256, 1024, 4096):
        c2 = bbb.CarrierRecovery(L, init, chunk_blocks=chunk)
        med, lo, hi = timed(lambda: c2.derotate(x), reps)
        line(case="carrier_chunk", chunk_blocks=chunk, n=n, ms=med, ms_min=lo, ms_max=hi)
    if missed:
        print("CONDITION MISSED: the fused call must give torch's pairs and be faster", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
