#!/usr/bin/env python3
"""Convolutional codec timings: one JSON line per measurement.

  timeout 900 python3 profiles/conv_bench.py [--log2n 27] [--reps 5] [--quick]

n = 2^27 resident steps of random data, encoded on the GPU by (7, 5) (K = 3) and (0171, 0133) (K = 7) at rate 1/2 and
punctured to 3/4, sent as +-64 plus Gaussian noise of sigma 40, decoded from the int16 values (soft) and from their signs
packed as RX.slice packs them (hard) under the default geometry (B, W, D = 192, 64, 64).  Every decoder line carries the
errors left, the estimate of DESIGN.md 25 written before the first run (cycles per decided step and SIMD at 1024 SIMDs and
2.4 GHz) and the ratio to it.  In the same session bbb_mlse_run at memory 4 and one sample per symbol over n symbols is the
yardstick, and the encoder is timed.  Medians of `reps` calls (hipEvents on the stream) after a warm-up call.
--quick: n = 2^24, 2 repetitions."""
import argparse
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import basebandboard_amd as bbb  # noqa: E402
from dfe_bench import line, timed  # noqa: E402

SIMD_RATE = 1024 * 2.4e9   # SIMD cycles per second
CYCLES = {7: 325.0, 3: 25.0}   # per decided step and SIMD


def estimate_ms(nsteps, K):
    return CYCLES[K] * nsteps / SIMD_RATE * 1e3


def values_of(tx, ntx, sigma=40.0):
    """int16 received values of packed transmitted bits: +-64 plus rounded Gaussian noise."""
    b = tx.view(torch.uint8)
    out = torch.empty(b.numel() * 8, dtype=torch.int16, device=tx.device)
    step = 1 << 24
    for lo in range(0, b.numel(), step):
        part = b[lo:lo + step]
        bits = ((part.to(torch.int16)[:, None] >> torch.arange(8, device=tx.device, dtype=torch.int16)) & 1).reshape(-1)
        noise = torch.randn(bits.numel(), device=tx.device).mul_(sigma).round_().to(torch.int16)
        out[8 * lo:8 * (lo + part.numel())] = bits * 128 - 64 + noise
    return out[:ntx]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    n, reps = (1 << 24, 2) if args.quick else (1 << args.log2n, args.reps)
    torch.manual_seed(25)
    dev = torch.device("cuda", 0)
    data = torch.randint(-(1 << 62), 1 << 62, (n // 64,), dtype=torch.int64, device=dev)
    x = torch.randint(-1000, 1000, (n,), dtype=torch.int16, device=dev)
    m = bbb.MLSE(bbb.FIR([1]), [800, 560, 15, -8, 3], 1)
    ref, lo, hi = timed(lambda: m.slice(x), reps)
    line(case="mlse_mem4_spb1", n=n, ms=ref, ms_min=lo, ms_max=hi, gsym_per_s=n / ref / 1e6)
    del x
    rx = bbb.RX(7, 1, 0)
    for K, gens in ((3, (7, 5)), (7, (0o171, 0o133))):
        for punct in (None, "3/4"):
            cc = bbb.ConvCode(K, gens, punct)
            rate = "1/2" if punct is None else punct
            med, lo, hi = timed(lambda: cc.encode(data, n), reps)
            line(case="conv_encode", K=K, rate=rate, n=n, ms=med, ms_min=lo, ms_max=hi, gbit_in_per_s=n / med / 1e6)
            tx, ntx = cc.encode(data, n)
            soft = values_of(tx, ntx)
            hard, nh = rx.slice(soft)
            for name, call in (("soft", lambda: cc.decode(soft)), ("hard", lambda: cc.decode(hard, hard=True, nbits=nh))):
                med, lo, hi = timed(call, reps)
                bits, nd = call()
                errors = int(sum(bin(v & 0xFFFFFFFFFFFFFFFF).count("1") for v in (bits[:4096] ^ data[:4096]).cpu().tolist()))
                est = estimate_ms(n, K)
                line(case="conv_decode", K=K, rate=rate, values=name, n=n, ms=med, ms_min=lo, ms_max=hi, gbit_per_s=n / med / 1e6,
                     estimate_ms=est, measured_over_estimate=med / est, ratio_to_mlse=med / ref, errors_in_first_262144=errors)
            del soft, hard, tx


if __name__ == "__main__":
    main()
