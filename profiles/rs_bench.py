#!/usr/bin/env python3
"""Reed-Solomon codec timings: one JSON line per measurement.

  timeout 900 python3 profiles/rs_bench.py [--log2n 22] [--reps 5] [--quick]

2^22 codewords of CCSDS (255, 223) at depth 4 (2^20 frames, 1.07 GB coded) of random data, encoded on the GPU (timed), then
decoded clean, with symbol errors at a rate of 1e-3 and with 8 wrong symbols in every codeword.  Every line carries the
estimate of DESIGN.md 26 written before the first run (cycles per codeword and SIMD at 1024 SIMDs and 2.4 GHz) and the ratio
to it, and the decoder's own statistics.  Then the chain's condition, in the same session: the frames whose bits make 2^27
steps of (0171, 0133) at rate 1/2, sent as +-64 plus Gaussian noise of sigma 42 (the closed loop of tests/rs_model.py), hard
decisions, bbb_conv_decode timed, and bbb_rs_decode of the bytes it produced timed: the outer decoder must take less.
Medians of `reps` calls (hipEvents on the stream) after a warm-up call.  --quick: 2^18 codewords, 2^24 steps, 2 repetitions."""
import argparse
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import basebandboard_amd as bbb  # noqa: E402
from conv_bench import values_of  # noqa: E402
from dfe_bench import line, timed  # noqa: E402

SIMD_RATE = 1024 * 2.4e9   # SIMD cycles per second
CYCLES = dict(clean=4800.0, ser=6600.0, eight=11300.0, encode=4600.0)   # per codeword and SIMD


def estimate_ms(ncw, case):
    return CYCLES[case] * ncw / SIMD_RATE * 1e3


def decode_line(rs, coded, case, ncw, reps, **more):
    med, lo, hi = timed(lambda: rs.decode(coded), reps)
    fresh = bbb.ReedSolomon.ccsds(rs.depth)
    fresh.decode(coded)
    est = estimate_ms(ncw, case)
    line(case="rs_decode_" + case, n=ncw, ms=med, ms_min=lo, ms_max=hi, mcodewords_per_s=ncw / med / 1e3,
         gbyte_in_per_s=coded.numel() / med / 1e6, estimate_ms=est, measured_over_estimate=med / est, **fresh.stats(), **more)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    ncw, nsteps, reps = (1 << 18, 1 << 24, 2) if args.quick else (1 << args.log2n, 1 << 27, args.reps)
    torch.manual_seed(26)
    dev = torch.device("cuda", 0)
    rs = bbb.ReedSolomon.ccsds(4)
    nf = ncw // 4
    data = torch.randint(0, 256, (nf * rs.data_bytes,), dtype=torch.uint8, device=dev)
    med, lo, hi = timed(lambda: rs.encode(data), reps)
    est = estimate_ms(ncw, "encode")
    line(case="rs_encode", codewords=ncw, ms=med, ms_min=lo, ms_max=hi, mcodewords_per_s=ncw / med / 1e3, estimate_ms=est, measured_over_estimate=med / est)
    coded = rs.encode(data)
    del data
    decode_line(rs, coded, "clean", ncw, reps)
    # symbol errors at a rate of 1e-3: a nonzero value XORed in, chunk by chunk
    bad = coded.clone()
    step = 1 << 26
    for lo_ in range(0, bad.numel(), step):
        part = bad[lo_:lo_ + step]
        hit = torch.rand(part.numel(), device=dev) < 1e-3
        part ^= hit.to(torch.uint8) * torch.randint(1, 256, (part.numel(),), dtype=torch.uint8, device=dev)
    decode_line(rs, bad, "ser", ncw, reps, ser=1e-3)
    # eight wrong symbols in every codeword: symbols (base + 31 j) mod 255, j < 8, of codeword w (frame w // 4, codeword w % 4)
    bad.copy_(coded)
    w = torch.arange(ncw, device=dev, dtype=torch.int64)
    base = torch.randint(0, 255, (ncw,), device=dev, dtype=torch.int64)
    for j in range(8):
        idx = (w // 4) * rs.frame_bytes + ((base + 31 * j) % 255) * 4 + w % 4
        bad[idx] ^= torch.randint(1, 256, (ncw,), dtype=torch.uint8, device=dev)
    decode_line(rs, bad, "eight", ncw, reps)
    del bad, coded, w, base, idx
    # the chain: the Viterbi decoder's bytes at the closed loop's error rate
    inner = bbb.ConvCode(7, (0o171, 0o133))
    cat = bbb.Concatenated(bbb.ReedSolomon.ccsds(4), inner)
    nfc = nsteps // (8 * rs.frame_bytes)
    data = torch.randint(0, 256, (nfc * rs.data_bytes,), dtype=torch.uint8, device=dev)
    tx, ntx = cat.encode(data)
    soft = values_of(tx, ntx, sigma=42.0)
    hard, nh = bbb.RX(7, 1, 0).slice(soft)
    del soft, tx
    vit_ms, lo, hi = timed(lambda: inner.decode(hard, hard=True, nbits=nh), reps)
    line(case="chain_conv_decode", K=7, steps=ntx // 2, ms=vit_ms, ms_min=lo, ms_max=hi)
    bits, nd = inner.decode(hard, hard=True, nbits=nh)
    got = bits.view(torch.uint8)[:nfc * rs.frame_bytes]
    rs_ms = decode_line(cat.outer, got, "eight", nfc * 4, reps, chain=True, viterbi_ms=vit_ms)
    out, _ = bbb.ReedSolomon.ccsds(4).decode(got)
    line(case="chain", steps=ntx // 2, conv_decode_ms=vit_ms, rs_decode_ms=rs_ms, rs_over_conv=rs_ms / vit_ms, met=bool(rs_ms < vit_ms),
         data_bytes_wrong=int((out != data).sum()))


if __name__ == "__main__":
    main()
