#!/usr/bin/env python3
"""LDPC codec timings: one JSON line per measurement.

  timeout -k 10 900 python3 profiles/ldpc_bench.py [--log2n 16] [--reps 5] [--quick]

2^16 codewords of array(127, 4, 16) (n 2032, rate 3/4) of random data, encoded on the GPU (f, timed), sent as +-64 plus rounded
Gaussian noise, and decoded with max_iter 20, norm 12: (a) at sigma 32, (b) clean, (c) at sigma 40, each in ms, codewords/s and
information Gbit/s with the decoder's own statistics; `ldpc_estimate` sets (a) against the estimate of DESIGN.md 29, which was
written before the first run.  (d) the same integer rule restated in batched torch ops over the same tensor (every message goes through HBM
once per layer), its data bits and iteration counts checked equal to bbb_ldpc_decode's first: the fused decoder must be
faster, and the script exits with 1 where it is not or where the two differ.  (e) bbb_conv_decode at K = 7, rate 3/4, soft values,
over the same number of information bits, in the same process.  Medians of `reps` calls (events on the stream) after a warm-up
call.  --quick: 2^12 codewords, 2 repetitions."""
import argparse
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import basebandboard_amd as bbb  # noqa: E402
from conv_bench import values_of  # noqa: E402
from dfe_bench import line, timed  # noqa: E402

ESTIMATE_MS_2_16 = 1.3     # 2^16 codewords at sigma 32, written before the first run


def torch_decode(ld, vals):
    """The definition of include/bbb.h in batched torch ops: (data bits [ncw, k] bool, iters [ncw])."""
    dev = vals.device
    Z, n = ld.Z, ld.n
    r = torch.arange(Z, device=dev)
    V = [torch.stack([c * Z + (r + s) % Z for c, s in enumerate(row) if s >= 0]) for row in ld.base]       # [deg, Z]
    P = vals.view(-1, n).to(torch.int32).clamp_(-32767, 32767)
    ncw = P.shape[0]
    R = [torch.zeros((ncw,) + tuple(v.shape), dtype=torch.int32, device=dev) for v in V]

    def unsatisfied():
        bad = torch.zeros(ncw, dtype=torch.bool, device=dev)
        for v in V:
            bad |= ((P[:, v] > 0).sum(dim=1) & 1).any(dim=1)
        return bad
    run = unsatisfied()
    iters = torch.where(run, 255, 0)
    for it in range(ld.max_iter):
        if not bool(run.any()):
            break
        upd = run[:, None, None]
        for j, v in enumerate(V):
            Pj = P[:, v]
            Q = (Pj - R[j]).clamp_(-32767, 32767)
            b = Q > 0
            S = (b.sum(dim=1) & 1).bool()
            A = Q.abs()
            m1 = A.amin(dim=1)
            e = torch.arange(v.shape[0], device=dev)[None, :, None]
            i1 = torch.where(A == m1[:, None, :], e, v.shape[0]).amin(dim=1)
            first = e == i1[:, None, :]
            m2 = torch.where(first, 1 << 20, A).amin(dim=1)
            a = (torch.where(first, m2[:, None, :], m1[:, None, :]) * ld.norm) >> 4
            Rn = torch.where(S[:, None, :] ^ b, a, -a).to(torch.int32)
            R[j] = torch.where(upd, Rn, R[j])
            P[:, v.reshape(-1)] = torch.where(upd, (Q + Rn).clamp_(-32767, 32767), Pj).reshape(ncw, -1)
        ok = run & ~unsatisfied()
        iters[ok] = it + 1
        run &= ~ok
    return P[:, :ld.k] > 0, iters


def unpack(words, nbits):
    sh = torch.arange(64, dtype=torch.int64, device=words.device)
    return ((words[:, None] >> sh) & 1).reshape(-1)[:nbits].bool()


def decode_line(ld, vals, case, reps, **more):
    ncw = vals.numel() // ld.n
    med, lo, hi = timed(lambda: ld.decode(vals), reps)
    fresh = bbb.LDPC(ld.base, ld.Z, ld.max_iter, ld.norm, ld.hard_mag)
    fresh.decode(vals)
    line(case="ldpc_decode_" + case, ms=med, ms_min=lo, ms_max=hi, mcodewords_per_s=ncw / med / 1e3,
         info_gbit_per_s=ncw * ld.k / med / 1e6, **fresh.stats(), **more)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    ncw, reps = (1 << 12, 2) if args.quick else (1 << args.log2n, args.reps)
    torch.manual_seed(29)
    dev = torch.device("cuda", 0)
    ld = bbb.LDPC.array(127, 4, 16)
    data = torch.randint(-(1 << 62), 1 << 62, ((ncw * ld.k + 63) // 64,), dtype=torch.int64, device=dev)
    med, lo, hi = timed(lambda: ld.encode(data, ncw), reps)
    line(case="ldpc_encode", codewords=ncw, ms=med, ms_min=lo, ms_max=hi, mcodewords_per_s=ncw / med / 1e3, info_gbit_per_s=ncw * ld.k / med / 1e6)
    tx, ntx = ld.encode(data, ncw)
    want = unpack(data, ncw * ld.k)
    est = ESTIMATE_MS_2_16 * ncw / (1 << 16)
    results = {}
    for case, sigma in (("sigma32", 32.0), ("clean", 0.0), ("sigma40", 40.0)):
        vals = values_of(tx, ntx, sigma=sigma)
        ms = decode_line(ld, vals, case, reps, sigma=sigma)
        bits, nb = ld.decode(vals)
        results[case] = ms
        line(case="ldpc_errors_" + case, data_bit_errors=int((unpack(bits, nb) != want).sum()))
        if case == "sigma32":
            line(case="ldpc_estimate", estimate_ms=est, measured_ms=ms, measured_over_estimate=ms / est)
            got_it = ld.iterations().clone()
            tbits, titers = torch_decode(ld, vals)
            same = bool(torch.equal(tbits.reshape(-1), unpack(bits, nb))) and bool(torch.equal(titers.to(torch.uint8), got_it))
            tms, tlo, thi = timed(lambda: torch_decode(ld, vals), max(1, reps // 2))
            line(case="torch_ldpc", codewords=ncw, ms=tms, ms_min=tlo, ms_max=thi, equal_to_fused=same, fused_speedup=tms / ms, met=bool(same and ms < tms))
            results["torch"], results["same"] = tms, same
        del vals
    # (e) the Viterbi decoder over the same number of information bits
    cd = bbb.ConvCode(7, (0o171, 0o133), "3/4")
    nbits = ncw * ld.k
    ctx, nctx = cd.encode(data, nbits)
    soft = values_of(ctx, nctx, sigma=32.0)
    vms, vlo, vhi = timed(lambda: cd.decode(soft), reps)
    line(case="conv_decode_34", K=7, steps=nbits, ms=vms, ms_min=vlo, ms_max=vhi, info_gbit_per_s=nbits / vms / 1e6, ldpc_over_conv=results["sigma32"] / vms)
    sys.exit(0 if results["same"] and results["sigma32"] < results["torch"] else 1)


if __name__ == "__main__":
    main()
