#!/usr/bin/env python3
"""Error-statistics timings: one JSON line per measurement, all in one session.

  python3 profiles/errstat_bench.py [--n 1e10] [--reps 10] [--quick]

For every error rate in 0, 1e-6, 1e-4, 1e-3, 1e-2, 0.5 a packed stream of n bits with independent errors is made on the device, then
  errstat        bbb_errstat_accumulate over the n bits (guard 64, blocks of 1e3 .. 1e6 bits), without a mask
  errstat_mask   the same with a mask of density 1e-5 (two buffers are read)
  check          bbb_prbs_check_dev over the same buffer: the existing reader of the same layout
and at 2^30 bits, rate 1e-4
  torch          what is there without bbb_errstat_*: unpack the words, torch.nonzero, diff, the binning, torch.bincount
  errstat_2p30   bbb_errstat_accumulate over those bits; its gap histogram must equal the composition's
Medians of `reps` calls (hipEvents on the stream) after two warm-up calls.  --quick: rates 1e-4 and 1e-2 only, 3 calls each and
nothing else (kernel-trace runs: the share of errstat_stitch_kernel is read from the trace)."""
import argparse
import ctypes as C
import json
import pathlib
import statistics
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import basebandboard_amd as bbb  # noqa: E402
from basebandboard_amd import _lib  # noqa: E402

DEV = torch.device("cuda", 0)
BLOCKS = (1000, 10000, 100000, 1000000)


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
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def fill(w, n, p, seed):
    """Independent errors of rate p into the packed int64 tensor w; returns their number (None at 0.5)."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    w.zero_()
    if p == 0:
        return 0
    if p >= 0.5:
        hi = torch.randint(0, 1 << 32, (w.numel(),), device=DEV, generator=g)
        w.copy_((hi << 32) | torch.randint(0, 1 << 32, (w.numel(),), device=DEV, generator=g))
        return None
    pos = torch.unique(torch.randint(0, n, (int(n * p),), device=DEV, generator=g))
    w.index_add_(0, pos >> 6, torch.ones_like(pos) << (pos & 63))     # distinct bits of a word: the sum is the OR
    return int(pos.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    n = int(a.n) // 128 * 128
    nw = n // 64
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    err = torch.zeros(nw, dtype=torch.int64, device=DEV)
    if a.quick:
        for p in (1e-4, 1e-2):
            fill(err, n, p, 7)
            with bbb.ErrorStats(64, BLOCKS) as es:
                for _ in range(3):
                    es.accumulate(err, None, n)
                print(json.dumps({"what": "quick", "rate": p, "errors": int(es.read().errors)}), flush=True)
        return
    mask = torch.zeros(nw, dtype=torch.int64, device=DEV)
    fill(mask, n, 1e-5, 99)
    nerr = torch.zeros(1, dtype=torch.int64, device=DEV)
    for p in (0, 1e-6, 1e-4, 1e-3, 1e-2, 0.5):
        cnt = fill(err, n, p, 7)
        for what, m in (("errstat", None), ("errstat_mask", mask)):
            with bbb.ErrorStats(64, BLOCKS) as es:
                es.accumulate(err, m, n)
                r = es.read()
                assert m is not None or cnt is None or r.errors == cnt, (r.errors, cnt)
                es.reset()
                med, lo, hi = timed(lambda: es.accumulate(err, m, n), a.reps)
                print(json.dumps({"what": what, "rate": p, "bits": n, "errors": int(r.errors), "bursts": int(r.bursts), "ms": med,
                                  "ms_min": lo, "ms_max": hi, "read_TBps": n / 8 * (2 if m is not None else 1) / med / 1e9}), flush=True)
        med, lo, hi = timed(lambda: _lib.check(lib.bbb_prbs_check_dev(31, 1, 0, n, C.c_void_p(err.data_ptr()),
                                                                      C.c_void_p(nerr.data_ptr()), 0, stream), "bbb_prbs_check_dev"), a.reps)
        print(json.dumps({"what": "check", "rate": p, "bits": n, "ms": med, "ms_min": lo, "ms_max": hi,
                          "read_TBps": n / 8 / med / 1e9}), flush=True)
    n2 = min(1 << 30, n)
    w2 = err[:n2 // 64]
    fill(err, n, 1e-4, 7)
    sh = torch.arange(64, device=DEV)

    def torch_way():
        bits = ((w2.unsqueeze(1) >> sh) & 1).reshape(-1)
        g = torch.nonzero(bits).squeeze(1).diff()
        e = torch.zeros_like(g)                    # floor(log2 g), exactly
        v = g.clone()
        for s in (32, 16, 8, 4, 2, 1):
            big = v >= (1 << s)
            e += big * s
            v = torch.where(big, v >> s, v)
        return torch.bincount(torch.where(g < 256, g, 256 + e - 8), minlength=312)

    med, lo, hi = timed(torch_way, 3, warm=1)
    print(json.dumps({"what": "torch", "rate": 1e-4, "bits": n2, "ms": med, "ms_min": lo, "ms_max": hi}), flush=True)
    with bbb.ErrorStats(64, ()) as es:
        es.accumulate(w2, None, n2)
        assert list(es.read().gap_hist) == torch_way().cpu().tolist(), "the composition's gap histogram differs"
        es.reset()
        med, lo, hi = timed(lambda: es.accumulate(w2, None, n2), a.reps)
        print(json.dumps({"what": "errstat_2p30", "rate": 1e-4, "bits": n2, "ms": med, "ms_min": lo, "ms_max": hi}), flush=True)


if __name__ == "__main__":
    main()
