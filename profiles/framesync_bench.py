#!/usr/bin/env python3
"""Frame synchroniser timings: one JSON line per measurement.

  timeout 900 python3 profiles/framesync_bench.py [--bits 10000000000] [--reps 5] [--quick]

CCSDS depth-4 frames (8192 bits, marker 1A CF FC 1D, randomised), tol_search 2, tol_lock 6, verify 1, flywheel 2.
  run_clean      bbb_framesync_run over `bits` bits of clean frames of random payloads (one acquisition, LOCK to the end)
  run_nomarker   bbb_framesync_run over as many random bits (SEARCH to the end, the candidates of chance all rejected)
  prbs_check     bbb_prbs_check_dev over the clean buffer in the same session: the memory-speed yardstick; the ratios to it
  extract        bbb_frame_extract of the clean stream's frames, against a torch device-to-device copy of as many bytes
  chain          the one pass/fail number: find plus extract over the bits a K = 7 hard-decision bbb_conv_decode of 2^27 steps
                 produces, against that Viterbi call in the same session: the synchroniser must take less
Every line carries the estimate of DESIGN.md 27 written before the first run and the ratio to it.  Medians of `reps` calls
(hipEvents on the stream) after a warm-up call.  --quick: 2^28 bits, 2^24 steps, 2 repetitions."""
import argparse
import ctypes as C
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import basebandboard_amd as bbb  # noqa: E402
from basebandboard_amd import _lib  # noqa: E402
from conv_bench import values_of  # noqa: E402
from dfe_bench import line, timed  # noqa: E402

SIMD_RATE = 1024 * 2.4e9            # SIMD cycles per second
SEARCH_CYCLES = 0.625               # 10 VALU instructions a position, 4 cycles a wave instruction, 64 positions a wave
LOCK_ROUND_US, SEARCH_ROUND_US = 3.0, 2.5
CANDIDATE_RATE = 2 * (1 + 32 + 496) / 2 ** 32      # random data, 32 bits, tol_search 2, both polarities
HBM = 4.0e12                        # bytes per second a streaming kernel reaches


def estimate_run_ms(nbits, clean):
    search = SEARCH_CYCLES * nbits / SIMD_RATE * 1e3
    chain = nbits / 8192 / 1024 * LOCK_ROUND_US / 1e3 if clean else nbits * CANDIDATE_RATE * SEARCH_ROUND_US / 1e3
    return search + chain


def find_fn(fs, words, nbits):
    """A bbb_framesync_run with buffers allocated once: what is timed is the library's two kernels and the flag memset."""
    mf = nbits // fs.frame_bits + 1
    state = fs.new_state()
    pos = torch.empty(mf, dtype=torch.int64, device=words.device)
    meta = torch.empty(mf, dtype=torch.int16, device=words.device)
    scratch = torch.empty(fs.plan(nbits)[0] // 8, dtype=torch.int64, device=words.device)
    cfg, lib = fs._cfg(), _lib.lib()

    def fn():
        state.zero_()
        _lib.check(lib.bbb_framesync_run(C.c_void_p(words.data_ptr()), nbits, 0, 1, C.byref(cfg), C.c_void_p(state.data_ptr()), C.c_void_p(pos.data_ptr()),
                                         C.c_void_p(meta.data_ptr()), mf, C.c_void_p(scratch.data_ptr()), 0, fs._stream_ptr()), "bbb_framesync_run")
    return fn, state, pos, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=10 ** 10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    nbits, nsteps, reps = (1 << 28, 1 << 24, 2) if args.quick else (args.bits, 1 << 27, args.reps)
    torch.manual_seed(27)
    dev = torch.device("cuda", 0)
    fs = bbb.FrameSync.ccsds(4, tol_search=2, tol_lock=6)
    nf = nbits // fs.frame_bits
    nbits = nf * fs.frame_bits
    payload = torch.randint(0, 256, (nf * fs.payload_bytes,), dtype=torch.uint8, device=dev)
    clean, _ = fs.attach(payload)
    fn, state, pos, meta = find_fn(fs, clean, nbits)
    med, lo, hi = timed(fn, reps)
    st = state.cpu().tolist()
    est = estimate_run_ms(nbits, True)
    line(case="run_clean", bits=nbits, ms=med, ms_min=lo, ms_max=hi, gbit_per_s=nbits / med / 1e6, estimate_ms=est, measured_over_estimate=med / est,
         frames=st[2], acquisitions=st[4], losses=st[5], rejected=st[6])
    assert st[2] == nf and st[4] == 1
    run_ms = med
    nerr = torch.zeros(1, dtype=torch.int64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    chk, lo, hi = timed(lambda: _lib.check(_lib.lib().bbb_prbs_check_dev(31, 1, 0, nbits, C.c_void_p(clean.data_ptr()), C.c_void_p(nerr.data_ptr()), 0, stream),
                                           "bbb_prbs_check_dev"), reps)
    line(case="prbs_check", bits=nbits, ms=chk, ms_min=lo, ms_max=hi, read_TBps=nbits / 8 / chk / 1e9, run_clean_over_check=run_ms / chk)
    # extract of those frames against a copy of as many bytes
    out = torch.empty(nf * fs.payload_bytes, dtype=torch.uint8, device=dev)
    cfg = fs._cfg()
    ext, lo, hi = timed(lambda: _lib.check(_lib.lib().bbb_frame_extract(C.c_void_p(clean.data_ptr()), nbits, 0, C.c_void_p(pos.data_ptr()), C.c_void_p(meta.data_ptr()),
                                                                        C.c_void_p(state.data_ptr()), nf, C.byref(cfg), C.c_void_p(out.data_ptr()), 0, stream),
                                           "bbb_frame_extract"), reps)
    ok = bool(torch.equal(out, payload))
    dst = torch.empty_like(out)
    cp, clo, chi = timed(lambda: dst.copy_(out), reps)
    est = 2 * out.numel() / HBM * 1e3 * 1.3
    line(case="extract", frames=nf, bytes=out.numel(), ms=ext, ms_min=lo, ms_max=hi, copy_ms=cp, extract_over_copy=ext / cp, estimate_ms=est,
         measured_over_estimate=ext / est, payloads_equal=ok)
    del payload, out, dst, clean, pos, meta
    # no marker at all
    noise = torch.randint(-2 ** 63, 2 ** 63 - 1, ((nbits + 63) // 64,), dtype=torch.int64, device=dev)
    fn, state, pos, meta = find_fn(fs, noise, nbits)
    med, lo, hi = timed(fn, reps)
    st = state.cpu().tolist()
    est = estimate_run_ms(nbits, False)
    line(case="run_nomarker", bits=nbits, ms=med, ms_min=lo, ms_max=hi, gbit_per_s=nbits / med / 1e6, estimate_ms=est, measured_over_estimate=med / est,
         run_over_check=med / chk, frames=st[2], acquisitions=st[4], rejected=st[6])
    del noise, pos, meta
    # the chain: the Viterbi decoder's bits at the closed loop's error rate, 1237 junk bits in front, the channel inverted
    outer, inner = bbb.ReedSolomon.ccsds(4), bbb.ConvCode(7, (0o171, 0o133))
    cat = bbb.Concatenated(outer, inner, sync=fs)
    nfc = nsteps // fs.frame_bits
    data = torch.randint(0, 256, (nfc * outer.data_bytes,), dtype=torch.uint8, device=dev)
    tx, ntx = cat.encode(data)
    soft = -values_of(tx, ntx, sigma=42.0)
    hard, nh = bbb.RX(7, 1, 0).slice(soft)
    del soft, tx
    vit_ms, lo, hi = timed(lambda: inner.decode(hard, hard=True, nbits=nh), reps)
    line(case="chain_conv_decode", K=7, steps=ntx // 2, ms=vit_ms, ms_min=lo, ms_max=hi)
    bits, nd = inner.decode(hard, hard=True, nbits=nh)

    def sync():
        p, m, count = fs.find(bits, nd)
        return fs.extract(bits, nd, p, m, count)
    sync_ms, lo, hi = timed(sync, reps)
    frames, n = fs.sync(bits, nd)
    got, _ = outer.decode(frames.contiguous())
    est = (SEARCH_CYCLES * nd / SIMD_RATE + nd / 8192 / 1024 * LOCK_ROUND_US / 1e6 + 2 * nd / 8 / HBM) * 1e3 + 0.1
    line(case="chain", steps=ntx // 2, conv_decode_ms=vit_ms, sync_ms=sync_ms, ms_min=lo, ms_max=hi, sync_over_conv=sync_ms / vit_ms, met=bool(sync_ms < vit_ms),
         estimate_ms=est, measured_over_estimate=sync_ms / est, frames=n, frames_sent=nfc, data_bytes_wrong=int((got != data[:got.numel()]).sum()))


if __name__ == "__main__":
    main()
