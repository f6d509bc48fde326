"""Eye diagram and bathtub counts -- the link tester's persistence eye (gateware/bbb/dso.py, drawn by ui.py with the
sampling-time / threshold cross-hair `thresh_x` / `thresh_y`, ui.py:139) and the BER per sampling phase, on the GPU.

The DSO keeps 256 rows x 64 columns and lights the pixel (127 - sample, position after a line trigger).  Here every sample
is counted: `hist[row, col]` (uint64) with row = 127 - clamp(x >> shift, -128, 127) and col = (n - col_origin) mod ncols
for sample number n; `persistence(hist)` is the DSO's memory image.  The bathtub decides data bit m from sample
8m + BIT_SAMPLE0 + p at phase p (0..7; phase 4 is the pulse centre) and counts `bathtub[p] = (bits, errors)` against the
transmitter's own source.  Both outputs are added to, so that a range may be cut into calls (include/bbb.h).

  RX.eye(samples)          eye of an int16 CUDA tensor (a capture, or TX.generate output): bbb_eye_accumulate_i16
  TX.eye(nsamples, ...)    eye and bathtub of the transmitter's waveform over any range, never materialised: bbb_tx_eye_*
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

BIT_SAMPLE0 = 45          # BBB_TX_BIT_SAMPLE0: bit m peaks at sample 8m + 49, phase p samples it at 8m + 45 + p
ROWS = 256


@dataclass
class EyeConfig:
    """bbb_eye_cfg.  ncols: 8, 16, 32 or 64 (the DSO: 64); shift: 0..15, bits dropped before the 8-bit row (4 takes a
    12-bit transmitter sample to the DSO's 8 bits); col_origin: the sample number that lands in column 0; threshold /
    strict: the bathtub's decision x >= threshold (rx.py:29 at 0) or x > threshold (software/memdump/decode.py:15)."""
    ncols: int = 64
    shift: int = 4
    col_origin: int = 0
    threshold: int = 0
    strict: bool = False

    def _c(self):
        if not 0 <= int(self.ncols) < 1 << 32 or not 0 <= int(self.shift) < 1 << 32:
            raise ValueError("ncols and shift are unsigned")
        return _lib.EyeCfg(int(self.ncols), int(self.shift), int(self.col_origin) & ((1 << 64) - 1), int(self.threshold),
                           int(bool(self.strict)))


def persistence(hist):
    """The DSO's memory image of a histogram: uint8 [256, ncols], 1 where a sample landed (row-major, so for ncols = 64
    the flat index is the DSO address row << 6 | col, dso.py:29-31).  Pure numpy."""
    h = hist.cpu().numpy() if isinstance(hist, torch.Tensor) else np.asarray(hist)
    if h.ndim != 2 or h.shape[0] != ROWS:
        raise ValueError("hist must be [256, ncols]")
    return (h > 0).astype(np.uint8)


def _counters(out, shape, dev, what):
    if out is None:
        return torch.zeros(shape, dtype=torch.uint64, device=dev)
    if (out.dtype not in (torch.uint64, torch.int64) or tuple(out.shape) != shape or not out.is_contiguous()
            or out.device != dev):
        raise ValueError(f"{what} must be a contiguous {list(shape)} uint64 (or int64) tensor on {dev}")
    return out


def capture_eye(samples, first_sample=0, eye=None, hist=None):
    """Eye of an int16 CUDA tensor: samples[i] is sample number first_sample + i.  Adds into `hist` ([256, ncols]
    uint64 on the samples' device, allocated zeroed when None) and returns it."""
    eye = eye or EyeConfig()
    if samples.dtype != torch.int16 or not samples.is_cuda or not samples.is_contiguous():
        raise ValueError("samples must be a contiguous int16 CUDA tensor")
    hist = _counters(hist, (ROWS, int(eye.ncols)), samples.device, "hist")
    dev = samples.device.index or 0
    cfg = eye._c()
    _lib.check(_lib.lib().bbb_eye_accumulate_i16(C.c_void_p(samples.data_ptr()), samples.numel(), int(first_sample),
                                                 C.byref(cfg), C.c_void_p(hist.data_ptr()), dev,
                                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
               "bbb_eye_accumulate_i16")
    return hist


class TxEye(_lib.Handle):
    """bbb_tx_eye_*: eye and bathtub of a TX's waveform (its settings copied at open), chunk by chunk on the generator's
    stream.  Context manager; close it before the TX's generator handle goes."""
    _handle, _close = "_e", "bbb_tx_eye_close"

    def __init__(self, tx, eye=None, warmup=16, chunk_samples=0):
        self.tx, self.eye = tx, eye or EyeConfig(col_origin=BIT_SAMPLE0)
        cfg = tx._c_cfg(warmup)
        ec = self.eye._c()
        e = C.c_void_p()
        tx.urng._bind_stream()
        _lib.check(_lib.lib().bbb_tx_eye_open(tx.urng._h, C.byref(cfg), C.byref(ec), int(chunk_samples), C.byref(e)),
                   "bbb_tx_eye_open")
        self._e = e

    def run(self, nsamples, first_sample=0, hist=None, bathtub=None, want_hist=True, want_bathtub=True):
        """Samples [first_sample, first_sample + nsamples): adds into hist ([256, ncols]) and bathtub ([8, 2]: bits, errors
        per phase), allocated zeroed when None and wanted; returns (hist, bathtub), None for an output not wanted."""
        dev = torch.device("cuda", self.tx.device)
        hist = _counters(hist, (ROWS, int(self.eye.ncols)), dev, "hist") if want_hist or hist is not None else None
        bathtub = _counters(bathtub, (8, 2), dev, "bathtub") if want_bathtub or bathtub is not None else None
        self.tx.urng._bind_stream()
        _lib.check(_lib.lib().bbb_tx_eye_run(self._e, int(first_sample), int(nsamples),
                                             C.c_void_p(hist.data_ptr() if hist is not None else None),
                                             C.c_void_p(bathtub.data_ptr() if bathtub is not None else None)),
                   "bbb_tx_eye_run")
        return hist, bathtub


def tx_eye(tx, nsamples, first_sample=0, warmup=16, eye=None, chunk_samples=0, hist=None, bathtub=None):
    """TX.eye: (hist [256, ncols] uint64, bathtub [8, 2] uint64) of samples [first_sample, first_sample + nsamples)."""
    with TxEye(tx, eye, warmup, chunk_samples) as e:
        return e.run(nsamples, first_sample, hist, bathtub)
