"""16x sinc interpolator -- mirror of gateware/bbb/sinc.py, the scope's SincInterpolator: 72 captured 8-bit samples in, 1024
interpolated samples out, 16 output samples per input sample through an 8-tap polyphase windowed sinc.

  acc(m, c) = sum_{i=0..7} h[16 i + c] * x[m - i]      y[16 m + c] = int8(acc(m, c) >> 8)      (x = 0 before the record)

`run` is the module as the scope uses it (y[109:1133] of 72 inputs); `interpolate` is the same filter as a stream over a
record of any length, int8 or int16 in and out, so that a capture at 4 samples per bit gives the eye 64 columns per bit
(`eye`, `RX.eye(..., interpolate=True)`) and the sampling knob 64 settings (`RX.phase_search(..., interpolate=True)`).
The DC gain is 125/256 or 126/256 per phase: the reference halves the amplitude, and so does this (include/bbb.h).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

UP = 16            # BBB_SINC_UP: output samples per input sample
TAPS = 8           # BBB_SINC_TAPS: input samples per output sample
BATCH_IN = 72      # the module's input record (sinc.py:56-57) ...
BATCH_OUT = 1024   # ... and output record,
BATCH_OFFSET = 109  # which is y[109:1133] of the stream form (the alignment gateware/bbb/tests/test_sinc.py asserts)

_DT = {torch.int8: 1, torch.int16: 2}


class SincInterpolator:
    def __init__(self, device=0):
        self.device = int(device)

    @staticmethod
    def coefficients():
        """The table h (bbb_sinc_coefficients, host only): int8[128], trunc(127 sinc(t) hamming), t = linspace(-4, 4, 128)
        (sinc.py:38-41).  Tap i of phase c is h[16 i + c]."""
        h = np.zeros(128, dtype=np.int8)
        _lib.check(_lib.lib().bbb_sinc_coefficients(h.ctypes.data_as(C.c_void_p)), "bbb_sinc_coefficients")
        return h

    @classmethod
    def packed_coefficients(cls):
        """The 32 words of the module's coefficient BRAM (sinc.py:42-48), as make_sinc_coefficients returns them."""
        u = cls.coefficients().view(np.uint8).astype(np.uint32)
        a = u[0:16] << 24 | u[16:32] << 16 | u[32:48] << 8 | u[48:64]
        b = u[64:80] << 24 | u[80:96] << 16 | u[96:112] << 8 | u[112:128]
        packed = np.empty(32, dtype=np.uint32)
        packed[0::2], packed[1::2] = a, b
        return packed.tolist()

    def _dev(self):
        return torch.device("cuda", self.device)

    def _check(self, samples, shift):
        _lib.cuda_tensor("samples", samples, _DT, "int8 or int16", self.device)
        shift = int(shift)
        if not 0 <= shift <= 15:
            raise ValueError("shift must be 0..15")
        if shift and samples.dtype == torch.int8:
            raise ValueError("shift must be 0 with int8 samples")
        return shift

    @staticmethod
    def _nbefore(samples, nbefore):
        nbefore = int(nbefore)
        if not 0 <= nbefore <= samples.numel():
            raise ValueError("nbefore must be 0 .. len(samples)")
        return nbefore

    def interpolate(self, samples, nbefore=0, shift=0, out_dtype=None, out=None):
        """The stream form over an int8 or int16 CUDA tensor (bbb_sinc_interpolate).  The first `nbefore` elements of
        `samples` are the record's earlier samples (the nearest 7 are used; history beyond them is 0) and produce no
        output: the result has 16 * (len(samples) - nbefore) elements, so that a record cut anywhere and handed over
        with 7 samples of overlap gives the same stream as one call.  int16 samples are taken as
        clamp(x >> shift, -128, 127).  out_dtype: torch.int8 or torch.int16 (default: the samples' dtype); `out`: a
        tensor to write into.  Asynchronous on the current torch stream."""
        shift = self._check(samples, shift)
        nbefore = self._nbefore(samples, nbefore)
        nin = samples.numel() - nbefore
        if out is not None:
            if out_dtype is not None and out.dtype != out_dtype:
                raise ValueError("out does not have out_dtype")
            out_dtype = out.dtype
        elif out_dtype is None:
            out_dtype = samples.dtype
        if out_dtype not in _DT:
            raise ValueError("out_dtype must be torch.int8 or torch.int16")
        if out is None:
            out = torch.empty(UP * nin, dtype=out_dtype, device=samples.device)
        elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dim() != 1 or not out.is_contiguous()
              or out.device != samples.device or out.numel() != UP * nin):
            raise ValueError(f"out must be a contiguous 1-D CUDA tensor of {UP * nin} elements on the samples' device")
        cfg = _lib.SincCfg(_DT[samples.dtype], _DT[out_dtype], shift)
        _lib.check(_lib.lib().bbb_sinc_interpolate(
            C.c_void_p(samples.data_ptr() + nbefore * samples.element_size()), nin, nbefore, C.byref(cfg),
            C.c_void_p(out.data_ptr()), self.device, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
            "bbb_sinc_interpolate")
        return out

    def run(self, samples):
        """The module's batch: 72 int8 values (a tensor, an array or a sequence) with no history -> the 1024 int8 values it
        writes to its output memory, y[109:1133].  A tensor in gives a tensor on the same device, anything else a numpy
        array."""
        if isinstance(samples, torch.Tensor):
            if samples.dtype != torch.int8 or samples.numel() != BATCH_IN:
                raise ValueError("samples must be 72 int8 values")
            x = samples.reshape(-1).to(self._dev()).contiguous()
        else:
            a = np.asarray(samples)
            if a.size != BATCH_IN or a.dtype.kind not in "iu" or a.min() < -128 or a.max() > 127:
                raise ValueError("samples must be 72 int8 values")
            x = torch.from_numpy(a.reshape(-1).astype(np.int8)).to(self._dev())
        y = self.interpolate(x)[BATCH_OFFSET:BATCH_OFFSET + BATCH_OUT]
        return y.to(samples.device) if isinstance(samples, torch.Tensor) else y.cpu().numpy()

    def eye(self, samples, first_sample=0, eye=None, hist=None, shift=0, nbefore=0, chunk_in=0):
        """Eye histogram of the interpolated record (bbb_sinc_eye_*), which is never handed to the caller: what
        eye.capture_eye counts over interpolate(samples, nbefore, shift, torch.int16), whose sample 16 m + c has the sample
        number 16 * (first_sample + m) + c.  `eye`: an eye.EyeConfig for the interpolated stream (default 64 columns, shift
        0: the interpolated values are 8-bit already); chunk_in: input samples per chunk of the object's buffer (0: 2^24).
        Returns hist [256, ncols] uint64 (added to when given)."""
        from .eye import EyeConfig, ROWS, _counters
        shift = self._check(samples, shift)
        nbefore = self._nbefore(samples, nbefore)
        eye = eye or EyeConfig(ncols=64, shift=0)
        hist = _counters(hist, (ROWS, int(eye.ncols)), samples.device, "hist")
        cfg, ec = _lib.SincCfg(_DT[samples.dtype], 2, shift), eye._c()
        lib = _lib.lib()
        e = C.c_void_p()
        _lib.check(lib.bbb_sinc_eye_open(C.byref(cfg), C.byref(ec), int(chunk_in), self.device,
                                         C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream), C.byref(e)),
                   "bbb_sinc_eye_open")
        try:
            _lib.check(lib.bbb_sinc_eye_run(e, C.c_void_p(samples.data_ptr() + nbefore * samples.element_size()),
                                            samples.numel() - nbefore, nbefore, int(first_sample),
                                            C.c_void_p(hist.data_ptr())), "bbb_sinc_eye_run")
        finally:
            _lib.check(lib.bbb_sinc_eye_close(e), "bbb_sinc_eye_close")
        return hist
