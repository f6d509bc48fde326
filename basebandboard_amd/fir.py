"""Exact integer FIR filter over int16 samples -- the receive filter of gateware/bbb/rx.py:24-26 (gateware/bbb/average.py),
a decimator, and the filtered slicer (include/bbb.h, bbb_fir_*).

  acc(n) = sum_i h[i] * x[n - i]        y[q] = sat(acc(phase + q * decim) >> shift)        (x = 0 before the record)

`FIR(taps, shift)` holds up to 256 int16 taps with sum |h| <= 65535, which keeps acc within int32: the arithmetic is exact.
`filter` returns the filtered (and decimated) samples, `slice` the decisions acc >= threshold packed as RX.slice packs them
without the filtered samples ever reaching memory, `stream` an object that filters a record handed over in pieces.
`FIR.moving_average()` is the reference's MovingAverage, `FIR.matched(coefficients)` the matched filter of a shaper tap set,
`FIR.mmse(h, ...)` the MMSE filter designed from a measured pulse response (equalizer.py).
"""
import ctypes as C

import torch

from . import _lib

MAX_TAPS = 256     # BBB_FIR_MAX_TAPS
MAX_DECIM = 256

_DT = {torch.int16: 2, torch.int32: 4}


def nout(nin, decim=1, phase=0):
    """Outputs of `nin` inputs: those at input indices phase, phase + decim, ... below nin."""
    return (nin - phase + decim - 1) // decim if phase < nin else 0


def next_phase(phase, decim, nin):
    """The phase of the chunk that follows a chunk of `nin` inputs filtered at `phase`: (phase - nin) mod decim."""
    return (phase - nin) % decim


class FIR:
    def __init__(self, taps, shift=0, device=0):
        taps = [int(v) for v in taps]
        if not 1 <= len(taps) <= MAX_TAPS:
            raise ValueError("between 1 and 256 taps")
        if any(not -32768 <= v <= 32767 for v in taps):
            raise ValueError("taps must be int16 values")
        if sum(abs(v) for v in taps) > 65535:
            raise ValueError("the sum of |taps| must be <= 65535")
        if not 0 <= int(shift) <= 31:
            raise ValueError("shift must be 0..31")
        self.taps, self.shift, self.device = taps, int(shift), int(device)
        self.design_delay = None          # set by a design that knows where its decision lands (FIR.mmse); link.LinkSweep prefers it

    @classmethod
    def moving_average(cls, pipeline=False, shift=0, device=0):
        """The reference's MovingAverage (bbb_fir_moving_average, host only): taps [1, 1, 1, 1]; with `pipeline` the module's
        registers, [0, 0, 0, 1, 1, 1, 1] (average.py:26-33: x(t) = s(t-3) + .. + s(t-6)).  shift 2 is what the module's
        test expects, 0 what the module computes."""
        c = _lib.FirCfg()
        _lib.check(_lib.lib().bbb_fir_moving_average(C.byref(c), int(bool(pipeline))), "bbb_fir_moving_average")
        return cls(list(c.taps[:c.ntaps]), shift=shift, device=device)

    @classmethod
    def matched(cls, coefficients, shift=0, device=0):
        """The matched filter of a shaper tap set (bitshaper.rcf_coefficients, PRBSShaper.coefficients[i]): the set
        time-reversed."""
        return cls(list(coefficients)[::-1], shift=shift, device=device)

    @classmethod
    def mmse(cls, h, spb, cursor, ntaps, noise_power, shift=0, device=0, scale_bits=8):
        """The MMSE receive filter of a measured pulse response (equalizer.mmse_taps: h from TX.pulse_response or
        RX.pulse_response, noise_power from equalizer.noise_power).  The design's re-timing is kept as `design_delay`
        (cursor - argmax |h|), which link.LinkSweep uses in place of delay() when no `delay` is given, so that the decision
        lands on the cursor."""
        from .equalizer import mmse_taps
        taps, delay = mmse_taps(h, spb, cursor, ntaps, noise_power, scale_bits)
        f = cls(taps.tolist(), shift=shift, device=device)
        f.design_delay = delay
        return f

    def __len__(self):
        return len(self.taps)

    def delay(self):
        """The filter's group delay in whole samples: the floor of the centroid of |h| (1 for [1, 1, 1, 1], 4 for the
        pipelined moving average; 0 for all-zero taps).  What link.LinkSweep re-times the filtered stream by."""
        total = sum(abs(v) for v in self.taps)
        return sum(i * abs(v) for i, v in enumerate(self.taps)) // total if total else 0

    def _cfg(self, decim, phase, out_bytes=2):
        decim, phase = int(decim), int(phase)
        if not 1 <= decim <= MAX_DECIM:
            raise ValueError("decim must be 1..256")
        if not 0 <= phase < decim:
            raise ValueError("phase must be 0 .. decim - 1")
        c = _lib.FirCfg()
        c.ntaps = len(self.taps)
        for i, v in enumerate(self.taps):
            c.taps[i] = v
        c.shift, c.decim, c.phase, c.out_bytes = self.shift, decim, phase, out_bytes
        return c

    def _samples(self, samples, nbefore):
        _lib.cuda_tensor("samples", samples, (torch.int16,), "int16", self.device)
        nbefore = int(nbefore)
        if not 0 <= nbefore <= samples.numel():
            raise ValueError("nbefore must be 0 .. len(samples)")
        return nbefore

    def filter(self, samples, decim=1, phase=0, nbefore=0, out_dtype=torch.int16, out=None):
        """The filtered samples of an int16 CUDA tensor (bbb_fir_filter).  The first `nbefore` elements of `samples` are the
        record's earlier samples (the nearest len(taps) - 1 are used; history beyond them is 0) and produce no output, as
        in SincInterpolator.interpolate; output q sits at index phase + q * decim of the rest.  out_dtype torch.int16
        saturates, torch.int32 never needs to; `out`: a tensor to write into.  Asynchronous on the current torch stream."""
        nbefore = self._samples(samples, nbefore)
        if out is not None:
            out_dtype = out.dtype
        if out_dtype not in _DT:
            raise ValueError("out_dtype must be torch.int16 or torch.int32")
        cfg = self._cfg(decim, phase, _DT[out_dtype])
        nin = samples.numel() - nbefore
        n = nout(nin, cfg.decim, cfg.phase)
        if out is None:
            out = torch.empty(n, dtype=out_dtype, device=samples.device)
        elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dim() != 1 or not out.is_contiguous()
              or out.device != samples.device or out.numel() != n):
            raise ValueError(f"out must be a contiguous 1-D CUDA tensor of {n} elements on the samples' device")
        got = C.c_uint64()
        _lib.check(_lib.lib().bbb_fir_filter(C.c_void_p(samples.data_ptr() + 2 * nbefore), nin, nbefore, C.byref(cfg),
                                             C.c_void_p(out.data_ptr()), C.byref(got), self.device,
                                             C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "bbb_fir_filter")
        assert got.value == n
        return out

    def slice(self, samples, stride=1, phase=0, threshold=0, strict=False, nbefore=0):
        """The decisions of the filtered stream (bbb_fir_slice): bit j = acc(phase + j * stride) >= threshold (`strict`: >),
        threshold in units of acc (`shift` plays no part).  Returns (packed int64 tensor, nbits) as RX.slice does."""
        nbefore = self._samples(samples, nbefore)
        cfg = self._cfg(stride, phase)
        nin = samples.numel() - nbefore
        nbits = nout(nin, cfg.decim, cfg.phase)
        out = torch.empty((nbits + 63) // 64, dtype=torch.int64, device=samples.device)
        got = C.c_uint64()
        _lib.check(_lib.lib().bbb_fir_slice(C.c_void_p(samples.data_ptr() + 2 * nbefore), nin, nbefore, C.byref(cfg),
                                            int(threshold), int(bool(strict)), C.c_void_p(out.data_ptr()), C.byref(got),
                                            self.device, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                   "bbb_fir_slice")
        assert got.value == nbits
        return out, nbits

    def stream(self, decim=1, phase=0, out_dtype=torch.int16):
        """A FIRStream: `push(chunk)` gives the outputs of that chunk, any cutting of a record those of one call."""
        return FIRStream(self, decim, phase, out_dtype)


class Carry:
    """The history of a record handed over in pieces (FIRStream, ddc.DDCStream): the last `keep` samples, in a buffer the
    object owns, in front of which every chunk is copied (so that the filter reads the chunk from a 16-byte aligned
    address)."""

    def __init__(self, keep):
        self.keep = keep
        self.lead = (keep + 7) // 8 * 8               # the chunk starts at this element of the buffer
        self.have = 0                                 # history samples held, at buf[lead - have : lead]
        self.buf = None

    def place(self, chunk):
        """Copies the chunk behind the history: ([history | chunk], nbefore) to hand to the filter."""
        n = chunk.numel()
        if self.buf is None or self.buf.numel() < self.lead + n:
            new = torch.empty(self.lead + max(n, 1), dtype=torch.int16, device=chunk.device)
            if self.have:
                new[self.lead - self.have:self.lead] = self.buf[self.lead - self.have:self.lead]
            self.buf = new
        self.buf[self.lead:self.lead + n] = chunk
        return self.buf[self.lead - self.have:self.lead + n], self.have

    def advance(self, n):
        """Behind the filter's call: the tail of [history | chunk of n] becomes the history."""
        have = min(self.keep, self.have + n)
        if have:
            # (the clone keeps an overlapping move exact)
            self.buf[self.lead - have:self.lead] = self.buf[self.lead + n - have:self.lead + n].clone()
        self.have = have


class FIRStream(Carry):
    """A record filtered piece by piece: the Carry of the last len(taps) - 1 samples, and the phase, which after a chunk of
    n samples is (phase - n) mod decim."""

    def __init__(self, fir, decim=1, phase=0, out_dtype=torch.int16):
        fir._cfg(decim, phase)
        if out_dtype not in _DT:
            raise ValueError("out_dtype must be torch.int16 or torch.int32")
        self.fir, self.decim, self.phase, self.out_dtype = fir, int(decim), int(phase), out_dtype
        super().__init__(len(fir.taps) - 1)

    def push(self, chunk):
        self.fir._samples(chunk, 0)
        samples, nbefore = self.place(chunk)
        out = self.fir.filter(samples, self.decim, self.phase, nbefore=nbefore, out_dtype=self.out_dtype)
        self.advance(chunk.numel())
        self.phase = next_phase(self.phase, self.decim, chunk.numel())
        return out
