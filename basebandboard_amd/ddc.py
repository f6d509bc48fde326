"""Digital down-converter -- the receive half of the NCO (include/bbb.h, bbb_ddc_*): an int16 capture at a carrier is mixed
with the oscillator's cosine and minus sine, both products are filtered and decimated by one exact integer FIR, and the
result is baseband I/Q, or its magnitude and phase.

  mi(n) = (x(n) * c(n)) >> 15    mq(n) = (x(n) * -s(n)) >> 15    c, s: the NCO's ROM at phase pa0 + (first_sample + n) * fcw
  I[q]  = sat16(sum_i h[i] mi(phase + q * decim - i) >> shift)   Q[q] likewise

The oscillator is a function of the absolute sample number, so a capture handed over in pieces (`stream`, or `nbefore` /
`first_sample` by hand) gives the outputs of one call.  `NCO.ddc(taps)` builds the converter that is phase-aligned with that
oscillator's own output.  `polar` / `am` / `pm` / `fm` give the magnitude (uint16), the phase (int16, 1/65536 turn) and the
phase's wrapped first difference.  Everything is exact integer arithmetic; bbb.h states it formula by formula.
"""
import ctypes as C

import torch

from . import _lib
from .fir import FIR, Carry, nout as fir_nout, next_phase

_MODE = {torch.int16: _lib.DDC_IQ16, torch.int32: _lib.DDC_IQ32}


def polar_host(i, q):
    """(mag, phase) of one int16 pair by the kernel's CORDIC (bbb_ddc_polar_host; no GPU needed)."""
    m, p = C.c_uint16(), C.c_int16()
    _lib.check(_lib.lib().bbb_ddc_polar_host(int(i), int(q), C.byref(m), C.byref(p)), "bbb_ddc_polar_host")
    return m.value, p.value


class DDC:
    def __init__(self, fcw, taps, decim=1, phase=0, shift=0, pa0=0, device=0):
        """fcw, pa0 < 2^24 as in NCO; `taps` a list of int16 (with `shift` and `device`) or a fir.FIR, which brings its own
        shift and device; decim 1..256 and phase < decim as in FIR.filter."""
        self.fir = taps if isinstance(taps, FIR) else FIR(taps, shift, device)
        self.device = self.fir.device
        self.fcw, self.pa0 = int(fcw), int(pa0)
        if not 0 <= self.fcw < 1 << 24:
            raise ValueError("fcw must be in [0, 2^24)")
        if not 0 <= self.pa0 < 1 << 24:
            raise ValueError("pa0 must be in [0, 2^24)")
        self.fir._cfg(decim, phase)
        self.decim, self.phase = int(decim), int(phase)

    def _run(self, samples, first_sample, nbefore, mode, out, phase=None):
        nbefore = self.fir._samples(samples, nbefore)
        first_sample = int(first_sample)
        if first_sample < 0:
            raise ValueError("first_sample must be >= 0")
        fcfg = self.fir._cfg(self.decim, self.phase if phase is None else phase)
        nin = samples.numel() - nbefore
        n = fir_nout(nin, fcfg.decim, fcfg.phase)
        dtype = torch.int32 if mode == _lib.DDC_IQ32 else torch.int16
        if out is None:
            out = torch.empty((n, 2), dtype=dtype, device=samples.device)
        elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != dtype or tuple(out.shape) != (n, 2)
              or not out.is_contiguous() or out.device != samples.device):
            raise ValueError(f"out must be a contiguous [{n}, 2] {dtype} CUDA tensor on the samples' device")
        cfg = _lib.DdcCfg(self.fcw, self.pa0, mode)
        got = C.c_uint64()
        _lib.check(_lib.lib().bbb_ddc_run(C.c_void_p(samples.data_ptr() + 2 * nbefore), nin, nbefore, first_sample, C.byref(cfg),
                                          C.byref(fcfg), C.c_void_p(out.data_ptr()), C.byref(got), self.device,
                                          C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "bbb_ddc_run")
        assert got.value == n
        return out

    def iq(self, samples, first_sample=0, nbefore=0, out_dtype=torch.int16, out=None, carrier=None):
        """[nout, 2] (I, Q) of an int16 CUDA tensor (bbb_ddc_run).  The first `nbefore` elements of `samples` are the
        record's earlier samples, as in FIR.filter, and samples[nbefore] has the absolute number `first_sample`.  out_dtype
        torch.int16 saturates, torch.int32 never needs to.  Asynchronous on the current torch stream.
        carrier (a carrier.CarrierRecovery; int16 only, excludes out): the pairs go through carrier.derotate, and what
        comes back are the pairs turned back by the recovered carrier phase, the data axis on I."""
        if carrier is not None and (out is not None or out_dtype != torch.int16):
            raise ValueError("carrier takes int16 pairs and excludes out")
        if out is not None:
            out_dtype = out.dtype
        if out_dtype not in _MODE:
            raise ValueError("out_dtype must be torch.int16 or torch.int32")
        pairs = self._run(samples, first_sample, nbefore, _MODE[out_dtype], out)
        return pairs if carrier is None else carrier.derotate(pairs)

    def polar(self, samples, first_sample=0, nbefore=0, out=None):
        """(mag uint16 [nout], phase int16 [nout]): views of one interleaved [nout, 2] int16 tensor (`out` when given)."""
        return _polar_views(self._run(samples, first_sample, nbefore, _lib.DDC_POLAR, out))

    def am(self, samples, first_sample=0, nbefore=0):
        """The magnitude: the envelope of an AM carrier."""
        return self.polar(samples, first_sample, nbefore)[0]

    def pm(self, samples, first_sample=0, nbefore=0):
        """The phase in 1/65536 turn."""
        return self.polar(samples, first_sample, nbefore)[1]

    def fm(self, samples, first_sample=0, nbefore=0):
        """The wrapped first difference of the phase, int16 [nout - 1]: element q is phase[q + 1] - phase[q] modulo 2^16,
        the frequency offset in 1/65536 turn per output sample."""
        p = self.pm(samples, first_sample, nbefore)
        return p[1:] - p[:-1]

    def stream(self, first_sample=0, out_dtype=torch.int16, polar=False):
        """A DDCStream: `push(chunk)` gives the outputs of that chunk, any cutting of a record those of one call."""
        return DDCStream(self, first_sample, out_dtype, polar)


def _polar_views(t):
    return t[:, 0].view(torch.uint16), t[:, 1]


class DDCStream(Carry):
    """A record converted piece by piece.  As FIRStream, the object is the fir.Carry of the last len(taps) - 1 samples; it
    carries the decimation phase (fir.next_phase) and the running sample number, which is all the oscillator needs."""

    def __init__(self, ddc, first_sample=0, out_dtype=torch.int16, polar=False):
        if out_dtype not in _MODE:
            raise ValueError("out_dtype must be torch.int16 or torch.int32")
        self.ddc, self.polar = ddc, bool(polar)
        self.mode = _lib.DDC_POLAR if polar else _MODE[out_dtype]
        self.phase, self.first_sample = ddc.phase, int(first_sample)
        super().__init__(len(ddc.fir.taps) - 1)

    def push(self, chunk):
        """[nout, 2] of the chunk ((mag, phase) views with polar=True)."""
        self.ddc.fir._samples(chunk, 0)
        n = chunk.numel()
        samples, nbefore = self.place(chunk)
        out = self.ddc._run(samples, self.first_sample, nbefore, self.mode, None, phase=self.phase)
        self.advance(n)
        self.phase = next_phase(self.phase, self.ddc.decim, n)
        self.first_sample += n
        return _polar_views(out) if self.polar else out
