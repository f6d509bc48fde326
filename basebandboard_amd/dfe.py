"""Exact decision-feedback equalizer over int16 samples -- the receiver's step behind the linear equalizer (include/bbb.h,
bbb_dfe_*): the post-cursor interference of the bits already decided is subtracted before the next decision.

  a[k] = acc(phase + k * spb)       v[k] = a[k] - sum_i fb[i] * d[k - 1 - i]       bit[k] = v[k] >= threshold     (d = +1 / -1)

`DFE(ff, fb, spb)` holds the feed-forward filter (a fir.FIR, or its taps) and up to 4 int32 feedback taps in units of acc;
32768 * sum |ff| + sum |fb| <= 2^31 - 1 keeps v within int32, so the arithmetic is exact.  `slice` returns the decisions packed
as RX.slice packs them, `equalize` the decisions and the soft values v, `stream` an object that equalizes a record handed
over in pieces.  The decisions in front of a call are a state word ON THE DEVICE (bit i: the decision i + 1 symbols back; a
zeroed word is the shift register out of reset), read and rewritten by the call, so a stream never synchronises.
`DFE.mmse(h, ...)` designs both filters from a measured pulse response (equalizer.dfe_taps).
"""
import ctypes as C

import torch

from . import _lib
from .fir import FIR, Carry, nout, next_phase, _DT

MAX_FB = 4     # BBB_DFE_MAX_FB


def geometry(spb):
    """Where the device cuts the work at `spb` samples per bit (bbb_dfe_geometry, host only): a dict of step_samples,
    step_symbols, wave_symbols and the defaults region_symbols and warmup_symbols."""
    names = ("step_samples", "step_symbols", "wave_symbols", "region_symbols", "warmup_symbols")
    v = [C.c_uint64() for _ in names]
    _lib.check(_lib.lib().bbb_dfe_geometry(int(spb), *[C.byref(x) for x in v]), "bbb_dfe_geometry")
    return {n: x.value for n, x in zip(names, v)}


class DFE:
    def __init__(self, ff, fb, spb, phase=0, threshold=0, strict=False, region_symbols=0, warmup_symbols=0):
        self.ff = ff if isinstance(ff, FIR) else FIR(ff)
        self.fb = [int(v) for v in fb]
        if len(self.fb) > MAX_FB:
            raise ValueError("at most 4 feedback taps")
        if any(not -2 ** 31 <= v < 2 ** 31 for v in self.fb):
            raise ValueError("feedback taps must be int32 values")
        if 32768 * sum(abs(v) for v in self.ff.taps) + sum(abs(v) for v in self.fb) > 2 ** 31 - 1:
            raise ValueError("32768 * sum |ff taps| + sum |fb| must be <= 2^31 - 1")
        if not -2 ** 31 <= int(threshold) < 2 ** 31:
            raise ValueError("threshold must be an int32 value")
        self.ff._cfg(spb, phase)
        self.spb, self.phase, self.threshold, self.strict = int(spb), int(phase), int(threshold), bool(strict)
        self.region_symbols, self.warmup_symbols = int(region_symbols), int(warmup_symbols)
        self.device = self.ff.device
        self.design_delay = None
        self._stats = None

    @classmethod
    def mmse(cls, h, spb, cursor, nff, nfb, noise_power, phase=0, shift=0, device=0, scale_bits=8, **kw):
        """The MMSE-DFE of a measured pulse response (equalizer.dfe_taps); the design's re-timing is kept as `design_delay`."""
        from .equalizer import dfe_taps
        ff, fb, delay = dfe_taps(h, spb, cursor, nff, nfb, noise_power, scale_bits)
        d = cls(FIR(ff.tolist(), shift=shift, device=device), fb.tolist(), spb, phase, **kw)
        d.design_delay = d.ff.design_delay = delay
        return d

    def _cfg(self, phase=None, out_bytes=2):
        c = _lib.DfeCfg()
        c.ff = self.ff._cfg(self.spb, self.phase if phase is None else phase, out_bytes)
        c.nfb = len(self.fb)
        for i, v in enumerate(self.fb):
            c.fb[i] = v
        c.threshold, c.strict = self.threshold, int(self.strict)
        c.region_symbols, c.warmup_symbols = self.region_symbols, self.warmup_symbols
        return c

    def new_state(self, value=0):
        """A state word on the device."""
        return torch.full((1,), int(value), dtype=torch.int32, device=torch.device("cuda", self.device))

    def _run(self, samples, nbefore, state, soft_dtype, phase=None):
        nbefore = self.ff._samples(samples, nbefore)
        if state is None:
            state = self.new_state()
        _lib.cuda_tensor("state", state, (torch.int32,), "int32", self.device)
        if state.numel() != 1:
            raise ValueError("state must hold one element")
        cfg = self._cfg(phase, 2 if soft_dtype is None else _DT[soft_dtype])
        nin = samples.numel() - nbefore
        nbits = nout(nin, cfg.ff.decim, cfg.ff.phase)
        bits = torch.empty((nbits + 63) // 64, dtype=torch.int64, device=samples.device)
        soft = None if soft_dtype is None else torch.empty(nbits, dtype=soft_dtype, device=samples.device)
        if self._stats is None:
            self._stats = torch.zeros(4, dtype=torch.int64, device=samples.device)
        got = C.c_uint64()
        _lib.check(_lib.lib().bbb_dfe_run(C.c_void_p(samples.data_ptr() + 2 * nbefore), nin, nbefore, C.byref(cfg),
                                          C.c_void_p(state.data_ptr()), C.c_void_p(bits.data_ptr()),
                                          C.c_void_p(soft.data_ptr()) if soft is not None else None,
                                          C.c_void_p(self._stats.data_ptr()), C.byref(got), self.device,
                                          C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "bbb_dfe_run")
        assert got.value == nbits
        return bits, nbits, soft

    def slice(self, samples, nbefore=0, state=None, phase=None):
        """The decisions of an int16 CUDA tensor (bbb_dfe_run): (packed int64 tensor, nbits) as FIR.slice returns them.  The
        first `nbefore` elements are the record's earlier samples, as in FIR.filter.  state: a one-element int32 CUDA tensor
        (new_state()), read and rewritten on the device; None: out of reset.  phase: in place of the object's.
        Asynchronous on the current torch stream."""
        bits, nbits, _ = self._run(samples, nbefore, state, None, phase)
        return bits, nbits

    def equalize(self, samples, nbefore=0, state=None, phase=None, out_dtype=torch.int16):
        """slice, and the soft values the decisions were taken from -- the equalized eye: (packed bits, nbits, soft), soft
        sat16(v >> ff.shift) as int16 or v itself as int32."""
        if out_dtype not in _DT:
            raise ValueError("out_dtype must be torch.int16 or torch.int32")
        return self._run(samples, nbefore, state, out_dtype, phase)

    def stream(self, out_dtype=None):
        """A DFEStream: `push(chunk)` gives the decisions (out_dtype given: and soft values) of that chunk, any cutting of a
        record those of one call."""
        return DFEStream(self, out_dtype)

    def stats(self):
        """What the calls through this object added up (synchronises): regions, regions whose start state was not proven by
        their warm-up, regions walked a second time, symbols."""
        v = [0, 0, 0, 0] if self._stats is None else self._stats.cpu().tolist()
        return dict(zip(("regions", "not_proven", "repaired", "symbols"), v))


class DFEStream(Carry):
    """A record equalized piece by piece: fir.Carry holds the last len(ff) - 1 samples, `state` the device's state word, and
    the phase moves on as FIRStream's does."""

    def __init__(self, dfe, out_dtype=None):
        if out_dtype is not None and out_dtype not in _DT:
            raise ValueError("out_dtype must be None, torch.int16 or torch.int32")
        self.dfe, self.phase, self.out_dtype = dfe, dfe.phase, out_dtype
        self.state = dfe.new_state()
        super().__init__(len(dfe.ff.taps) - 1)

    def push(self, chunk):
        """(packed bits, nbits) of the chunk, or (packed bits, nbits, soft)."""
        self.dfe.ff._samples(chunk, 0)
        samples, nbefore = self.place(chunk)
        out = self.dfe._run(samples, nbefore, self.state, self.out_dtype, self.phase)
        self.advance(chunk.numel())
        self.phase = next_phase(self.phase, self.dfe.spb, chunk.numel())
        return out if self.out_dtype is not None else out[:2]
