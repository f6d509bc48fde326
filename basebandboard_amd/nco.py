"""Numerically controlled oscillator -- mirror of gateware/bbb/nco.py, the board's tone source (NCOTest, gateware/top.py:38-61).

`NCO(fcw, am, fm, pm)` keeps the reference's signature and widths (n = 24, m = 10, p = 16; no others).  The constants are the
module's inputs held still; `generate` takes per-sample CUDA tensors in their place for one call (the NCOTest wiring
`fm = adc_b.data << 8` is `generate(n, fm=capture.int() << 8)`).  The object keeps the module's four registers on the device
and every call continues the waveform from them (include/bbb.h, bbb_nco_* gives the register semantics).
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib

NCOState = collections.namedtuple("NCOState", "pa q w y")
NCOState.__doc__ = "The module's registers: pa (24-bit phase accumulator), q (the ROM port's output), w, y.  All 0 = reset."

_RESET = NCOState(0, 0, 0, 0)


def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an integer")
    if not lo <= int(v) < hi:
        raise ValueError(f"{name} must be in [{lo}, {hi}) (got {v})")
    return int(v)


class NCO(_lib.StreamHandle):
    _handle, _close, _set_stream = "_o", "bbb_nco_close", "bbb_nco_set_stream"

    def __init__(self, fcw, am=0xFFFF, fm=0, pm=0, n=24, m=10, p=16, device=0):
        if (n, m, p) != (24, 10, 16):
            raise ValueError("only the reference's widths n=24, m=10, p=16 are implemented")
        self.device = int(device)
        self._cfg = self._make_cfg(fcw, am, fm, pm)
        o = C.c_void_p()
        _lib.check(_lib.lib().bbb_nco_open(C.byref(self._cfg), self.device, self._open_stream(), C.byref(o)), "bbb_nco_open")
        self._o = o

    @staticmethod
    def _make_cfg(fcw, am, fm, pm):
        return _lib.NcoCfg(_int_in("fcw", fcw, 0, 1 << 24), _int_in("am", am, 0, 1 << 16),
                           _int_in("fm", fm, -(1 << 23), 1 << 23), _int_in("pm", pm, -512, 512))

    @staticmethod
    def rom_table():
        """The ROM (bbb_nco_rom, host only): int16[1024], round(32767 sin(2 pi i / 1023)) (nco.py:30-31)."""
        r = np.zeros(1024, dtype=np.int16)
        _lib.check(_lib.lib().bbb_nco_rom(r.ctypes.data_as(C.c_void_p)), "bbb_nco_rom")
        return r

    @property
    def rom(self):
        return self.rom_table()

    @property
    def fcw(self):
        return self._cfg.fcw

    @property
    def am(self):
        return self._cfg.am

    @property
    def fm(self):
        return self._cfg.fm

    @property
    def pm(self):
        return self._cfg.pm

    def set_cfg(self, fcw=None, am=None, fm=None, pm=None):
        """Retune (any of the constants) between calls; the registers are kept."""
        c = self._cfg
        cfg = self._make_cfg(c.fcw if fcw is None else fcw, c.am if am is None else am, c.fm if fm is None else fm,
                             c.pm if pm is None else pm)
        _lib.check(_lib.lib().bbb_nco_set_cfg(self._o, C.byref(cfg)), "bbb_nco_set_cfg")
        self._cfg = cfg

    def _buf(self, name, t, dtype, nsamples):
        if t is None:
            return None
        _lib.cuda_tensor(name, t, (dtype,), dtype, self.device)
        if t.numel() < nsamples:
            raise ValueError(f"{name} holds {t.numel()} values, the call needs {nsamples}")
        return t

    def generate(self, nsamples, fm=None, am=None, pm=None, out=None):
        """The next nsamples outputs x(t) as an int16 CUDA tensor (into `out` when given).  fm (int32; its low 24 bits count),
        am (uint16) and pm (int16; its low 10 bits count) CUDA tensors of at least nsamples values override the constants
        for this call.  Asynchronous on the current torch stream."""
        nsamples = int(nsamples)
        if nsamples < 0:
            raise ValueError("nsamples must be >= 0")
        fm = self._buf("fm", fm, torch.int32, nsamples)
        am = self._buf("am", am, torch.uint16, nsamples)
        pm = self._buf("pm", pm, torch.int16, nsamples)
        if out is None:
            out = torch.empty(nsamples, dtype=torch.int16, device=torch.device("cuda", self.device))
        else:
            out = self._buf("out", out, torch.int16, nsamples)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)   # noqa: E731
        self._bind_stream()
        _lib.check(_lib.lib().bbb_nco_run(self._o, ptr(fm), ptr(am), ptr(pm), nsamples, ptr(out)), "bbb_nco_run")
        return out

    @property
    def state(self):
        """The registers after every call queued so far (waits for them)."""
        s = _lib.NcoState()
        self._bind_stream()
        _lib.check(_lib.lib().bbb_nco_get_state(self._o, C.byref(s)), "bbb_nco_get_state")
        return NCOState(s.pa, s.q, s.w, s.y)

    @state.setter
    def state(self, st):
        pa, q, w, y = st
        s = _lib.NcoState(_int_in("pa", pa, 0, 1 << 24), _int_in("q", q, -(1 << 15), 1 << 15),
                          _int_in("w", w, -(1 << 15), 1 << 15), _int_in("y", y, -(1 << 31), 1 << 31))
        self._bind_stream()
        _lib.check(_lib.lib().bbb_nco_set_state(self._o, C.byref(s)), "bbb_nco_set_state")

    def reset(self):
        self.state = _RESET

    def state_after(self, t, start=_RESET):
        """The registers after t clocks of the constant inputs from `start` (host arithmetic, any t < 2^64)."""
        t = _int_in("t", t, 0, 1 << 64)
        pa0, q0, w0, y0 = start
        c = self._cfg
        inc = (c.fcw + c.fm) % (1 << 24)
        rom = self.rom_table()

        def r(j):                       # R(j) = rom[adr(j)], R(-1) = q0, R(-2) = w0
            if j < 0:
                return (w0, q0)[j + 2]
            return int(rom[((((pa0 + j * inc) % (1 << 24)) >> 14) + c.pm) & 1023])
        y = y0 if t == 0 else c.am * r(t - 3)
        return NCOState((pa0 + t * inc) % (1 << 24), r(t - 1), r(t - 2), y)

    def seek(self, t):
        """Set the registers to those after t clocks from reset with the constant inputs (computed on the host)."""
        self.state = self.state_after(t)

    def acf(self, nsamples, nlags=256, chunk_samples=1 << 24, acf=None):
        """Autocorrelation counters (spectrum.capture_acf) of the next nsamples outputs with the constant inputs, generated
        chunk by chunk with each chunk's nlags - 1 samples of look-ahead: equal to capture_acf of one capture of the whole
        waveform.  Advances the registers by nsamples, as generate would.  Returns [nlags + 1] int64 (added to when given)."""
        from .spectrum import capture_acf, _acf_out
        nsamples, nlags = int(nsamples), int(nlags)
        if not 1 <= nlags <= 4096:
            raise ValueError("nlags must be 1..4096")
        look = nlags - 1
        pad = (look + 7) & ~7                 # new samples start 16-byte aligned in the buffer
        chunk = (max(int(chunk_samples), pad) + 7) & ~7
        dev = torch.device("cuda", self.device)
        acf = _acf_out(acf, nlags, dev)
        if nsamples <= 0:
            return acf
        buf = torch.empty(pad + chunk + look, dtype=torch.int16, device=dev)
        pos, keep = 0, 0                      # samples [pos, pos + keep) sit in buf[pad - keep, pad)
        while pos < nsamples:
            nfirst = min(chunk, nsamples - pos)
            more = min(nfirst + look, nsamples - pos) - keep
            if more > 0:
                self.generate(more, out=buf[pad:pad + more])
            else:
                more = 0
            capture_acf(buf[pad - keep:pad + more], nlags, nfirst, acf)
            tail = keep + more - nfirst       # samples [pos + nfirst, pos + keep + more), at most look of them
            if tail > 0:
                buf[pad - tail:pad] = buf[pad + more - tail:pad + more].clone()
            pos, keep = pos + nfirst, max(tail, 0)
        return acf

    def spectrum(self, nsamples, nlags=256, chunk_samples=1 << 24, **psd_kw):
        """(freqs, psd) of the next nsamples outputs: spectrum.psd of NCO.acf.  psd_kw: window, nfft, fs, detrend, onesided."""
        from .spectrum import psd
        return psd(self.acf(nsamples, nlags, chunk_samples), int(nsamples), **psd_kw)

    def ddc(self, taps, decim=1, phase=0, shift=0):
        """The down-converter of this oscillator's own output (ddc.DDC at its fcw): pa0 = (-3 fcw) mod 2^24 undoes the
        module's latency of 3, so that the converter's phase at sample t is the phase x(t) was made from when the waveform
        started at reset.  `taps`: a list of int16 with `shift`, or a fir.FIR."""
        from .ddc import DDC
        return DDC(self.fcw, taps, decim, phase, shift, pa0=(-3 * self.fcw) % (1 << 24), device=self.device)
