"""Transmitter output stream -- host-side mirror of gateware/bbb/tx.py.

`TX(prbs_k, bit_en, src_sel, shape_sel, noise_en, noise_var)` takes the reference's arguments
(tx.py:39-52).  Its output is the shaped data bits (PRBS-k or the pulse source) plus the CLT noise
stream scaled by `noise_var`, each gated by its enable, as 12-bit signed samples at 8 per data bit.
`generate` fills a tensor with that stream on the GPU.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .bitshaper import PRBSShaper, Pulser, _cfg
from .prbs import PRBS
from .rng import CLTGRNG, LUTOPT


def _shaper(tx):
    """The shaper whose output is the waveform (tx.py:65).  The one place where the selection is made."""
    return tx.pulse_shaper if tx.src_sel else tx.prbs_shaper


class TX:
    def __init__(self, prbs_k, bit_en, src_sel, shape_sel, noise_en, noise_var, device=0, init=1, prbs_init=1):
        self.betas = np.linspace(0, 1, 32).tolist()                      # tx.py:54
        self.prbs = PRBS(prbs_k, init=prbs_init, device=device)           # tx.py:55 (raises ValueError on a bad k)
        self.prbs_shaper = PRBSShaper.from_rcf(self.prbs, shape_sel, self.betas)
        self.pulse = Pulser()
        self.pulse_shaper = PRBSShaper.from_rcf(self.pulse, shape_sel, self.betas)
        self.urng = LUTOPT.shipped(256, init=init, device=device)         # tx.py:70: the n256 recurrence
        self.grng = CLTGRNG(self.urng)
        if not 0 <= int(noise_var) <= 15:
            raise ValueError("noise_var is a 4-bit unsigned value")      # tx.py:52
        self.bit_en, self.src_sel, self.noise_en, self.noise_var = bool(bit_en), int(src_sel), bool(noise_en), int(noise_var)
        self.device = int(device)

    def _c_cfg(self, warmup):
        """The bbb_tx_cfg of this transmitter: what generate and every analyser of its waveform hand the library."""
        sh = _shaper(self)
        return _cfg(sh.coefficients[sh.setsel], sh.prbs, self.bit_en, self.noise_en, self.noise_var, warmup)

    def generate(self, nsamples, first_sample=0, warmup=16, out=None, stream_on=True):
        """Samples first_sample .. first_sample + nsamples - 1 of `x` (int16, 12-bit signed).
        stream_on: announce that the next call continues where this one ends (bbb_awgn_prefetch), so that the
        noise generator's start states for it are derived beside this call's kernels; a call that does not
        continue there simply ignores the hint."""
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty(int(nsamples), dtype=torch.int16, device=dev)
        if out.dtype != torch.int16 or out.numel() < nsamples or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out must be a contiguous int16 tensor on {dev} with >= nsamples elements")
        cfg = self._c_cfg(warmup)
        self.urng._bind_stream()
        _lib.check(_lib.lib().bbb_tx_fill_i16(self.urng._h, C.byref(cfg), C.c_void_p(out.data_ptr()), int(nsamples),
                                              int(first_sample)), "bbb_tx_fill_i16")
        if stream_on and self.noise_en:
            _lib.check(_lib.lib().bbb_awgn_prefetch(self.urng._h, int(nsamples), int(warmup) + int(first_sample) + int(nsamples)),
                       "bbb_awgn_prefetch")
        return out[:nsamples]

    def eye(self, nsamples, first_sample=0, warmup=16, eye=None, chunk_samples=0, hist=None, bathtub=None, rx_filter=None,
            delay=None):
        """Eye histogram and bathtub of `x` over samples [first_sample, first_sample + nsamples), the waveform never
        materialised (bbb_tx_eye_*): (hist [256, ncols] uint64, bathtub [8, 2] uint64 = bits, errors per phase).  `eye`: an
        eye.EyeConfig, default 64 columns, shift 4 and col_origin = eye.BIT_SAMPLE0 (column c is bathtub phase c mod 8).
        hist / bathtub given: added to.  rx_filter: a fir.FIR -- eye and bathtub of the stream behind that filter instead,
        re-timed by `delay` (None: the filter's design_delay where FIR.mmse set one, else rx_filter.delay()); the histogram bins sat16(acc >> shift), the bathtub decides acc
        against the eye's threshold in units of acc (bbb_link_sweep_*, link.py)."""
        if rx_filter is not None:
            from .link import link_eye
            return link_eye(self, nsamples, rx_filter, delay, first_sample, warmup, eye, chunk_samples, hist, bathtub)
        if delay is not None:
            raise ValueError("delay belongs to rx_filter")
        from .eye import tx_eye
        return tx_eye(self, nsamples, first_sample, warmup, eye, chunk_samples, hist, bathtub)

    def acf(self, nsamples, first_sample=0, nlags=256, warmup=16, chunk_samples=0, acf=None):
        """Autocorrelation counters of `x` (bbb_tx_acf_*), the waveform never materialised: [nlags + 1] int64, acf[l] = sum
        of x[n] x[n + l] over first elements n in [first_sample, first_sample + nsamples), acf[nlags] = sum of those x[n].
        Added to when given."""
        from .spectrum import tx_acf
        return tx_acf(self, nsamples, first_sample, nlags, warmup, chunk_samples, acf)

    def spectrum(self, nsamples, first_sample=0, nlags=256, warmup=16, chunk_samples=0, **psd_kw):
        """(freqs, psd) of `x` over nsamples first elements: spectrum.psd of TX.acf (Bartlett lag window by default: what
        the spectrum analyser shows with averaging).  The noise generator's own spectrum is that of
        TX(k, bit_en=0, src_sel=0, shape_sel, noise_en=1, noise_var=1): the waveform is then wrap12(g * 1) = g.
        psd_kw: window, nfft, fs, detrend, onesided."""
        from .spectrum import psd, tx_acf
        return psd(tx_acf(self, nsamples, first_sample, nlags, warmup, chunk_samples), int(nsamples), **psd_kw)

    def pulse_response(self, nsamples, nlags=64, first_sample=0, warmup=16, chunk_samples=0):
        """The pulse response of `x` measured against the transmitter's own data bits over samples [first_sample,
        first_sample + nsamples), the waveform never materialised (bbb_tx_xcorr_*, equalizer.py): float64 [nlags], lag l
        lining up with the shaper's coefficients[l].  What equalizer.mmse_taps / FIR.mmse design a receive filter from."""
        from .equalizer import tx_pulse_response
        return tx_pulse_response(self, nsamples, nlags, first_sample, warmup, chunk_samples)

    def ber_sweep(self, nsamples, noise_vars=range(16), shape_sels=None, threshold=0, strict=False, first_sample=0, warmup=16,
                  chunk_samples=0, counters=None, rx_filter=None, delay=None):
        """Bathtub of `x` for every (shape_sel, noise_var) of the grid in one pass over the noise stream
        (bbb_tx_ber_sweep_*): [len(shape_sels), len(noise_vars), 8, 2] uint64 = bits, errors per phase, each entry what
        TX.eye's bathtub gives for a TX with that shape_sel and noise_var.  shape_sels None: the TX's own set; bit_en and
        noise_en are the TX's; the decision x >= threshold (x > threshold when strict).  counters given: added to.
        rx_filter: a fir.FIR -- the bathtub of the stream behind that filter instead, re-timed by `delay` (None: the
        filter's design_delay where FIR.mmse set one, else rx_filter.delay()), the threshold then in units of acc (bbb_link_sweep_*, link.py)."""
        from .txsweep import tx_ber_sweep
        return tx_ber_sweep(self, nsamples, noise_vars, shape_sels, threshold, strict, first_sample, warmup, chunk_samples,
                            counters, rx_filter, delay)

    def stream(self, nsamples_per_call, first_sample=0, warmup=16):
        """TX.x read sequentially (bbb_tx_stream_*): `with tx.stream(n) as s: s.next(out=buf)`."""
        return WaveformStream(self, nsamples_per_call, first_sample, warmup)


class WaveformStream(_lib.Handle):
    """bbb_tx_stream_*: the transmitter's waveform read sequentially in equal calls; the library turns the two-kernel
    form on and announces every next call.  The TX object's settings are copied when the stream is opened.  Context
    manager; closing restores the generator handle's mode."""
    _handle, _close = "_s", "bbb_tx_stream_close"

    def __init__(self, tx, nsamples_per_call, first_sample=0, warmup=16):
        self.tx, self.n = tx, int(nsamples_per_call)
        cfg = tx._c_cfg(warmup)
        s = C.c_void_p()
        tx.urng._bind_stream()
        _lib.check(_lib.lib().bbb_tx_stream_open(tx.urng._h, C.byref(cfg), self.n, int(first_sample), C.byref(s)), "bbb_tx_stream_open")
        self._s = s

    def _out(self, n, out):
        dev = torch.device("cuda", self.tx.device)
        if out is None:
            out = torch.empty(n, dtype=torch.int16, device=dev)
        if out.dtype != torch.int16 or out.numel() < n or not out.is_contiguous() or out.device != dev:
            raise ValueError(f"out must be a contiguous int16 tensor on {dev} with >= {n} elements")
        self.tx.urng._bind_stream()
        return out

    def next(self, out=None):
        out = self._out(self.n, out)
        _lib.check(_lib.lib().bbb_tx_stream_next(self._s, C.c_void_p(out.data_ptr())), "bbb_tx_stream_next")
        return out[:self.n]

    def read(self, nsamples, out=None):
        n = int(nsamples)
        out = self._out(n, out)
        _lib.check(_lib.lib().bbb_tx_stream_read(self._s, C.c_void_p(out.data_ptr()), n), "bbb_tx_stream_read")
        return out[:n]

    def seek(self, first_sample):
        _lib.check(_lib.lib().bbb_tx_stream_seek(self._s, int(first_sample)), "bbb_tx_stream_seek")

    def tell(self):
        v = C.c_uint64()
        _lib.check(_lib.lib().bbb_tx_stream_tell(self._s, C.byref(v)), "bbb_tx_stream_tell")
        return v.value

