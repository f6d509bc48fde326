"""Autocorrelation counters and power spectrum of the waveform -- the lab's spectrum of a capture
(software/memdump/fftplot.py) and the spectrum analyser's view of the DAC (results/dac_tests/*_spec.png), on the GPU.

The device computes exact int64 counters (include/bbb.h, bbb_acf_accumulate_i16 / bbb_tx_acf_*):

  acf[l]     = sum_{n < count} x[n] x[n + l]    l = 0 .. nlags - 1
  acf[nlags] = sum_{n < count} x[n]

added to, so that a range may be cut into calls.  `psd(acf, count)` turns them into a spectrum on the host.

  RX.acf / RX.spectrum(samples, ...)         an int16 CUDA tensor (a capture, or TX.generate output)
  TX.acf / TX.spectrum(nsamples, ...)        the transmitter's waveform over any range, never materialised
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_LAGS = 4096           # BBB_ACF_MAX_LAGS


def _acf_out(out, nlags, dev):
    shape = (int(nlags) + 1,)
    if out is None:
        return torch.zeros(shape, dtype=torch.int64, device=dev)
    if out.dtype != torch.int64 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"acf must be a contiguous [{shape[0]}] int64 tensor on {dev}")
    return out


def capture_acf(samples, nlags=256, nfirst=None, acf=None):
    """Counters of an int16 CUDA tensor: first elements samples[0 .. nfirst) (default: all of them), partners up to the end
    of the tensor (beyond it they count as 0: with nfirst = len the biased estimate of one capture).  Adds into `acf`
    ([nlags + 1] int64 on the samples' device, allocated zeroed when None) and returns it."""
    if samples.dtype != torch.int16 or not samples.is_cuda or not samples.is_contiguous() or samples.dim() != 1:
        raise ValueError("samples must be a contiguous 1-D int16 CUDA tensor")
    navail = samples.numel()
    nfirst = navail if nfirst is None else int(nfirst)
    acf = _acf_out(acf, nlags, samples.device)
    dev = samples.device.index or 0
    _lib.check(_lib.lib().bbb_acf_accumulate_i16(C.c_void_p(samples.data_ptr()), nfirst, navail, int(nlags),
                                                 C.c_void_p(acf.data_ptr()), dev,
                                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
               "bbb_acf_accumulate_i16")
    return acf


class TxAcf(_lib.Handle):
    """bbb_tx_acf_*: counters of a TX's waveform (its settings copied at open), chunk by chunk on the generator's stream.
    Context manager; close it before the TX's generator handle goes."""
    _handle, _close = "_a", "bbb_tx_acf_close"

    def __init__(self, tx, nlags=256, warmup=16, chunk_samples=0):
        self.tx, self.nlags = tx, int(nlags)
        cfg = tx._c_cfg(warmup)
        a = C.c_void_p()
        tx.urng._bind_stream()
        _lib.check(_lib.lib().bbb_tx_acf_open(tx.urng._h, C.byref(cfg), self.nlags, int(chunk_samples), C.byref(a)),
                   "bbb_tx_acf_open")
        self._a = a

    def run(self, nsamples, first_sample=0, acf=None):
        """First elements [first_sample, first_sample + nsamples): adds into acf ([nlags + 1] int64, allocated zeroed when
        None) and returns it."""
        acf = _acf_out(acf, self.nlags, torch.device("cuda", self.tx.device))
        self.tx.urng._bind_stream()
        _lib.check(_lib.lib().bbb_tx_acf_run(self._a, int(first_sample), int(nsamples), C.c_void_p(acf.data_ptr())),
                   "bbb_tx_acf_run")
        return acf


def tx_acf(tx, nsamples, first_sample=0, nlags=256, warmup=16, chunk_samples=0, acf=None):
    """TX.acf: the [nlags + 1] int64 counters of first elements [first_sample, first_sample + nsamples)."""
    with TxAcf(tx, nlags, warmup, chunk_samples) as a:
        return a.run(nsamples, first_sample, acf)


def psd(acf, count, window="bartlett", nfft=None, fs=1.0, detrend=True, onesided=True):
    """Power spectral density from counters (Blackman-Tukey).  Pure numpy; returns (freqs, p).

    With L = len(acf) - 1 lags: mu = acf[L] / count, c[l] = acf[l] / count - (mu^2 if detrend), the lag window
    w[l] = 1 - l / L ("bartlett") or 1 ("rect"), and
        P[k] = w[0] c[0] + 2 sum_{l=1}^{L-1} w[l] c[l] cos(2 pi k l / nfft),     freqs = k fs / nfft,
    divided by fs.  nfft defaults to the smallest power of two >= 2L.  onesided: bins 0 .. nfft/2, with bins 1 .. nfft/2 - 1
    doubled; else all nfft bins.  The Bartlett form is the expected averaged periodogram of length-L segments (what a spectrum
    analyser shows with averaging on): in expectation each segment's |FFT|^2 / L equals it, and the expectation is never
    negative.  An estimate from a finite record (partners past the first elements, the mean removed) can still dip below
    zero in bins where the true spectrum is close to zero.  The rect form with L = count is the periodogram
    |rfft(x, nfft)|^2 / count of the whole record."""
    a = acf.cpu().numpy() if isinstance(acf, torch.Tensor) else np.asarray(acf)
    a = a.astype(np.float64)
    L = len(a) - 1
    if L < 1:
        raise ValueError("acf needs at least one lag and the sum")
    if count <= 0:
        raise ValueError("count must be positive")
    if window == "bartlett":
        w = 1.0 - np.arange(L) / L
    elif window == "rect":
        w = np.ones(L)
    else:
        raise ValueError("window must be 'bartlett' or 'rect'")
    nfft = 1 << int(np.ceil(np.log2(2 * L))) if nfft is None else int(nfft)
    if nfft < 2:
        raise ValueError("nfft must be >= 2")
    mu = a[L] / count
    c = a[:L] / count - (mu * mu if detrend else 0.0)
    y = w * c
    nbins = nfft // 2 + 1 if onesided else nfft
    k = np.arange(nbins, dtype=np.int64)
    l = np.arange(1, L, dtype=np.int64)
    table = np.cos(2 * np.pi * np.arange(nfft) / nfft)
    p = np.empty(nbins)
    for lo in range(0, nbins, 256):                     # cos(2 pi ((k l) mod nfft) / nfft), rows of 256 bins at a time
        kk = k[lo:lo + 256, None]
        p[lo:lo + 256] = y[0] + 2.0 * (table[(kk * l[None, :]) % nfft] @ y[1:])
    p /= fs
    if onesided and nfft > 2:
        p[1:nfft // 2] *= 2.0
    return k * (fs / nfft), p
