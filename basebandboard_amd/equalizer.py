"""Pulse response and receive-filter design -- what a link tester does before it judges a link: correlate the received
samples with the known data bits, read the link's pulse response off the result, and derive the receive filter from it.

The device computes exact int64 counters (include/bbb.h, bbb_xcorr_accumulate_i16 / bbb_tx_xcorr_*): with `spb` samples per
data bit, bit m >= 0 of sign s[m] = +1 / -1, absolute sample numbers n and `origin` the sample at which bit 0 has lag 0,

  xc[l] = sum of s[m] x[n]   over the samples n of the range with n - origin - l = spb * m, m >= 0        l = 0 .. nlags - 1

added to, so that a range may be cut into calls.  Everything else is host arithmetic in numpy:

  xcorr_counts(...)                          the number of terms of every lag (closed form)
  pulse_response(xc, counts)                 h[l] = xc[l] / counts[l]: the estimate of the link's pulse response
  noise_power(acf0, count, h, spb)           what of the waveform's power the pulse response does not explain
  mmse_taps(h, spb, cursor, ntaps, sigma2)   the MMSE feed-forward filter for white +-1 data, as int16 taps for fir.FIR

The closed loop: measure with TX.pulse_response / RX.pulse_response, design with mmse_taps (FIR.mmse), apply with fir.FIR,
verify with link.LinkSweep.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_LAGS = 1024           # BBB_XCORR_MAX_LAGS
TX_BIT_ORIGIN = 17        # BBB_TX_BIT_ORIGIN: lag l of the transmitter's waveform lines up with coefficients[l]
TX_SPB = 8


def _xc_out(out, nlags, dev):
    shape = (int(nlags),)
    if out is None:
        return torch.zeros(shape, dtype=torch.int64, device=dev)
    if out.dtype != torch.int64 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"xcorr must be a contiguous [{shape[0]}] int64 tensor on {dev}")
    return out


def capture_xcorr(samples, bits, spb, origin, nlags, first_sample=0, bit0=0, xcorr=None):
    """Counters of an int16 CUDA tensor against packed data bits: samples[i] is sample number first_sample + i, `bits` a
    contiguous int64 CUDA tensor that holds data bits bit0 .. bit0 + 64 * len(bits) - 1 LSB first (PRBS.generate's layout).
    Adds into `xcorr` ([nlags] int64 on the samples' device, allocated zeroed when None) and returns it.  A bit range that
    does not cover what the samples need is a ValueError."""
    if samples.dtype != torch.int16 or not samples.is_cuda or not samples.is_contiguous() or samples.dim() != 1:
        raise ValueError("samples must be a contiguous 1-D int16 CUDA tensor")
    if bits.dtype != torch.int64 or not bits.is_contiguous() or bits.dim() != 1 or bits.device != samples.device:
        raise ValueError("bits must be a contiguous 1-D int64 tensor on the samples' device")
    xcorr = _xc_out(xcorr, nlags, samples.device)
    dev = samples.device.index or 0
    cfg = _lib.XcorrCfg(int(spb), int(nlags), int(origin))
    _lib.check(_lib.lib().bbb_xcorr_accumulate_i16(C.c_void_p(samples.data_ptr()), samples.numel(), int(first_sample),
                                                   C.c_void_p(bits.data_ptr()), int(bit0), 64 * bits.numel(), C.byref(cfg),
                                                   C.c_void_p(xcorr.data_ptr()), dev,
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
               "bbb_xcorr_accumulate_i16")
    return xcorr


class TxXcorr(_lib.Handle):
    """bbb_tx_xcorr_*: counters of a TX's waveform against its own data bits (its settings copied at open; spb 8, origin
    TX_BIT_ORIGIN), chunk by chunk on the generator's stream.  Context manager; close it before the TX's generator handle
    goes."""
    _handle, _close = "_x", "bbb_tx_xcorr_close"

    def __init__(self, tx, nlags=64, warmup=16, chunk_samples=0):
        self.tx, self.nlags = tx, int(nlags)
        cfg = tx._c_cfg(warmup)
        x = C.c_void_p()
        tx.urng._bind_stream()
        _lib.check(_lib.lib().bbb_tx_xcorr_open(tx.urng._h, C.byref(cfg), self.nlags, int(chunk_samples), C.byref(x)),
                   "bbb_tx_xcorr_open")
        self._x = x

    def run(self, nsamples, first_sample=0, xcorr=None):
        """Samples [first_sample, first_sample + nsamples): adds into xcorr ([nlags] int64, allocated zeroed when None) and
        returns it."""
        xcorr = _xc_out(xcorr, self.nlags, torch.device("cuda", self.tx.device))
        self.tx.urng._bind_stream()
        _lib.check(_lib.lib().bbb_tx_xcorr_run(self._x, int(first_sample), int(nsamples), C.c_void_p(xcorr.data_ptr())),
                   "bbb_tx_xcorr_run")
        return xcorr


def tx_xcorr(tx, nsamples, first_sample=0, nlags=64, warmup=16, chunk_samples=0, xcorr=None):
    """The [nlags] int64 counters of a TX's samples [first_sample, first_sample + nsamples)."""
    with TxXcorr(tx, nlags, warmup, chunk_samples) as x:
        return x.run(nsamples, first_sample, xcorr)


def xcorr_counts(first_sample, nsamples, spb, origin, nlags):
    """The number of terms of every lag: the samples n in [first_sample, first_sample + nsamples) with n = origin + l modulo
    spb and n >= origin + l.  int64 numpy array of nlags entries."""
    first, n, spb, origin = int(first_sample), int(nsamples), int(spb), int(origin)
    start = origin + np.arange(int(nlags), dtype=np.int64)        # the first sample of lag l: bit 0
    low = np.maximum(start, first)
    n0 = low + (start - low) % spb                                # the first sample of the lag's residue at or above both
    return np.maximum(0, (first + n - n0 + spb - 1) // spb).astype(np.int64)


def pulse_response(xc, counts):
    """xc / counts as float64, 0 where a lag has no term."""
    a = xc.cpu().numpy() if isinstance(xc, torch.Tensor) else np.asarray(xc)
    a, c = a.astype(np.float64), np.asarray(counts, dtype=np.float64)
    if a.shape != c.shape:
        raise ValueError("xc and counts must have the same length")
    return np.divide(a, c, out=np.zeros_like(a), where=c > 0)


def noise_power(acf0, count, h, spb):
    """The noise power per sample of a waveform of white +-1 data through pulse response `h`: its mean square acf0 / count
    (acf0 the lag-0 counter of capture_acf / TxAcf over `count` samples) less the data's share sum(h^2) / spb, clamped at
    0."""
    if count <= 0:
        raise ValueError("count must be positive")
    h = np.asarray(h, dtype=np.float64)
    return max(0.0, float(acf0) / float(count) - float((h * h).sum()) / int(spb))


def _mmse_system(h, spb, cursor, ntaps, noise_power, nfb=0):
    h = np.asarray(h, dtype=np.float64)
    L, spb, cursor, ntaps = len(h), int(spb), int(cursor), int(ntaps)
    # G[i, k] = h[cursor - i + spb * k] over every bit offset k at which some tap sees the pulse (0 outside its lags)
    k = np.arange(-((cursor + spb - 1) // spb) - 1, (L + ntaps) // spb + 2, dtype=np.int64)
    idx = cursor - np.arange(ntaps, dtype=np.int64)[:, None] + spb * k[None, :]
    G = np.where((idx >= 0) & (idx < L), h[np.clip(idx, 0, L - 1)], 0.0)
    p = G[:, int(np.flatnonzero(k == 0)[0])]
    G = G[:, (k < 1) | (k > int(nfb))]           # the nfb bits in front of the cursor's are the feedback's to remove
    R = G @ G.T + float(noise_power) * np.eye(ntaps)
    return R, p


def mmse_taps(h, spb, cursor, ntaps, noise_power, scale_bits=8):
    """The model-based MMSE feed-forward receive filter for white +-1 data: (taps, delay), taps an int16 numpy array.

    Bit m is decided from acc(t) = sum_i taps[i] x(t - i) at t = origin + spb * m + cursor: tap 0 sees lag `cursor` of the
    pulse, tap i lag cursor - i, and beside bit m the sample x(t - i) carries bit m - k through h[cursor - i + spb * k].  So
        R[i][j] = sum_k h[cursor - i + spb k] h[cursor - j + spb k] + noise_power [i == j]      p[i] = h[cursor - i]
    (h = 0 outside its lags), R w = p, and taps = round(w * 2^scale_bits / max |w|) clipped to int16 (a singular R, as
    with noise_power 0 and a pulse that some taps never see, takes the least-squares solution of least norm).

    Sign and delay: the filter is causal, fir.FIR's acc(n) = sum_i taps[i] x(n - i), so it can only decide bit m at or after
    the sample the unfiltered decision uses, origin + spb * m + peak with peak = argmax |h|; cursor >= peak is required and
    delay = cursor - peak.  That is the `delay` of link.LinkSweep (its stream sample n is acc(n + delay)): with it the
    filtered bathtub's best phase is the unfiltered one's.  FIR.delay() is the centroid of |taps| instead; for a filter whose
    largest tap answers the peak (tap cursor - peak) the two agree to within the taps' asymmetry, and the centroid is what
    remains when no pulse response is known."""
    return _mmse_design(h, spb, cursor, ntaps, noise_power, scale_bits, 0)


def _mmse_design(h, spb, cursor, ntaps, noise_power, scale_bits, nfb):
    h = np.asarray(h, dtype=np.float64)
    spb, cursor, ntaps = int(spb), int(cursor), int(ntaps)
    if h.ndim != 1 or len(h) == 0 or not np.abs(h).max() > 0:
        raise ValueError("h must be a 1-D pulse response with a nonzero lag")
    if spb < 1 or not 1 <= ntaps <= 256:
        raise ValueError("spb must be >= 1 and ntaps 1..256")
    if noise_power < 0 or not 0 <= int(scale_bits) <= 15:
        raise ValueError("noise_power must be >= 0 and scale_bits 0..15")
    peak = int(np.abs(h).argmax())
    if not peak <= cursor < len(h) + ntaps - 1:
        raise ValueError(f"cursor must be {peak} (the pulse's peak) .. {len(h) + ntaps - 2}")
    R, p = _mmse_system(h, spb, cursor, ntaps, noise_power, nfb)
    try:
        w = np.linalg.solve(R, p)
    except np.linalg.LinAlgError:
        w = np.linalg.lstsq(R, p, rcond=None)[0]
    if not np.isfinite(w).all() or not np.abs(w).max() > 0:
        w = np.linalg.lstsq(R, p, rcond=None)[0]
    if not np.abs(w).max() > 0:
        raise ValueError("no tap sees the pulse: move the cursor or lengthen the filter")
    taps = np.clip(np.rint(w * (1 << int(scale_bits)) / np.abs(w).max()), -32768, 32767).astype(np.int16)
    return taps, cursor - peak


def dfe_taps(h, spb, cursor, nff, nfb, noise_power, scale_bits=8):
    """The MMSE decision-feedback design for white +-1 data: (ff, fb, delay) for dfe.DFE.

    The feed-forward filter is mmse_taps' system R w = p with the nfb bits in front of the cursor's taken out of the
    interference (bit m - k reaches tap i through h[cursor - i + spb k]; k = 1 .. nfb are decided already and the feedback
    removes them), scaled to int16 taps the same way.  The feedback taps are what the INTEGER feed-forward filter makes of
    those bits, fb[i] = round(sum_j ff[j] h[cursor - j + spb (i + 1)]), so they are in units of the filter's acc and undo
    exactly what the filter that runs lets through.  fb is an int64 numpy array of nfb entries; nfb = 0 gives mmse_taps'
    taps.  delay as in mmse_taps."""
    nfb = int(nfb)
    if not 0 <= nfb <= 4:
        raise ValueError("nfb must be 0..4")
    ff, delay = _mmse_design(h, spb, cursor, nff, noise_power, scale_bits, nfb)
    h = np.asarray(h, dtype=np.float64)
    idx = int(cursor) - np.arange(len(ff), dtype=np.int64)[None, :] + int(spb) * np.arange(1, nfb + 1, dtype=np.int64)[:, None]
    post = np.where((idx >= 0) & (idx < len(h)), h[np.clip(idx, 0, len(h) - 1)], 0.0)
    fb = np.rint(post @ ff.astype(np.float64)).astype(np.int64)
    return ff, fb, delay


def mlse_target(h, spb, cursor, nff, mem, noise_power, shift=None, scale_bits=8):
    """Filter and target for mlse.MLSE from the MMSE decision-feedback design: (ff, g, shift).

    ff is dfe_taps' feed-forward filter with `mem` feedback taps: it leaves the cursor and the mem bits behind it and
    suppresses the rest, which is the shortened channel a sequence detector wants.  The target is what the INTEGER filter
    makes of those bits, in units of y = acc >> shift: g[0] = round(sum_j ff[j] h[cursor - j] / 2^shift), g[i] =
    round(fb[i - 1] / 2^shift).  shift None: the smallest with sum |g| <= 16383, which leaves a noiseless y a factor of two
    of headroom in int16.  g is an int64 numpy array of mem + 1 entries."""
    mem = int(mem)
    if not 1 <= mem <= 4:
        raise ValueError("mem must be 1..4")
    ff, fb, _ = dfe_taps(h, spb, cursor, nff, mem, noise_power, scale_bits)
    h = np.asarray(h, dtype=np.float64)
    idx = int(cursor) - np.arange(len(ff), dtype=np.int64)
    main = float(np.where((idx >= 0) & (idx < len(h)), h[np.clip(idx, 0, len(h) - 1)], 0.0) @ ff.astype(np.float64))
    raw = np.concatenate([[main], fb.astype(np.float64)])

    def target(s):
        return np.rint(raw / float(1 << s)).astype(np.int64)

    if shift is None:
        shift = next((s for s in range(32) if int(np.abs(target(s)).sum()) <= 16383), None)
        if shift is None:
            raise ValueError("no shift of 0..31 brings sum |g| to 16383")
    shift = int(shift)
    if not 0 <= shift <= 31:
        raise ValueError("shift must be 0..31")
    return ff, target(shift), shift


def tx_pulse_response(tx, nsamples, nlags=64, first_sample=0, warmup=16, chunk_samples=0):
    """TX.pulse_response: the float64 estimate h[0 .. nlags) of the transmitter's pulse response over a sample range; lag l
    lines up with coefficients[l]."""
    xc = tx_xcorr(tx, nsamples, first_sample, nlags, warmup, chunk_samples)
    return pulse_response(xc, xcorr_counts(first_sample, nsamples, TX_SPB, TX_BIT_ORIGIN, nlags))


def rx_pulse_response(samples, bits, spb, origin, nlags=None, first_sample=0, bit0=0):
    """RX.pulse_response: the estimate from a capture and its packed reference bits; nlags None: 8 * spb."""
    nlags = 8 * int(spb) if nlags is None else int(nlags)
    xc = capture_xcorr(samples, bits, spb, origin, nlags, first_sample, bit0)
    return pulse_response(xc, xcorr_counts(first_sample, samples.numel(), spb, origin, nlags))
