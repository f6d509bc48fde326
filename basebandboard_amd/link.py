"""The filtered link: eye, bathtub and BER sweep of the transmitter's waveform BEHIND a receive filter (include/bbb.h,
bbb_link_sweep_*) -- the question gateware/bbb/rx.py:24-26 leaves open (`MovingAverage(sample)`, commented out), at scale.

`TX.eye` and `TX.ber_sweep` decide on the raw sample x(n).  Here the decision is made on the filtered stream

    acc(n) = sum_i h[i] * x(n - i)        z(n) = sat16(acc(n) >> shift)        stream sample n: acc / z at n + delay

(`delay` re-times the stream by the filter's group delay: by default `FIR.design_delay` of a designed filter, else `FIR.delay()`), with the threshold in units of acc as
`FIR.slice` takes it, and the eye histogram bins z.  `LinkSweep(tx, settings, rx_filter).run(n)` gives the bathtub (and,
with `eye=`, the histogram) of every setting in one pass over the noise stream; neither the waveform nor the filtered
stream reaches memory.  `TX.eye(..., rx_filter=)` and `TX.ber_sweep(..., rx_filter=)` go through it.
"""
import ctypes as C

import torch

from . import _lib
from .eye import ROWS, _counters
from .tx import _shaper
from .txsweep import TxSetting, _c_setting

MAX_DELAY = 255


class LinkSweep(_lib.Handle):
    """bbb_link_sweep_*: bathtub and eye of a TX's waveform behind `rx_filter` (a fir.FIR) for many settings at once, chunk by
    chunk on the generator's stream.  The TX supplies the source, the PRBS and the generator, each txsweep.TxSetting the
    rest (its threshold is in units of acc).  delay None: rx_filter.design_delay where a design set it (FIR.mmse), else rx_filter.delay().  eye: an eye.EyeConfig for histograms of z
    (ncols, shift, col_origin; its threshold / strict are not used).  Context manager; close it before the TX's generator
    handle goes."""
    _handle, _close = "_s", "bbb_link_sweep_close"

    def __init__(self, tx, settings, rx_filter, delay=None, eye=None, warmup=16, chunk_samples=0):
        self.tx, self.eye = tx, eye
        self.settings = list(settings)
        if not self.settings:
            raise ValueError("at least one setting")
        if delay is None:                  # a designed filter knows its own re-timing; any other filter gives its centroid
            design = getattr(rx_filter, "design_delay", None)
            delay = rx_filter.delay() if design is None else design
        self.delay = int(delay)
        if not 0 <= self.delay < 1 << 32:
            raise ValueError("delay must be 0..255")
        base = tx._c_cfg(warmup)
        arr = (_lib.TxSetting * len(self.settings))(*[_c_setting(tx, s) for s in self.settings])
        fir = rx_filter._cfg(1, 0)
        ec = eye._c() if eye is not None else None
        h = C.c_void_p()
        tx.urng._bind_stream()
        _lib.check(_lib.lib().bbb_link_sweep_open(tx.urng._h, C.byref(base), arr, len(self.settings), C.byref(fir), self.delay,
                                                  C.byref(ec) if ec is not None else None, int(chunk_samples), C.byref(h)),
                   "bbb_link_sweep_open")
        self._s = h

    def run(self, nsamples, first_sample=0, counters=None, hist=None):
        """Stream samples [first_sample, first_sample + nsamples): adds into counters ([nset, 8, 2] uint64 = bits, errors per
        setting and phase) and, when `eye` was given, hist ([nset, 256, ncols] uint64), each allocated zeroed when None.
        Returns counters, or (counters, hist) when `eye` was given."""
        dev = torch.device("cuda", self.tx.device)
        nset = len(self.settings)
        counters = _counters(counters, (nset, 8, 2), dev, "counters")
        if self.eye is not None:
            hist = _counters(hist, (nset, ROWS, int(self.eye.ncols)), dev, "hist")
        elif hist is not None:
            raise ValueError("hist needs the eye= of LinkSweep")
        self.tx.urng._bind_stream()
        _lib.check(_lib.lib().bbb_link_sweep_run(self._s, int(first_sample), int(nsamples), C.c_void_p(counters.data_ptr()),
                                                 C.c_void_p(hist.data_ptr() if hist is not None else None)),
                   "bbb_link_sweep_run")
        return counters if self.eye is None else (counters, hist)


def link_eye(tx, nsamples, rx_filter, delay=None, first_sample=0, warmup=16, eye=None, chunk_samples=0, hist=None, bathtub=None):
    """TX.eye with a receive filter: (hist [256, ncols], bathtub [8, 2]) of the filtered stream of the TX's own setting; the
    eye's threshold / strict decide, in units of acc."""
    from .eye import BIT_SAMPLE0, EyeConfig
    eye = eye or EyeConfig(col_origin=BIT_SAMPLE0)
    dev = torch.device("cuda", tx.device)
    hist = _counters(hist, (ROWS, int(eye.ncols)), dev, "hist")
    bathtub = _counters(bathtub, (8, 2), dev, "bathtub")
    st = TxSetting(noise_var=tx.noise_var, bit_en=tx.bit_en, noise_en=tx.noise_en, threshold=eye.threshold, strict=eye.strict)
    with LinkSweep(tx, [st], rx_filter, delay, eye, warmup, chunk_samples) as s:
        s.run(nsamples, first_sample, bathtub.view(1, 8, 2), hist.view(1, ROWS, int(eye.ncols)))
    return hist, bathtub


def link_ber_sweep(tx, nsamples, rx_filter, delay=None, noise_vars=range(16), shape_sels=None, threshold=0, strict=False,
                   first_sample=0, warmup=16, chunk_samples=0, counters=None):
    """TX.ber_sweep with a receive filter: the filtered stream's bathtub for every (shape_sel, noise_var) of the grid."""
    if shape_sels is None:
        shape_sels = [_shaper(tx).setsel]
    shape_sels, noise_vars = [int(s) for s in shape_sels], [int(v) for v in noise_vars]
    settings = [TxSetting(shape_sel=s, noise_var=v, bit_en=tx.bit_en, noise_en=tx.noise_en, threshold=threshold, strict=strict)
                for s in shape_sels for v in noise_vars]
    shape = (len(shape_sels), len(noise_vars), 8, 2)
    if counters is not None:
        counters = _counters(counters, shape, torch.device("cuda", tx.device), "counters")
    with LinkSweep(tx, settings, rx_filter, delay, None, warmup, chunk_samples) as s:
        flat = s.run(nsamples, first_sample, None if counters is None else counters.view(len(settings), 8, 2))
    return flat.view(shape)
