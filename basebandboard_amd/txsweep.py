"""BER of the shaped link over many transmitter settings in one pass (include/bbb.h, bbb_tx_ber_sweep_*).

The board's transmitter has knobs -- the raised-cosine set `shape_sel` (32 roll-offs, tx.py:54), `noise_var` (0..15,
tx.py:52), `bit_en` / `noise_en` -- and the receiver decides at one of 8 sampling phases against a threshold.  The noise
sample and the data bit of a sample do not depend on those knobs, so one pass over the noise stream serves every setting:
`TxBerSweep(tx, settings).run(n)` gives, for each setting, exactly the bathtub (bits, errors per phase) that `TX.eye` gives
for a TX with that setting, and `TX.ber_sweep` does it for the shape_sel x noise_var grid.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _lib
from .eye import _counters
from .tx import _shaper


@dataclass
class TxSetting:
    """One setting (bbb_tx_setting): the coefficient set is `coeffs` (64 integers) when given, else set `shape_sel` of the
    TX's shaper (its own set when None); noise_var 0..15; the decision x >= threshold, or x > threshold when strict."""
    shape_sel: Optional[int] = None
    noise_var: int = 8
    bit_en: bool = True
    noise_en: bool = True
    threshold: int = 0
    strict: bool = False
    coeffs: Optional[Sequence[int]] = None


def _c_setting(tx, s):
    sh = _shaper(tx)
    coeffs = s.coeffs
    if coeffs is None:
        sel = sh.setsel if s.shape_sel is None else int(s.shape_sel)
        if not 0 <= sel < len(sh.coefficients):
            raise ValueError(f"shape_sel must be 0..{len(sh.coefficients) - 1}")
        coeffs = sh.coefficients[sel]
    if len(coeffs) != 64:
        raise ValueError("a coefficient set has 64 entries (8 per bit duration, bitshaper.py:19-21)")
    c = _lib.TxSetting()
    for i, v in enumerate(coeffs):
        c.coeffs[i] = int(v)        # range checked by the library (EINVAL -> ValueError)
    c.bit_en, c.noise_en, c.noise_var = int(bool(s.bit_en)), int(bool(s.noise_en)), int(s.noise_var)
    c.threshold, c.strict, c.reserved = int(s.threshold), int(bool(s.strict)), 0
    return c


class TxBerSweep(_lib.Handle):
    """bbb_tx_ber_sweep_*: the bathtub of a TX's waveform for many settings at once, chunk by chunk on the generator's
    stream.  The TX supplies the source (PRBS or Pulser, tx.src_sel), the PRBS and the generator; each setting supplies the
    rest.  Context manager; close it before the TX's generator handle goes."""
    _handle, _close = "_s", "bbb_tx_ber_sweep_close"

    def __init__(self, tx, settings, warmup=16, chunk_samples=0):
        self.tx = tx
        self.settings = list(settings)
        if not self.settings:
            raise ValueError("at least one setting")
        base = tx._c_cfg(warmup)
        arr = (_lib.TxSetting * len(self.settings))(*[_c_setting(tx, s) for s in self.settings])
        h = C.c_void_p()
        tx.urng._bind_stream()
        _lib.check(_lib.lib().bbb_tx_ber_sweep_open(tx.urng._h, C.byref(base), arr, len(self.settings), int(chunk_samples),
                                                    C.byref(h)), "bbb_tx_ber_sweep_open")
        self._s = h

    def run(self, nsamples, first_sample=0, counters=None):
        """Samples [first_sample, first_sample + nsamples): adds into counters ([nset, 8, 2] uint64 = bits, errors per
        setting and phase; allocated zeroed when None) and returns it."""
        dev = torch.device("cuda", self.tx.device)
        counters = _counters(counters, (len(self.settings), 8, 2), dev, "counters")
        self.tx.urng._bind_stream()
        _lib.check(_lib.lib().bbb_tx_ber_sweep_run(self._s, int(first_sample), int(nsamples), C.c_void_p(counters.data_ptr())),
                   "bbb_tx_ber_sweep_run")
        return counters


def tx_ber_sweep(tx, nsamples, noise_vars=range(16), shape_sels=None, threshold=0, strict=False, first_sample=0, warmup=16,
                 chunk_samples=0, counters=None, rx_filter=None, delay=None):
    """TX.ber_sweep: the bathtub for every (shape_sel, noise_var) of the grid, [len(shape_sels), len(noise_vars), 8, 2]
    uint64 (bits, errors).  shape_sels None: the TX's own set.  bit_en and noise_en are the TX's.  rx_filter (a fir.FIR):
    the bathtub behind that filter, through link.LinkSweep."""
    if rx_filter is not None:
        from .link import link_ber_sweep
        return link_ber_sweep(tx, nsamples, rx_filter, delay, noise_vars, shape_sels, threshold, strict, first_sample, warmup,
                              chunk_samples, counters)
    if delay is not None:
        raise ValueError("delay belongs to rx_filter")
    if shape_sels is None:
        shape_sels = [_shaper(tx).setsel]
    shape_sels, noise_vars = [int(s) for s in shape_sels], [int(v) for v in noise_vars]
    settings = [TxSetting(shape_sel=s, noise_var=v, bit_en=tx.bit_en, noise_en=tx.noise_en, threshold=threshold, strict=strict)
                for s in shape_sels for v in noise_vars]
    shape = (len(shape_sels), len(noise_vars), 8, 2)
    if counters is not None:
        counters = _counters(counters, shape, torch.device("cuda", tx.device), "counters")
    with TxBerSweep(tx, settings, warmup, chunk_samples) as s:
        flat = s.run(nsamples, first_sample, None if counters is None else counters.view(len(settings), 8, 2))
    return flat.view(shape)
