"""Exact Viterbi sequence detector (MLSE) over int16 samples -- the receiver's strongest detector (include/bbb.h, bbb_mlse_*):
the most likely SEQUENCE of bits behind a channel with inter-symbol interference, where the DFE decides bit by bit.

  y[k]      = sat16(acc(phase + k * spb) >> ff.shift)                 s(h, b) = g[0] d(b) + sum_i g[i] d(bit i - 1 of h)
  gain(h,b) = 2 y s(h, b) - s(h, b)^2, maximised over the paths       d = +1 / -1, h the last mem decisions

`MLSE(ff, g, spb)` holds the feed-forward filter (a fir.FIR, or its taps) and the mem + 1 int32 target taps g in units of y
(mem 1..4, sum |g| <= 2^20).  The record is decided in blocks of `block_symbols` ABSOLUTE symbols, each from one Viterbi run over
the block, `warmup_symbols` in front of it and `lookahead_symbols` behind it (0: 192, 32, 32; they are part of the definition).
`slice` returns the decisions packed as RX.slice packs them; a call that is not `final` decides only the whole blocks whose
window lies inside it, so `stream` can hand a record over in pieces and get the bits of one call.  The detector has no state
on the device.  `MLSE.mmse(h, ...)` designs filter and target from a measured pulse response (equalizer.mlse_target).
"""
import ctypes as C

import torch

from . import _lib
from .fir import FIR, Carry

MAX_MEM = 4          # BBB_MLSE_MAX_MEM
G_BOUND = 1 << 20


class MLSE:
    def __init__(self, ff, g, spb, phase=0, init_state=0, block_symbols=0, warmup_symbols=0, lookahead_symbols=0):
        self.ff = ff if isinstance(ff, FIR) else FIR(ff)
        self.g = [int(v) for v in g]
        if not 2 <= len(self.g) <= MAX_MEM + 1:
            raise ValueError("g must hold 2..5 taps (memory 1..4)")
        if sum(abs(v) for v in self.g) > G_BOUND:
            raise ValueError("sum |g| must be <= 2^20")
        self.ff._cfg(spb, phase)
        self.spb, self.phase, self.init_state = int(spb), int(phase), int(init_state)
        self.block_symbols, self.warmup_symbols, self.lookahead_symbols = int(block_symbols), int(warmup_symbols), int(lookahead_symbols)
        self.device = self.ff.device
        self.design_delay = None
        self._stats = None
        self.plan(0)                                # the geometry's limits

    @classmethod
    def mmse(cls, h, spb, cursor, nff, mem, noise_power, phase=0, shift=None, device=0, scale_bits=8, **kw):
        """Filter and target of a measured pulse response (equalizer.mlse_target); the design's re-timing is kept as
        `design_delay`."""
        import numpy as np
        from .equalizer import mlse_target
        ff, g, shift = mlse_target(h, spb, cursor, nff, mem, noise_power, shift, scale_bits)
        d = cls(FIR(ff.tolist(), shift=shift, device=device), g.tolist(), spb, phase, **kw)
        d.design_delay = d.ff.design_delay = int(cursor) - int(np.abs(np.asarray(h, dtype=np.float64)).argmax())   # dfe_taps' delay
        return d

    @property
    def mem(self):
        return len(self.g) - 1

    def _cfg(self, phase=None):
        c = _lib.MlseCfg()
        c.ff = self.ff._cfg(self.spb, self.phase if phase is None else phase)
        c.mem = self.mem
        for i, v in enumerate(self.g):
            c.g[i] = v
        c.init_state = self.init_state & 0xFFFFFFFF
        c.block_symbols, c.warmup_symbols, c.lookahead_symbols = self.block_symbols, self.warmup_symbols, self.lookahead_symbols
        return c

    def plan(self, nin, first_symbol=0, final=True, phase=None):
        """(nsym, ndecided, nbefore_wanted) of a call over `nin` samples (bbb_mlse_plan, host only): its symbols, how many of
        them it decides, and the history in samples with which its first window is not zero-filled."""
        v = [C.c_uint64() for _ in range(3)]
        _lib.check(_lib.lib().bbb_mlse_plan(C.byref(self._cfg(phase)), int(nin), int(first_symbol), int(bool(final)),
                                            *[C.byref(x) for x in v]), "bbb_mlse_plan")
        return tuple(x.value for x in v)

    def slice(self, samples, nbefore=0, first_symbol=0, final=True, phase=None):
        """The decisions of an int16 CUDA tensor (bbb_mlse_run): (packed int64 tensor, nbits) as FIR.slice returns them, bit k the
        decision of symbol first_symbol + k.  The first `nbefore` elements are the record's earlier samples, as in FIR.filter.
        final=False: the record goes on, only the blocks whose window lies inside the call are decided.  phase: in place of the
        object's.  Asynchronous on the current torch stream."""
        nbefore = self.ff._samples(samples, nbefore)
        cfg = self._cfg(phase)
        nin = samples.numel() - nbefore
        _, nbits, _ = self.plan(nin, first_symbol, final, phase)
        bits = torch.empty((nbits + 63) // 64, dtype=torch.int64, device=samples.device)
        if self._stats is None:
            self._stats = torch.zeros(2, dtype=torch.int64, device=samples.device)
        got = C.c_uint64()
        _lib.check(_lib.lib().bbb_mlse_run(C.c_void_p(samples.data_ptr() + 2 * nbefore), nin, nbefore, int(first_symbol), int(bool(final)),
                                           C.byref(cfg), C.c_void_p(bits.data_ptr()), C.c_void_p(self._stats.data_ptr()), C.byref(got),
                                           self.device, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "bbb_mlse_run")
        assert got.value == nbits
        return bits, nbits

    def stream(self):
        """An MLSEStream: `push(chunk)` gives the decisions that are certain so far, `finish()` the rest; together those of
        one call over the whole record."""
        return MLSEStream(self)

    def stats(self):
        """What the calls through this object added up (synchronises): windows walked, symbols decided."""
        v = [0, 0] if self._stats is None else self._stats.cpu().tolist()
        return dict(zip(("windows", "symbols"), v))


class MLSEStream(Carry):
    """A record detected piece by piece.  fir.Carry holds the samples of the symbols not decided yet and, in front of them,
    the history the next call's first window reaches (`nbefore` of them); `first_symbol` and `phase` are those of the next
    call.  Nothing lives on the device between calls."""

    def __init__(self, mlse):
        self.mlse, self.phase, self.first_symbol, self.nbefore = mlse, mlse.phase, 0, 0
        c = mlse._cfg()
        geom = [v or d for v, d in zip((c.block_symbols, c.warmup_symbols, c.lookahead_symbols), (192, 32, 32))]
        # the most that is ever held: a block and its lookahead not yet decided, a symbol cut short, the warm-up, the taps' reach
        super().__init__((sum(geom) + 1) * mlse.spb + len(mlse.ff.taps))
        self.keep = 0

    def _call(self, chunk, final):
        self.mlse.ff._samples(chunk, 0)
        samples, have = self.place(chunk)
        nin = have - self.nbefore + chunk.numel()
        bits, nbits = self.mlse.slice(samples, self.nbefore, self.first_symbol, final, self.phase)
        if nbits:
            pos = self.phase + nbits * self.mlse.spb     # the first symbol not decided yet, counted from this call's first sample
            used = min(pos, nin)
            self.first_symbol, self.phase = self.first_symbol + nbits, pos - used
            wanted = self.mlse.plan(0, self.first_symbol, False, self.phase)[2]
            self.nbefore = min(wanted, self.nbefore + used)
            self.keep = self.nbefore + nin - used
        else:
            self.keep = have + chunk.numel()
        assert self.keep <= self.lead
        self.advance(chunk.numel())
        return bits, nbits

    def push(self, chunk):
        """(packed bits, nbits) decided by this chunk: the blocks whose window is now complete (often none)."""
        return self._call(chunk, False)

    def finish(self):
        """(packed bits, nbits) of the symbols still held: the record ends here."""
        empty = torch.empty(0, dtype=torch.int16, device=torch.device("cuda", self.mlse.device))
        return self._call(empty, True)
