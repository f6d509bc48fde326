"""Exact convolutional codec -- forward error correction for the receiver's decisions (include/bbb.h, bbb_conv_*): a rate 1/n code
of constraint length K 3..7, punctured or not, encoded on the GPU and decoded by a Viterbi run per block.

  state h = the last K-1 input bits      coded bit i = parity of the window (h, b) under gens[i], written as in the books
  gain    = sum_i r_i d(c_i), maximised over the paths      r_i the received value of coded bit i, 0 where it was punctured

`ConvCode(K, gens)` holds the code: `ConvCode(7, (0o171, 0o133))` is the usual one, `puncture="3/4"` (or "2/3", "5/6", "7/8",
or `(period, keep)` with one mask per generator) its punctured forms.  `encode` takes packed bits to packed transmitted bits;
`decode` takes either int16 SOFT values (positive means 1, 0 is an erasure) or packed HARD bits to the packed decisions.  The
record is decided in blocks of ABSOLUTE steps, each from one Viterbi run over the block, `warmup` steps in front and
`lookahead` behind (`geometry=(block, warmup, lookahead)`, 0: 192, 64, 64; they are part of the definition), so a call that
is not `final` decides only the whole blocks whose window lies inside it and `stream` can hand a record over in pieces and
get the bits of one call.  The decoder has no state on the device.

Soft values are the int16 outputs of FIR.filter, DFE.equalize or TimingRecovery.recover; the decoder's zero is the decision
threshold, so the caller SUBTRACTS THE THRESHOLD FIRST where it is not 0 (and keeps the result inside int16).
"""
import ctypes as C
from fractions import Fraction

import torch

from . import _lib
from .fir import Carry

PRESETS = {"2/3": (2, (0b01, 0b11)), "3/4": (3, (0b101, 0b011)), "5/6": (5, (0b10101, 0b01011)), "7/8": (7, (0b1010001, 0b0101111))}
DEFAULTS = (192, 64, 64)


class ConvCode:
    def __init__(self, K, gens, puncture=None, terminated=False, init_state=0, geometry=(0, 0, 0), device=0):
        self.K, self.gens = int(K), [int(g) for g in gens]
        if not 3 <= self.K <= 7:
            raise ValueError("K must be 3..7")
        if not 2 <= len(self.gens) <= 3:
            raise ValueError("gens must hold 2..3 generators")
        if isinstance(puncture, str):
            if puncture not in PRESETS:
                raise ValueError("puncture must be one of " + ", ".join(PRESETS) + " or (period, keep)")
            if len(self.gens) != 2:
                raise ValueError("the punctured presets are patterns of a rate 1/2 code")
            puncture = PRESETS[puncture]
        self.period, keep = (1, [1] * len(self.gens)) if puncture is None else (int(puncture[0]), [int(k) for k in puncture[1]])
        if len(keep) != len(self.gens):
            raise ValueError("keep must hold one mask per generator")
        self.keep = keep
        self.terminated, self.init_state, self.geometry, self.device = bool(terminated), int(init_state), tuple(int(v) for v in geometry), int(device)
        if len(self.geometry) != 3:
            raise ValueError("geometry must be (block, warmup, lookahead)")
        self._stats = None
        self.plan(0)                                # everything wrong with the code, from the library
        self._cum = [0]
        for r in range(self.period):
            self._cum.append(self._cum[-1] + sum(k >> r & 1 for k in self.keep))

    @property
    def n(self):
        return len(self.gens)

    @property
    def rate(self):
        """Input bits per transmitted bit, a Fraction."""
        return Fraction(self.period, self._cum[-1])

    def idx(self, t):
        """The transmitted bits in front of step t."""
        return t // self.period * self._cum[-1] + self._cum[t % self.period]

    def _cfg(self):
        c = _lib.ConvCfg()
        c.K, c.n, c.init_state, c.period, c.terminated = self.K, self.n, self.init_state & 0xFFFFFFFF, self.period, int(self.terminated)
        for i in range(self.n):
            c.gen[i], c.keep[i] = self.gens[i], self.keep[i]
        c.block_steps, c.warmup_steps, c.lookahead_steps = self.geometry
        return c

    def plan(self, nin, first_step=0, final=True):
        """(nsteps, ndecided, nbefore_wanted) of a decoder call over `nin` received values (bbb_conv_plan, host only): the whole
        steps they hold, how many of them it decides, and the history in values with which its first window is not zero-filled."""
        v = [C.c_uint64() for _ in range(3)]
        _lib.check(_lib.lib().bbb_conv_plan(C.byref(self._cfg()), int(nin), int(first_step), int(bool(final)), *[C.byref(x) for x in v]),
                   "bbb_conv_plan")
        return tuple(x.value for x in v)

    def _stream_ptr(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def encode(self, bits, nbits, first_step=0, state=None):
        """The transmitted bits of `nbits` input bits packed in an int64 CUDA tensor (bbb_conv_encode): (packed int64 tensor,
        count).  state: an int32 CUDA tensor of one element, the encoder's state, read and written, with which a record
        encoded in pieces gives the bits of one call (None: the call starts from init_state).  Termination is the caller
        appending K - 1 zero bits.  Asynchronous on the current torch stream."""
        _lib.cuda_tensor("bits", bits, (torch.int64,), "int64", self.device)
        if not 0 <= nbits <= 64 * bits.numel():
            raise ValueError("nbits must lie inside the tensor")
        if state is not None:
            _lib.cuda_tensor("state", state, (torch.int32,), "int32", self.device)
        nout = self.idx(first_step + nbits) - self.idx(first_step)
        out = torch.empty((nout + 63) // 64, dtype=torch.int64, device=bits.device)
        got = C.c_uint64()
        _lib.check(_lib.lib().bbb_conv_encode(C.c_void_p(bits.data_ptr()), int(nbits), int(first_step), C.byref(self._cfg()),
                                              C.c_void_p(state.data_ptr()) if state is not None else None, C.c_void_p(out.data_ptr()),
                                              C.byref(got), self.device, self._stream_ptr()), "bbb_conv_encode")
        assert got.value == nout
        return out, nout

    def decode(self, values, hard=False, nbits=None, nbefore=0, first_step=0, final=True):
        """The decisions of the received values (bbb_conv_decode): (packed int64 tensor, ndecided), bit k the decision of step
        first_step + k.  hard=False: `values` is an int16 CUDA tensor of soft values (positive means 1, 0 an erasure; remove
        the decision threshold first).  hard=True: a packed int64 CUDA tensor of `nbits` received bits, as RX.slice returns
        them.  The first `nbefore` values are the record's earlier ones, history for the first window.  final=False: the
        record goes on, only the blocks whose window lies inside the call are decided.  Asynchronous on the current torch
        stream."""
        if hard:
            _lib.cuda_tensor("values", values, (torch.int64,), "int64", self.device)
            if nbits is None or not 0 <= nbits <= 64 * values.numel():
                raise ValueError("hard decisions need nbits, inside the tensor")
            total = int(nbits)
        else:
            _lib.cuda_tensor("values", values, (torch.int16,), "int16", self.device)
            total = values.numel()
        nbefore = int(nbefore)
        if not 0 <= nbefore <= total:
            raise ValueError("nbefore must lie inside the values")
        _, nd, _ = self.plan(total - nbefore, first_step, final)
        bits = torch.empty((nd + 63) // 64, dtype=torch.int64, device=values.device)
        if self._stats is None:
            self._stats = torch.zeros(2, dtype=torch.int64, device=values.device)
        got = C.c_uint64()
        _lib.check(_lib.lib().bbb_conv_decode(C.c_void_p(values.data_ptr()), nbefore, total - nbefore, nbefore, int(first_step), int(bool(final)),
                                              _lib.CONV_HARD if hard else _lib.CONV_SOFT16, C.byref(self._cfg()), C.c_void_p(bits.data_ptr()),
                                              C.c_void_p(self._stats.data_ptr()), C.byref(got), self.device, self._stream_ptr()),
                   "bbb_conv_decode")
        assert got.value == nd
        return bits, nd

    def stream(self):
        """A ConvStream over int16 soft values: `push(chunk)` gives the decisions that are certain so far, `finish()` the rest;
        together those of one call over the whole record.  (Hard decisions stream as the values +1 / -1.)"""
        return ConvStream(self)

    def stats(self):
        """What the decoder calls through this object added up (synchronises): windows walked, steps decided."""
        v = [0, 0] if self._stats is None else self._stats.cpu().tolist()
        return dict(zip(("windows", "steps"), v))


class ConvStream(Carry):
    """A record decoded piece by piece, cut where mlse.MLSEStream cuts.  fir.Carry holds the received values of the steps not
    decided yet and, in front of them, the history the next call's first window reaches (`nbefore` of them); `first_step` is
    that of the next call.  Nothing lives on the device between calls."""

    def __init__(self, code):
        self.code, self.first_step, self.nbefore = code, 0, 0
        geom = [v or d for v, d in zip(code.geometry, DEFAULTS)]
        # the most that is ever held: a block and its lookahead not yet decided, a step cut short, the warm-up
        super().__init__((sum(geom) + 2) * code.n)
        self.keep = 0

    def _call(self, chunk, final):
        _lib.cuda_tensor("chunk", chunk, (torch.int16,), "int16", self.code.device)
        values, have = self.place(chunk)
        nin = have - self.nbefore + chunk.numel()
        bits, nd = self.code.decode(values, nbefore=self.nbefore, first_step=self.first_step, final=final)
        if nd:
            used = self.code.idx(self.first_step + nd) - self.code.idx(self.first_step)
            self.first_step += nd
            self.nbefore = min(self.code.plan(0, self.first_step, False)[2], self.nbefore + used)
            self.keep = self.nbefore + nin - used
        else:
            self.keep = have + chunk.numel()
        assert self.keep <= self.lead
        self.advance(chunk.numel())
        return bits, nd

    def push(self, chunk):
        """(packed bits, nbits) decided by this chunk: the blocks whose window is now complete (often none)."""
        return self._call(chunk, False)

    def finish(self):
        """(packed bits, nbits) of the steps still held: the record ends here."""
        return self._call(torch.empty(0, dtype=torch.int16, device=torch.device("cuda", self.code.device)), True)
