"""Exact symbol timing recovery over int16 samples -- the block between the front end and the detectors (include/bbb.h,
bbb_timing_*).  Every other path of the receiver decides at phase + k * stride: one sampling phase for the whole record, which
holds while transmitter and receiver share a clock.  A capture from an ADC with its own clock drifts; this tracker follows it.

  a(n) = acc(n)        block j = L symbols of P samples        E_j[p] = sum_i |a(j L P + i P + p) - threshold|

The first block after reset takes `init_phase`, or the phase with the largest metric; every later block moves the phase by at
most one, towards the larger neighbour where that beats the current phase by more than cur >> hysteresis_shift.  A move across
phase 0 wraps: that block emits L - 1 or L + 1 bits, so no bit is sampled twice or skipped.  All in exact integers; the state
(locked, phase, bits emitted) is two words ON THE DEVICE, so a stream never synchronises for it.

`TimingRecovery(spb, ff)` holds the receive filter (a fir.FIR or its taps; None: no filter).  `slice` returns the decisions
packed as RX.slice packs them, `recover` also the soft values and the phase of every block, `stream` an object that takes a
record in pieces of any size.  The number of bits depends on the data: it is read from the device once per call.

The soft values come at one sample per symbol, which is what the detectors take at spb 1:

    tr = TimingRecovery(8, FIR.moving_average())
    bits, nbits, soft, phases = tr.recover(capture)
    DFE([1], fb, spb=1).slice(soft[:nbits])           # or MLSE([1], g, spb=1)
    tr.clock_offset_ppm(phases)                       # the ADC's clock against the transmitter's
"""
import ctypes as C

import torch

from . import _lib
from .fir import FIR, Carry, _DT

ACQUIRE = 0xFFFFFFFF     # BBB_TIMING_ACQUIRE
_STATS = ("blocks", "moves", "wraps_up", "wraps_down")


class TimingRecovery:
    def __init__(self, spb, ff=None, block_symbols=0, hysteresis_shift=0, threshold=0, strict=False, init_phase=None, chunk_blocks=0):
        self.ff = ff if isinstance(ff, FIR) else FIR([1] if ff is None else ff)
        self.spb, self.block_symbols, self.hysteresis_shift = int(spb), int(block_symbols), int(hysteresis_shift)
        if not 3 <= self.spb <= 256:
            raise ValueError("spb must be 3..256")
        self.L = self.block_symbols or 64
        if not 8 <= self.L <= 1024 or self.L * self.spb > 65536:
            raise ValueError("block_symbols must be 8..1024 with block_symbols * spb <= 65536")
        if not 0 <= self.hysteresis_shift <= 63:
            raise ValueError("hysteresis_shift must be 1..63 (0: the default, 4)")
        if not -2 ** 31 <= int(threshold) < 2 ** 31:
            raise ValueError("threshold must be an int32 value")
        if init_phase is not None and not 0 <= int(init_phase) < self.spb:
            raise ValueError("init_phase must be None (acquire) or 0 .. spb - 1")
        self.threshold, self.strict = int(threshold), bool(strict)
        self.init_phase = ACQUIRE if init_phase is None else int(init_phase)
        self.chunk_blocks = int(chunk_blocks)
        self.device = self.ff.device
        self._stats = None

    def _cfg(self, out_bytes=2):
        c = _lib.TimingCfg()
        c.ff = self.ff._cfg(1, 0, out_bytes)
        c.spb, c.block_symbols, c.hysteresis_shift = self.spb, self.block_symbols, self.hysteresis_shift
        c.threshold, c.strict, c.init_phase, c.chunk_blocks = self.threshold, int(self.strict), self.init_phase, self.chunk_blocks
        return c

    def plan(self, nin, final=True):
        """The sizes of a call of `nin` samples (bbb_timing_plan, host only): a dict of nblocks, nconsumed (a call that is not
        final leaves the samples behind its last whole block), max_bits and nbefore_wanted."""
        names = ("nblocks", "nconsumed", "max_bits", "nbefore_wanted")
        v = [C.c_uint64() for _ in names]
        cfg = self._cfg()
        _lib.check(_lib.lib().bbb_timing_plan(C.byref(cfg), int(nin), int(bool(final)), *[C.byref(x) for x in v]), "bbb_timing_plan")
        return {n: x.value for n, x in zip(names, v)}

    def new_state(self):
        """The two state words on the device, out of reset."""
        return torch.zeros(2, dtype=torch.int64, device=torch.device("cuda", self.device))

    def _run(self, samples, nbefore, state, final, soft_dtype, want_phases):
        nbefore = self.ff._samples(samples, nbefore)
        if state is None:
            state = self.new_state()
        _lib.cuda_tensor("state", state, (torch.int64,), "int64", self.device)
        if state.numel() != 2:
            raise ValueError("state must hold two elements")
        nin = samples.numel() - nbefore
        p = self.plan(nin, final)
        dev = samples.device
        bits = torch.empty((p["max_bits"] + 63) // 64, dtype=torch.int64, device=dev)
        soft = None if soft_dtype is None else torch.empty(p["max_bits"], dtype=soft_dtype, device=dev)
        phases = torch.empty(p["nblocks"], dtype=torch.uint8, device=dev) if want_phases else None
        if self._stats is None:
            self._stats = torch.zeros(4, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        cfg = self._cfg(2 if soft_dtype is None else _DT[soft_dtype])
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())                                    # noqa: E731
        _lib.check(_lib.lib().bbb_timing_run(C.c_void_p(samples.data_ptr() + 2 * nbefore), nin, nbefore, int(bool(final)), C.byref(cfg),
                                             ptr(state), ptr(bits), ptr(soft), ptr(phases), ptr(self._stats), ptr(count), self.device,
                                             C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "bbb_timing_run")
        nbits = int(count.item())                     # the one read of the call: the count depends on the data
        return bits, nbits, soft, phases, p["nconsumed"]

    def slice(self, samples, nbefore=0, state=None, final=True):
        """The decisions of an int16 CUDA tensor (bbb_timing_run): (packed int64 tensor, nbits) as FIR.slice returns them; the
        words hold room for one more bit per block than a steady phase gives, the bits from nbits on are 0.  The first
        `nbefore` elements are the record's earlier samples (the nearest len(ff) are used).  state: new_state(), read and
        rewritten on the device; None: out of reset.  final=False: only whole blocks are decided (see plan)."""
        bits, nbits, _, _, _ = self._run(samples, nbefore, state, final, None, False)
        return bits, nbits

    def recover(self, samples, nbefore=0, state=None, final=True, out_dtype=torch.int16):
        """slice, the soft values the decisions were taken from, one per symbol (room for max_bits, nbits written:
        sat16(a >> ff.shift) as int16 or a itself as int32), and the phase of every block (uint8): (bits, nbits, soft, phases)."""
        if out_dtype not in _DT:
            raise ValueError("out_dtype must be torch.int16 or torch.int32")
        return self._run(samples, nbefore, state, final, out_dtype, True)[:4]

    def stats(self):
        """What the calls through this object added up (synchronises): blocks, moves, wraps_up, wraps_down."""
        v = [0, 0, 0, 0] if self._stats is None else self._stats.cpu().tolist()
        return dict(zip(_STATS, v))

    def stream(self, out_dtype=None):
        """A TimingStream: `push(chunk)` takes chunks of any size, any cutting of a record gives the bits of one call."""
        return TimingStream(self, out_dtype)

    def clock_offset_ppm(self, phases):
        """The receiver's sample clock against the transmitter's bit clock in parts per million, from the phase of every block
        (a tensor or array, as `recover` returns it): the slope of a least-squares line through the unwrapped phase track,
        in samples per block, over the block's spb * block_symbols samples.  Positive: the sampling instants move later,
        the capture holds more than spb samples per bit."""
        import numpy as np
        ph = np.asarray(phases.cpu() if isinstance(phases, torch.Tensor) else phases, dtype=np.int64)
        if len(ph) < 2:
            return 0.0
        d = np.diff(ph)
        d = (d + self.spb // 2) % self.spb - self.spb // 2         # a step of at most one phase, across the wrap too
        track = np.concatenate([[0], np.cumsum(d)]) + ph[0]
        slope = np.polyfit(np.arange(len(track), dtype=np.float64), track.astype(np.float64), 1)[0]
        return float(slope / (self.spb * self.L) * 1e6)


class TimingStream(Carry):
    """A record recovered piece by piece.  fir.Carry holds what the next call reads again: the samples behind the last whole
    block (a call that is not final leaves them) and len(ff) samples of history in front of them; `state` is the device's two
    words.  `push(chunk, final=False)` returns (packed bits, nbits), with out_dtype (packed bits, nbits, soft); it reads the
    bit count once."""

    def __init__(self, tr, out_dtype=None):
        if out_dtype is not None and out_dtype not in _DT:
            raise ValueError("out_dtype must be None, torch.int16 or torch.int32")
        self.tr, self.out_dtype = tr, out_dtype
        self.state = tr.new_state()
        self.ntaps = len(tr.ff.taps)
        self.hist = 0                              # of the samples carried, those in front of the next block
        self.phases = []
        super().__init__(self.ntaps + tr.L * tr.spb)

    def push(self, chunk, final=False):
        self.tr.ff._samples(chunk, 0)
        samples, have = self.place(chunk)
        # [history | remainder | chunk]: the remainder and the chunk are the call's samples
        nbefore = self.hist
        bits, nbits, soft, phases, nconsumed = self.tr._run(samples, nbefore, self.state, final, self.out_dtype, True)
        self.phases.append(phases)
        left = samples.numel() - nbefore - nconsumed                  # the samples behind the last whole block
        self.hist = min(self.ntaps, nbefore + nconsumed)
        self.keep = self.hist + left
        self.advance(chunk.numel())
        self.keep = self.ntaps + self.tr.L * self.tr.spb
        return (bits, nbits, soft) if self.out_dtype is not None else (bits, nbits)
