"""Exact carrier recovery over int16 (I, Q) pairs -- the block between the down-converter and the decisions (include/bbb.h,
bbb_carrier_*).  The down-converter's oscillator is a function of the sample number; a transmitter a few ppm away leaves a
baseband vector that turns slowly, and neither I nor Q can be decided.  This block follows it.

  block j = L pairs        SR_j = sum(I I - Q Q)    SI_j = 2 sum(I Q)        h_j = (CORDIC phase of (SR_j, SI_j)) / 2
  est_j = h_j or h_j + half a turn, whichever lies within a quarter turn of est_(j-1)
  I' = sat16((I c + Q s) >> 15)    Q' = sat16((Q c - I s) >> 15)    with (c, s) the NCO ROM's cosine and sine at est_j

Squaring removes the BPSK data, and with it half a turn: `init_phase` (1/65536 turn; 16384 makes bit 1 positive for a carrier
phase-modulated by -512 per bit 1) or the frame synchroniser's polarity search decides which half.  The estimate is constant
over a block: the carrier may turn well below a quarter turn per block.  All in exact integers; the state (started, the last
estimate, pairs consumed) is two words ON THE DEVICE, and no call synchronises.

    iq = ddc.iq(capture)                                  # [n, 2] int16
    cr = CarrierRecovery(block_pairs=32, init_phase=16384)
    bits, nbits = cr.slice(iq)                            # packed as RX.slice packs them
    cr.carrier_offset()                                   # turns per pair
"""
import ctypes as C

import torch

from . import _lib

_STATS = ("blocks", "flips", "zero_blocks", "phase_steps")


class CarrierRecovery:
    def __init__(self, block_pairs=0, init_phase=0, threshold=0, strict=False, chunk_blocks=0, device=0):
        self.block_pairs, self.init_phase, self.threshold = int(block_pairs), int(init_phase), int(threshold)
        self.L = self.block_pairs or 32
        if not 8 <= self.L <= 1024 or self.L % 8:
            raise ValueError("block_pairs must be a multiple of 8 in 8..1024 (0: the default, 32)")
        if not 0 <= self.init_phase <= 65535:
            raise ValueError("init_phase must be 0..65535, in 1/65536 turn")
        if not -2 ** 31 <= self.threshold < 2 ** 31:
            raise ValueError("threshold must be an int32 value")
        self.strict, self.chunk_blocks, self.device = bool(strict), int(chunk_blocks), int(device)
        self._stats = None

    def _cfg(self):
        c = _lib.CarrierCfg()
        c.block_pairs, c.init_phase, c.threshold, c.strict, c.chunk_blocks = self.block_pairs, self.init_phase, self.threshold, int(self.strict), self.chunk_blocks
        return c

    def plan(self, nin, final=True):
        """The sizes of a call of `nin` pairs (bbb_carrier_plan, host only): a dict of nblocks and nconsumed (a call that is
        not final leaves the pairs behind its last whole block)."""
        nb, nc = C.c_uint64(), C.c_uint64()
        cfg = self._cfg()
        _lib.check(_lib.lib().bbb_carrier_plan(C.byref(cfg), int(nin), int(bool(final)), C.byref(nb), C.byref(nc)), "bbb_carrier_plan")
        return dict(nblocks=nb.value, nconsumed=nc.value)

    def new_state(self):
        """The two state words on the device, out of reset."""
        return torch.zeros(2, dtype=torch.int64, device=torch.device("cuda", self.device))

    def reset(self):
        """Forgets the counters of stats()."""
        self._stats = None

    def _pairs(self, pairs):
        if (not isinstance(pairs, torch.Tensor) or pairs.dtype != torch.int16 or not pairs.is_cuda or not pairs.is_contiguous()
                or pairs.dim() != 2 or pairs.shape[1] != 2):
            raise ValueError("pairs must be a contiguous [n, 2] int16 CUDA tensor")
        if (pairs.device.index or 0) != self.device:
            raise ValueError(f"pairs must be on cuda:{self.device}")
        if pairs.data_ptr() % 4:
            raise ValueError("pairs must be 4-byte aligned")

    def _run(self, pairs, state, final, want_iq, want_bits, want_soft, want_phase):
        self._pairs(pairs)
        if state is None:
            state = self.new_state()
        _lib.cuda_tensor("state", state, (torch.int64,), "int64", self.device)
        if state.numel() != 2:
            raise ValueError("state must hold two elements")
        p = self.plan(pairs.shape[0], final)
        n, nblocks, dev = p["nconsumed"], p["nblocks"], pairs.device
        iq = torch.empty((n, 2), dtype=torch.int16, device=dev) if want_iq else None
        bits = torch.empty((nblocks * self.L + 63) // 64, dtype=torch.int64, device=dev) if want_bits else None
        soft = torch.empty(n, dtype=torch.int16, device=dev) if want_soft else None
        phases = torch.empty(nblocks, dtype=torch.uint16, device=dev) if want_phase else None
        if self._stats is None:
            self._stats = torch.zeros(4, dtype=torch.int64, device=dev)
        if nblocks == 0:                              # nothing but the state to rewrite, and to what it is: no call (the empty
            return iq, bits, n, soft, phases          # outputs have no address to hand over)
        cfg = self._cfg()
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())                                    # noqa: E731
        _lib.check(_lib.lib().bbb_carrier_run(ptr(pairs), pairs.shape[0], int(bool(final)), C.byref(cfg), ptr(state), ptr(iq), ptr(bits),
                                              ptr(soft), ptr(phases), ptr(self._stats), self.device,
                                              C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "bbb_carrier_run")
        return iq, bits, n, soft, phases

    def derotate(self, pairs, state=None, final=True):
        """The pairs turned back, [nconsumed, 2] int16 (bbb_carrier_run): the data axis lies on I.  state: new_state(), read and
        rewritten on the device; None: out of reset.  final=False: only whole blocks are taken (see plan)."""
        return self._run(pairs, state, final, True, False, False, False)[0]

    def slice(self, pairs, state=None, final=True):
        """The decisions I' >= threshold: (packed int64 tensor, nbits) as FIR.slice returns them."""
        _, bits, n, _, _ = self._run(pairs, state, final, False, True, False, False)
        return bits, n

    def recover(self, pairs, state=None, final=True):
        """Every output of one call: (pairs [n, 2], packed bits, nbits, soft int16 [n], phases uint16 [nblocks])."""
        return self._run(pairs, state, final, True, True, True, True)

    def stats(self):
        """What the calls through this object added up (synchronises): blocks, flips (blocks whose estimate changed sides),
        zero_blocks (both sums 0), phase_steps (the sum of the wrapped steps of the estimate, 1/65536 turn)."""
        v = [0, 0, 0, 0] if self._stats is None else self._stats.cpu().tolist()
        return dict(zip(_STATS, v))

    def carrier_offset(self):
        """The carrier against the down-converter's oscillator in turns per pair: the mean step of the estimate per block over
        the block's pairs.  Positive: the baseband vector turns counter-clockwise.  0.0 before the first block."""
        s = self.stats()
        return s["phase_steps"] / (s["blocks"] * self.L * 65536.0) if s["blocks"] else 0.0

    def stream(self, outputs="iq"):
        """A CarrierStream: `push(chunk)` takes chunks of any size, any cutting of a record gives the outputs of one call."""
        return CarrierStream(self, outputs)


class CarrierStream:
    """A record recovered piece by piece.  The pairs behind the last whole block (fewer than L) wait for the next chunk;
    `state` is the device's two words.  outputs "iq": `push(chunk, final=False)` returns the pairs turned back; "bits":
    (packed bits, nbits); "all": what CarrierRecovery.recover returns.  The phases of every call collect in `phases`."""

    def __init__(self, cr, outputs="iq"):
        if outputs not in ("iq", "bits", "all"):
            raise ValueError('outputs must be "iq", "bits" or "all"')
        self.cr, self.outputs = cr, outputs
        self.state = cr.new_state()
        self.rest = None
        self.phases = []

    def push(self, chunk, final=False):
        self.cr._pairs(chunk)
        pairs = chunk if self.rest is None or self.rest.shape[0] == 0 else torch.cat([self.rest, chunk])
        o = self.outputs
        iq, bits, n, soft, phases = self.cr._run(pairs, self.state, final, o != "bits", o != "iq", o == "all", True)
        self.phases.append(phases)
        self.rest = pairs[n:].clone()
        return iq if o == "iq" else ((bits, n) if o == "bits" else (iq, bits, n, soft, phases))
