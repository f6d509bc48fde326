"""Exact frame synchroniser (include/bbb.h, bbb_framesync_* and bbb_frame_*): finds the frames of a packed bit stream that starts
anywhere, in front of the Reed-Solomon decoder.

  transmit   attach: a sync marker in front of every frame, the payload XORed with a pseudo-random byte table (optional)
  receive    find: the markers by correlation (dist <= tol_search in either polarity), then the classic machine: a candidate is
             confirmed by `verify` more markers a frame apart, LOCK emits a frame per step and rides over up to `flywheel`
             bad markers in a row before it falls back to SEARCH
             extract: the frames cut out at their bit positions into byte-aligned payloads, complemented where the polarity came
             up inverted, derandomised

The machine is serial and causal by definition (bbb.h has it in full); the GPU runs it exactly.  A record handed over in pieces
(`FrameSyncStream`) gives the frames, counters and state of one call.  Out of scope: bit-slip windows in lock, node
synchronisation of the inner code, soft-decision correlation, convolutional interleavers, markers longer than 64 bits.
"""
import ctypes as C

import torch

from . import _lib

CCSDS_MARKER, CCSDS_RANDOMIZER = 0x1DFCCF1A, (0x1A9, 0xFF)    # the buffer bytes 1A CF FC 1D; x^8 + x^7 + x^5 + x^3 + 1 from all ones
COUNTERS = ("frames", "flywheeled", "acquisitions", "losses", "rejected", "marker_bit_errors")
META_POLARITY, META_FLYWHEELED, META_FIRST = 1 << 8, 1 << 9, 1 << 10


class FrameSync:
    """A frame format and the synchroniser's settings.  marker: bit i is compared with stream bit p + i; marker_bits 8..64;
    frame_bits, marker included; tol_search <= tol_lock <= marker_bits / 4 (tol_lock None: tol_search); verify 0..7 further
    markers that confirm a candidate; flywheel 0..7 bad markers in a row that lock rides over; randomizer None or
    (rand_poly, rand_seed)."""

    def __init__(self, marker, marker_bits, frame_bits, tol_search=0, tol_lock=None, verify=1, flywheel=2, both_polarities=True,
                 randomizer=None, device=0):
        self.marker, self.marker_bits, self.frame_bits, self.tol_search = int(marker), int(marker_bits), int(frame_bits), int(tol_search)
        self.tol_lock = self.tol_search if tol_lock is None else int(tol_lock)
        self.verify, self.flywheel, self.both_polarities, self.device = int(verify), int(flywheel), bool(both_polarities), int(device)
        if randomizer is not None and (len(randomizer) != 2 or not randomizer[0]):
            raise ValueError("randomizer must be None or (rand_poly, rand_seed)")
        self.randomizer = None if randomizer is None else (int(randomizer[0]), int(randomizer[1]))
        for name in ("marker", "marker_bits", "frame_bits", "tol_search", "tol_lock", "verify", "flywheel"):
            if not 0 <= getattr(self, name) < 1 << (64 if name == "marker" else 32):
                raise ValueError(f"{name} out of range")
        self._totals = None
        self.plan(0)                                # everything else that is wrong with the settings, from the library

    @classmethod
    def ccsds(cls, depth, k=223, tol_search=0, tol_lock=None, verify=1, flywheel=2, both_polarities=True, randomize=True, device=0):
        """The CCSDS format around ReedSolomon.ccsds(depth, k) at the byte level: marker 1A CF FC 1D, frames of 32 + 8 * depth * 255
        bits, the standard's randomiser.  (The order of the bits within a byte on the channel is this project's.)"""
        if k not in (223, 239):
            raise ValueError("the CCSDS codes are (255, 223) and (255, 239)")
        return cls(CCSDS_MARKER, 32, 32 + 8 * int(depth) * 255, tol_search, tol_lock, verify, flywheel, both_polarities,
                   CCSDS_RANDOMIZER if randomize else None, device)

    @property
    def payload_bytes(self):
        """Bytes of a frame's payload; frame_bits - marker_bits must be a multiple of 8 for attach and extract."""
        if (self.frame_bits - self.marker_bits) % 8:
            raise ValueError("frame_bits - marker_bits must be a multiple of 8")
        return (self.frame_bits - self.marker_bits) // 8

    def _cfg(self):
        c = _lib.FrameSyncCfg()
        c.marker, c.marker_bits, c.frame_bits, c.tol_search, c.tol_lock = self.marker, self.marker_bits, self.frame_bits, self.tol_search, self.tol_lock
        c.verify, c.flywheel, c.both_polarities = self.verify, self.flywheel, int(self.both_polarities)
        if self.randomizer is not None:
            c.rand_poly, c.rand_seed = self.randomizer[0] & 0xFFFFFFFF, self.randomizer[1] & 0xFFFFFFFF
        return c

    def _stream_ptr(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def plan(self, nbits):
        """(scratch_bytes, holdback_bits, tile_bits) of a find over nbits (bbb_framesync_plan, host only): the scratch, the bits
        a stream holds back (a multiple of 64) and the bits one workgroup of the search pass covers."""
        out = _lib.FrameSyncPlan()
        _lib.check(_lib.lib().bbb_framesync_plan(int(nbits), C.byref(self._cfg()), C.byref(out)), "bbb_framesync_plan")
        return out.scratch_bytes, out.holdback_bits, out.tile_bits

    def new_state(self):
        """A zeroed state (SEARCH at position 0): an int64 CUDA tensor of 8 words, laid out as bbb.h says."""
        return torch.zeros(_lib.FRAMESYNC_NSTATE, dtype=torch.int64, device=torch.device("cuda", self.device))

    def attach(self, payload):
        """(packed int64 bits, nbits) of whole payloads in a uint8 or packed int64 CUDA tensor (bbb_frame_attach): frame i, marker
        then randomised payload, at bit i * frame_bits.  Asynchronous on the current torch stream."""
        _lib.cuda_tensor("payload", payload, (torch.uint8, torch.int64), "uint8 or int64", self.device)
        b = payload if payload.dtype == torch.uint8 else payload.view(torch.uint8)
        if b.numel() % self.payload_bytes:
            raise ValueError(f"payload must hold whole frames of {self.payload_bytes} bytes")
        nf = b.numel() // self.payload_bytes
        out = torch.empty((nf * self.frame_bits + 63) // 64, dtype=torch.int64, device=b.device)
        _lib.check(_lib.lib().bbb_frame_attach(C.c_void_p(b.data_ptr()), nf, C.byref(self._cfg()), C.c_void_p(out.data_ptr()), self.device,
                                               self._stream_ptr()), "bbb_frame_attach")
        return out, nf * self.frame_bits

    def find(self, bits, nbits, final=True, first_bit=0, state=None, max_frames=None):
        """(pos, meta, count) of `nbits` packed bits in an int64 CUDA tensor (bbb_framesync_run): the absolute positions of the
        frames' markers (int64), their meta words (int16; META_*), and the number of frames as a 0-dim int64 CUDA tensor (no
        host round trip; frames beyond max_frames, by default all that fit, are counted but not written).  state: the machine's
        state from new_state(), read and written; None: a fresh one, SEARCH at first_bit.  Asynchronous on the current torch
        stream."""
        _lib.cuda_tensor("bits", bits, (torch.int64,), "int64", self.device)
        nbits, first_bit = int(nbits), int(first_bit)
        if not 0 <= nbits <= 64 * bits.numel():
            raise ValueError("nbits must lie inside the tensor")
        own = state is None
        if own:
            state = self.new_state()
            if first_bit:
                state[1] = first_bit
        else:
            _lib.cuda_tensor("state", state, (torch.int64,), "int64", self.device)
            if state.numel() != _lib.FRAMESYNC_NSTATE:
                raise ValueError("state must hold 8 words")
        before = None if own else state[2:].clone()
        mf = nbits // self.frame_bits + 1 if max_frames is None else int(max_frames)
        pos = torch.empty(mf, dtype=torch.int64, device=bits.device)
        meta = torch.empty(mf, dtype=torch.int16, device=bits.device)
        scratch = torch.empty(max(1, self.plan(nbits)[0] // 8), dtype=torch.int64, device=bits.device)
        _lib.check(_lib.lib().bbb_framesync_run(C.c_void_p(bits.data_ptr()), nbits, first_bit, int(bool(final)), C.byref(self._cfg()),
                                                C.c_void_p(state.data_ptr()), C.c_void_p(pos.data_ptr()), C.c_void_p(meta.data_ptr()), mf,
                                                C.c_void_p(scratch.data_ptr()), self.device, self._stream_ptr()), "bbb_framesync_run")
        delta = state[2:] if own else state[2:] - before
        self._totals = delta.clone() if self._totals is None else self._totals + delta
        return pos, meta, state[0] >> 32 & 0xFFFFFFFF

    def extract(self, bits, nbits, pos, meta, count, first_bit=0):
        """The payloads of the first `count` records of a find over the same bits (bbb_frame_extract): a uint8 CUDA tensor of
        pos.numel() * payload_bytes bytes of which the first count * payload_bytes are written.  count: what find returned (a
        CUDA tensor, read on the device) or an int.  Asynchronous on the current torch stream."""
        _lib.cuda_tensor("bits", bits, (torch.int64,), "int64", self.device)
        _lib.cuda_tensor("pos", pos, (torch.int64,), "int64", self.device)
        _lib.cuda_tensor("meta", meta, (torch.int16,), "int16", self.device)
        if pos.numel() != meta.numel():
            raise ValueError("pos and meta must have one element per record")
        if not 0 <= nbits <= 64 * bits.numel():
            raise ValueError("nbits must lie inside the tensor")
        state = self.new_state()
        state[0] = (count if isinstance(count, torch.Tensor) else int(count)) << 32
        out = torch.empty((pos.numel() * self.payload_bytes + 7) // 8, dtype=torch.int64, device=bits.device).view(torch.uint8)
        _lib.check(_lib.lib().bbb_frame_extract(C.c_void_p(bits.data_ptr()), int(nbits), int(first_bit), C.c_void_p(pos.data_ptr()),
                                                C.c_void_p(meta.data_ptr()), C.c_void_p(state.data_ptr()), pos.numel(), C.byref(self._cfg()),
                                                C.c_void_p(out.data_ptr()), self.device, self._stream_ptr()), "bbb_frame_extract")
        return out[:pos.numel() * self.payload_bytes]

    def sync(self, bits, nbits):
        """(frames, count): find and extract over one whole record: the payloads as a uint8 CUDA tensor of count * payload_bytes
        bytes, and the count as an int (synchronises to read it)."""
        pos, meta, count = self.find(bits, nbits)
        out = self.extract(bits, nbits, pos, meta, count)
        n = int(count.item())
        return out[:n * self.payload_bytes], n

    def stream(self):
        """A FrameSyncStream: `push(words)` gives the frames that are certain so far, `finish(words, nbits)` the rest."""
        return FrameSyncStream(self)

    def stats(self):
        """What the find calls through this object (its streams included) added up (synchronises)."""
        v = [0] * len(COUNTERS) if self._totals is None else self._totals.cpu().tolist()
        return dict(zip(COUNTERS, v))


class FrameSyncStream:
    """A record synchronised piece by piece.  Every push but the last is whole 64-bit words.  The stream keeps the last
    hold-back words of `plan` on the device in front of the next piece, whatever the machine did, so nothing is read back to decide
    what to keep; the machine's state lives in `state` on the device.  The pieces give the frames, counters and state of one
    call."""

    def __init__(self, fs):
        self.fs, self.state = fs, fs.new_state()
        self.hold = fs.plan(0)[1] // 64
        self.held, self.nbits = None, 0                # the last words pushed (at most `hold`), the bits pushed so far

    def _call(self, words, nbits, final):
        _lib.cuda_tensor("words", words, (torch.int64,), "int64", self.fs.device)
        if not 0 <= nbits <= 64 * words.numel() or (not final and nbits != 64 * words.numel()):
            raise ValueError("every push but the last is whole words")
        buf = words if self.held is None or not self.held.numel() else torch.cat([self.held, words])
        nheld = buf.numel() - words.numel()
        first = self.nbits - 64 * nheld
        pos, meta, count = self.fs.find(buf, 64 * nheld + nbits, final=final, first_bit=first, state=self.state)
        frames = self.fs.extract(buf, 64 * nheld + nbits, pos, meta, count, first_bit=first)
        self.nbits += nbits
        self.held = buf[max(0, buf.numel() - self.hold):].clone()
        return frames, pos, meta, count

    def push(self, words):
        """(frames, pos, meta, count) of the frames this piece decides: count is a 0-dim CUDA tensor, the first count payloads
        of `frames` and records of pos and meta are written."""
        return self._call(words, 64 * words.numel(), False)

    def finish(self, words=None, nbits=0):
        """The record ends here, with a last piece of nbits bits (or none)."""
        if words is None:
            words = torch.empty(0, dtype=torch.int64, device=torch.device("cuda", self.fs.device))
        return self._call(words, int(nbits), True)
