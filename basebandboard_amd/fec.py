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

A Viterbi decoder leaves its errors in bursts.  `ReedSolomon` (include/bbb.h, bbb_rs_*) is the outer code that removes them: an
exact Reed-Solomon codec over GF(2^8) whose codewords are interleaved symbol by symbol to depth 1..8, and `Concatenated(outer,
inner)` is the pair as one `fec=`; with `sync=` (a framesync.FrameSync) it marks its frames and finds them again.
"""
import ctypes as C
from fractions import Fraction

import torch

from . import _lib
from .fir import Carry
from .framesync import FrameSync

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


def _as_bytes(name, t, device):
    """The uint8 view of a uint8 or packed int64 CUDA tensor (byte j = bits 8j .. 8j + 7 of the packed stream)."""
    _lib.cuda_tensor(name, t, (torch.uint8, torch.int64), "uint8 or int64", device)
    return t if t.dtype == torch.uint8 else t.view(torch.uint8)


class ReedSolomon:
    """Exact Reed-Solomon codec over GF(2^8) with symbol interleaving (include/bbb.h, bbb_rs_*): the outer code that removes
    the error bursts a Viterbi decoder leaves.  (n, k) with n <= 255 (below: shortened), t = (n - k) / 2 symbols corrected per
    codeword; the field is `prim_poly`'s, the generator's roots alpha^(prim (fcr + i)); `depth` codewords are interleaved symbol
    by symbol into a frame of depth * n bytes whose first depth * k bytes are the data unchanged.  The decoder is a
    bounded-distance decoder: a codeword with more than t wrong symbols FAILS (its data pass through, nerr 255) or, rarely,
    decodes to another codeword.  No erasures, no soft decisions, no dual basis.  The frames must start at byte 0:
    framesync.FrameSync finds them in a stream that does not."""

    def __init__(self, n=255, k=223, prim_poly=0x11D, fcr=0, prim=1, depth=1, device=0):
        self.n, self.k, self.prim_poly, self.fcr, self.prim, self.depth, self.device = (int(v) for v in (n, k, prim_poly, fcr, prim, depth, device))
        if not 1 <= self.k < self.n <= 255:
            raise ValueError("n must be k + 1 .. 255 and k at least 1")
        self._stats = None
        # everything else that is wrong with the code, from the library (host only)
        _lib.check(_lib.lib().bbb_rs_encode_host(None, 0, C.byref(self._cfg()), None), "bbb_rs_encode_host")

    @classmethod
    def ccsds(cls, depth=1, k=223, device=0):
        """The CCSDS (255, 223) or (255, 239) code in the conventional basis at interleaving depth 1..8."""
        if k not in (223, 239):
            raise ValueError("the CCSDS codes are (255, 223) and (255, 239)")
        return cls(255, k, 0x187, 112 if k == 223 else 120, 11, depth, device)

    @classmethod
    def dvb(cls, device=0):
        """The DVB (204, 188) code: (255, 239) over 0x11D from root alpha^0, shortened."""
        return cls(204, 188, 0x11D, 0, 1, 1, device)

    @property
    def nroots(self):
        return self.n - self.k

    @property
    def t(self):
        return self.nroots // 2

    @property
    def frame_bytes(self):
        return self.depth * self.n

    @property
    def data_bytes(self):
        return self.depth * self.k

    def _cfg(self):
        c = _lib.RSCfg()
        c.prim_poly, c.fcr, c.prim, c.nroots, c.n, c.depth = self.prim_poly, self.fcr, self.prim, self.n - self.k, self.n, self.depth
        return c

    def _stream_ptr(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _frames(self, name, t, per):
        b = _as_bytes(name, t, self.device)
        if b.numel() % per:
            raise ValueError(f"{name} must hold whole frames of {per} bytes")
        return b, b.numel() // per

    def encode(self, data):
        """The coded frames (a uint8 CUDA tensor) of whole data frames in a uint8 or packed int64 CUDA tensor (bbb_rs_encode).
        Asynchronous on the current torch stream."""
        b, nf = self._frames("data", data, self.data_bytes)
        out = torch.empty(nf * self.frame_bytes, dtype=torch.uint8, device=b.device)
        _lib.check(_lib.lib().bbb_rs_encode(C.c_void_p(b.data_ptr()), nf, C.byref(self._cfg()), C.c_void_p(out.data_ptr()), self.device,
                                            self._stream_ptr()), "bbb_rs_encode")
        return out

    def decode(self, coded):
        """(data, nerr) of whole coded frames in a uint8 or packed int64 CUDA tensor (bbb_rs_decode): the data frames as a uint8
        CUDA tensor and one uint8 per codeword (frame f, codeword c at f * depth + c): the symbols corrected, 255 where the
        codeword failed.  Asynchronous on the current torch stream."""
        b, nf = self._frames("coded", coded, self.frame_bytes)
        data = torch.empty(nf * self.data_bytes, dtype=torch.uint8, device=b.device)
        nerr = torch.empty(nf * self.depth, dtype=torch.uint8, device=b.device)
        if self._stats is None:
            self._stats = torch.zeros(_lib.RS_NSTATS, dtype=torch.int64, device=b.device)
        _lib.check(_lib.lib().bbb_rs_decode(C.c_void_p(b.data_ptr()), nf, C.byref(self._cfg()), C.c_void_p(data.data_ptr()),
                                            C.c_void_p(nerr.data_ptr()), C.c_void_p(self._stats.data_ptr()), self.device, self._stream_ptr()),
                   "bbb_rs_decode")
        return data, nerr

    def stream(self):
        """An RSStream: `push(chunk)` decodes the whole frames that are complete so far, `finish()` says what was left over."""
        return RSStream(self)

    def stats(self):
        """What the decoder calls through this object added up (synchronises)."""
        v = [0] * _lib.RS_NSTATS if self._stats is None else self._stats.cpu().tolist()
        return dict(zip(("codewords", "clean", "failed", "symbols_corrected", "bits_corrected"), v))


class RSStream:
    """A coded record decoded piece by piece: the bytes of an incomplete frame are held back until the rest arrives, so the
    pieces give the data and nerr of one call.  Nothing lives on the device between calls but those bytes."""

    def __init__(self, code):
        self.code, self.held = code, None

    def push(self, chunk):
        """(data, nerr) of the frames this chunk completes (often none)."""
        b = _as_bytes("chunk", chunk, self.code.device).reshape(-1)
        buf = b if self.held is None or not self.held.numel() else torch.cat([self.held, b])
        whole = buf.numel() // self.code.frame_bytes * self.code.frame_bytes
        self.held = buf[whole:].clone()
        return self.code.decode(buf[:whole].contiguous())

    def finish(self):
        """The record ends here: the number of bytes of a last, incomplete frame, which are dropped."""
        left = 0 if self.held is None else self.held.numel()
        self.held = None
        return left


class LDPC:
    """Exact quasi-cyclic LDPC codec (include/bbb.h, bbb_ldpc_*): a layered normalised min-sum decoder over int16 posteriors and
    an encoder for codes whose parity part is block upper triangular.  `base` is the J x K base matrix of Z x Z circulants
    (-1: the zero block, s: the identity shifted by s); n = K Z coded bits, k = (K - J) Z data bits first, m = J Z checks.
    `max_iter` 1..64 iterations of J layers; `norm` / 16 scales the check messages (1..16); a HARD bit counts as +-`hard_mag`.
    A codeword whose checks are not all satisfied after max_iter iterations FAILED (iterations() gives 255) and its data bits
    are the hard decisions as they stand.  No puncturing, no shortening, no soft outputs."""

    def __init__(self, base, Z, max_iter=20, norm=12, hard_mag=32, device=0):
        rows = [[int(v) for v in row] for row in base]
        if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
            raise ValueError("base must be a J x K matrix")
        self.base, self.Z, self.J, self.K = rows, int(Z), len(rows), len(rows[0])
        self.max_iter, self.norm, self.hard_mag, self.device = int(max_iter), int(norm), int(hard_mag), int(device)
        if self.J > _lib.LDPC_MAX_J:
            raise ValueError("J must be 1..32")
        if self.K > _lib.LDPC_MAX_K:
            raise ValueError("K must be J + 1 .. 64")
        if not 1 <= self.norm <= 16:
            raise ValueError("norm must be 1..16")
        if not 1 <= self.hard_mag <= 32767:
            raise ValueError("hard_mag must be 1..32767")
        if any(not -1 <= v < max(self.Z, 0) for r in rows for v in r):
            raise ValueError("base entries must lie in -1 .. Z-1")
        self._stats, self._iters = None, None
        # everything else that is wrong with the code, from the library (host only)
        _lib.check(_lib.lib().bbb_ldpc_model_host(None, 0, 0, _lib.CONV_SOFT16, C.byref(self._cfg()), None, None, None), "bbb_ldpc_model_host")

    @classmethod
    def array(cls, p, J, K, max_iter=20, norm=12, hard_mag=32, device=0):
        """The triangular array code: p an odd prime, Z = p, J < K <= p; it needs no table and has an encoder."""
        p, J, K = int(p), int(J), int(K)
        if p < 3 or p % 2 == 0 or any(p % d == 0 for d in range(3, int(p ** 0.5) + 1, 2)):
            raise ValueError("p must be an odd prime")
        if not 1 <= J < K <= p:
            raise ValueError("array codes need 1 <= J < K <= p")
        base = [[j * (c + J - j) % p for c in range(K - J)] + [j * (i - j) % p if i >= j else -1 for i in range(J)] for j in range(J)]
        return cls(base, p, max_iter, norm, hard_mag, device)

    @property
    def n(self):
        return self.K * self.Z

    @property
    def k(self):
        return (self.K - self.J) * self.Z

    @property
    def m(self):
        return self.J * self.Z

    @property
    def rate(self):
        """Data bits per coded bit, a Fraction."""
        return Fraction(self.K - self.J, self.K)

    def _cfg(self):
        c = _lib.LDPCCfg()
        c.Z, c.J, c.K, c.max_iter, c.norm, c.hard_mag = self.Z, self.J, self.K, self.max_iter, self.norm, self.hard_mag
        for j, row in enumerate(self.base):
            for i, v in enumerate(row):
                c.base[j * self.K + i] = v
        return c

    def _stream_ptr(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def encode(self, bits, ncodewords):
        """The coded bits of `ncodewords` blocks of k data bits packed contiguously in an int64 CUDA tensor (bbb_ldpc_encode):
        (packed int64 tensor, ncodewords * n), codeword w's bit i at bit w n + i.  Asynchronous on the current torch stream."""
        _lib.cuda_tensor("bits", bits, (torch.int64,), "int64", self.device)
        ncodewords = int(ncodewords)
        if not 0 <= ncodewords * self.k <= 64 * bits.numel():
            raise ValueError("ncodewords * k bits must lie inside the tensor")
        out = torch.empty((ncodewords * self.n + 63) // 64, dtype=torch.int64, device=bits.device)
        _lib.check(_lib.lib().bbb_ldpc_encode(C.c_void_p(bits.data_ptr()), ncodewords, C.byref(self._cfg()), C.c_void_p(out.data_ptr()),
                                              self.device, self._stream_ptr()), "bbb_ldpc_encode")
        return out, ncodewords * self.n

    def decode(self, values, hard=False, nbits=None):
        """(packed int64 data bits, count) of the whole codewords among the received values (bbb_ldpc_decode); a ragged tail is
        ignored.  hard=False: `values` is an int16 CUDA tensor of soft values (positive means 1, 0 an erasure).  hard=True: a
        packed int64 CUDA tensor of `nbits` received bits, as RX.slice returns them.  iterations() then gives the byte per
        codeword of this call.  Asynchronous on the current torch stream."""
        if hard:
            _lib.cuda_tensor("values", values, (torch.int64,), "int64", self.device)
            if nbits is None or not 0 <= nbits <= 64 * values.numel():
                raise ValueError("hard decisions need nbits, inside the tensor")
            total = int(nbits)
        else:
            _lib.cuda_tensor("values", values, (torch.int16,), "int16", self.device)
            total = values.numel()
        ncw = total // self.n
        bits = torch.empty((ncw * self.k + 63) // 64, dtype=torch.int64, device=values.device)
        self._iters = torch.empty(ncw, dtype=torch.uint8, device=values.device)
        if self._stats is None:
            self._stats = torch.zeros(_lib.LDPC_NSTATS, dtype=torch.int64, device=values.device)
        _lib.check(_lib.lib().bbb_ldpc_decode(C.c_void_p(values.data_ptr()), 0, ncw, _lib.CONV_HARD if hard else _lib.CONV_SOFT16,
                                              C.byref(self._cfg()), C.c_void_p(bits.data_ptr()), C.c_void_p(self._iters.data_ptr()),
                                              C.c_void_p(self._stats.data_ptr()), self.device, self._stream_ptr()), "bbb_ldpc_decode")
        return bits, ncw * self.k

    def iterations(self):
        """The last decode call's byte per codeword (a uint8 CUDA tensor): 0 clean, 1..max_iter the iterations taken, 255 FAILED."""
        if self._iters is None:
            raise ValueError("no decode call yet")
        return self._iters

    def stream(self):
        """An LDPCStream over int16 soft values: `push(chunk)` decodes the codewords that are complete so far, `finish()` says
        how many values were left over."""
        return LDPCStream(self)

    def stats(self):
        """What the decoder calls through this object added up (synchronises)."""
        v = [0] * _lib.LDPC_NSTATS if self._stats is None else self._stats.cpu().tolist()
        return dict(zip(("codewords", "clean", "failed", "iterations", "bits_corrected"), v))


class LDPCStream:
    """A received record decoded piece by piece: the values of an incomplete codeword are held back until the rest arrives, so
    the pieces give the codewords of one call, each piece's data packed from its own bit 0.  Nothing lives on the device between
    calls but those values."""

    def __init__(self, code):
        self.code, self.held = code, None

    def push(self, chunk):
        """(packed data bits, count, iterations) of the codewords this chunk completes (often none)."""
        _lib.cuda_tensor("chunk", chunk, (torch.int16,), "int16", self.code.device)
        b = chunk.reshape(-1)
        buf = b if self.held is None or not self.held.numel() else torch.cat([self.held, b])
        whole = buf.numel() // self.code.n * self.code.n
        self.held = buf[whole:].clone()
        bits, nbits = self.code.decode(buf[:whole].contiguous())
        return bits, nbits, self.code.iterations()

    def finish(self):
        """The record ends here: the number of values of a last, incomplete codeword, which are dropped."""
        left = 0 if self.held is None else self.held.numel()
        self.held = None
        return left


class Concatenated:
    """The classic concatenation: an outer ReedSolomon around an inner ConvCode.  `decode` has the contract of
    ConvCode.decode for one final call from step 0, so RX.slice / count_errors / detect take it as `fec=`.  Without `sync`,
    step 0 of the inner code is bit 0 of frame 0.  With sync (a framesync.FrameSync whose payload is one coded frame), `encode`
    attaches a marker to every coded frame (and randomises it, if the FrameSync does) and `decode` finds the frames among the
    Viterbi decoder's bits wherever they start and whichever polarity they have, and hands those to the Reed-Solomon decoder."""

    def __init__(self, outer, inner, sync=None):
        if not isinstance(outer, ReedSolomon) or not isinstance(inner, ConvCode):
            raise ValueError("outer must be a ReedSolomon and inner a ConvCode")
        if outer.device != inner.device:
            raise ValueError("outer and inner must live on one device")
        if sync is not None:
            if not isinstance(sync, FrameSync):
                raise ValueError("sync must be a FrameSync")
            if sync.device != outer.device:
                raise ValueError("sync must live on the codes' device")
            if sync.payload_bytes != outer.frame_bytes:
                raise ValueError(f"sync's payload must be one coded frame of {outer.frame_bytes} bytes")
        self.outer, self.inner, self.sync = outer, inner, sync

    def encode(self, data):
        """(packed int64 transmitted bits, count) of whole data frames: RS-encoded, markers attached if there is a `sync`, then
        the frames' bits convolutionally encoded from step 0, with K - 1 zero steps appended if the inner code is terminated."""
        coded = self.outer.encode(data)
        tail = self.inner.K - 1 if self.inner.terminated else 0
        if self.sync is not None:
            framed, nframed = self.sync.attach(coded)
            packed = torch.zeros((nframed + tail + 63) // 64, dtype=torch.int64, device=coded.device)
            packed[:framed.numel()] = framed
            return self.inner.encode(packed, nframed + tail)
        nbits = 8 * coded.numel() + tail
        packed = torch.zeros((nbits + 63) // 64, dtype=torch.int64, device=coded.device)
        packed.view(torch.uint8)[:coded.numel()] = coded
        return self.inner.encode(packed, nbits)

    def decode(self, values, hard=False, nbits=None):
        """(packed int64 data bits, nbits): one final inner decode of the received values (soft int16, or hard packed bits with
        their count), then the RS decode of the whole frames among the decided steps; a trailing partial frame is dropped.
        With a `sync` the frames are those it finds (this reads their number back: it synchronises)."""
        bits, nd = self.inner.decode(values, hard=hard, nbits=nbits)
        if self.sync is not None:
            frames, _ = self.sync.sync(bits, nd)
            data, _ = self.outer.decode(frames.contiguous())
            out = torch.zeros((data.numel() + 7) // 8, dtype=torch.int64, device=data.device)
            out.view(torch.uint8)[:data.numel()] = data
            return out, 8 * data.numel()
        nf = nd // (8 * self.outer.frame_bytes)
        data, _ = self.outer.decode(bits.view(torch.uint8)[:nf * self.outer.frame_bytes])
        out = torch.zeros((data.numel() + 7) // 8, dtype=torch.int64, device=data.device)
        out.view(torch.uint8)[:data.numel()] = data
        return out, 8 * data.numel()
