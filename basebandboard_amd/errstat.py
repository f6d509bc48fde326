"""How a link's errors are distributed: gaps between errors, bursts, errored blocks (include/bbb.h, bbb_errstat_*).

`ErrorStats(guard, block_bits)` reads packed error streams on the GPU -- the `err` stream of
`PRBSErrorDetector.run_stream` with `reload` as its mask, or any stream in the layout of `PRBS.generate` -- and keeps exact
integer counters on the device.  Positions are absolute over the life of the object: every `accumulate` and `skip` continues
where the previous call ended, so a long record may arrive in pieces.

    bin(v) = v below 256, 256 + floor(log2 v) - 8 above: `bin_edges()` gives the lower edge of each of the NBINS bins.
    gap_hist            the distances between consecutive errors
    burst_len_hist,     a burst starts at the first error and at every error more than `guard` positions behind its
    burst_weight_hist   predecessor; its length is last - first + 1, its weight the number of its errors
    errored_blocks[j]   blocks of block_bits[j] positions (aligned to position 0) with at least one error
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

NBINS = _lib.ERRSTAT_NBINS

_SCALARS = ("bits", "errors", "first_error", "last_error", "max_gap", "bursts", "burst_len_sum", "max_burst_len",
            "max_burst_weight", "open_first", "open_last", "open_weight")
_HISTS = ("gap_hist", "burst_len_hist", "burst_weight_hist")


def vbin(v):
    """The bin of a value v >= 1."""
    v = int(v)
    if not 1 <= v < 1 << 64:
        raise ValueError("v must be in [1, 2^64)")
    return v if v < 256 else 256 + (v.bit_length() - 1) - 8


def bin_edges():
    """The lower edge of every bin (uint64[NBINS]): 0..255, then 2^8, 2^9, ... 2^63."""
    return np.array(list(range(256)) + [1 << e for e in range(8, 64)], dtype=np.uint64)


def geometry():
    """(tile_bits, wave_bits): the positions one workgroup and one wavefront of the kernel cover (host only)."""
    t, w = C.c_uint64(), C.c_uint64()
    _lib.check(_lib.lib().bbb_errstat_geometry(C.byref(t), C.byref(w)), "bbb_errstat_geometry")
    return t.value, w.value


def summarise(res, block_bits=(), close=True):
    """The dict `ErrorStats.result` returns, from a bbb_errstat_result (`_lib.ErrstatResult`): its fields as ints and numpy
    uint64 arrays, and on top ber, nblocks[j], errored_block_rate[j], mean_burst_len, mean_burst_weight.  close=True counts
    the burst that is still open at the end of the data as a burst (host arithmetic; open_* stay as they are)."""
    out = {n: int(getattr(res, n)) for n in _SCALARS}
    for n in _HISTS:
        out[n] = np.array(getattr(res, n), dtype=np.uint64)
    block_bits = [int(b) for b in block_bits]
    out["block_bits"] = block_bits
    out["errored_blocks"] = [int(res.errored_blocks[j]) for j in range(len(block_bits))]
    out["closed"] = bool(close) and out["open_weight"] > 0
    if out["closed"]:
        length, weight = out["open_last"] - out["open_first"] + 1, out["open_weight"]
        out["burst_len_hist"][vbin(length)] += 1
        out["burst_weight_hist"][vbin(weight)] += 1
        out["bursts"] += 1
        out["burst_len_sum"] += length
        out["max_burst_len"] = max(out["max_burst_len"], length)
        out["max_burst_weight"] = max(out["max_burst_weight"], weight)
    in_bursts = out["errors"] if out["closed"] else out["errors"] - out["open_weight"]
    bits = out["bits"]
    out["ber"] = out["errors"] / bits if bits else 0.0
    out["nblocks"] = [-(-bits // b) if b else 0 for b in block_bits]
    out["errored_block_rate"] = [e / n if n else 0.0 for e, n in zip(out["errored_blocks"], out["nblocks"])]
    out["mean_burst_len"] = out["burst_len_sum"] / out["bursts"] if out["bursts"] else 0.0
    out["mean_burst_weight"] = in_bursts / out["bursts"] if out["bursts"] else 0.0
    return out


class ErrorStats(_lib.StreamHandle):
    _handle, _close, _set_stream = "_o", "bbb_errstat_close", "bbb_errstat_set_stream"

    def __init__(self, guard=0, block_bits=(), device=0):
        block_bits = [int(b) for b in block_bits]
        if not 0 <= int(guard) < 1 << 32:
            raise ValueError("guard must be in [0, 2^32)")
        if len(block_bits) > 4:
            raise ValueError("at most 4 block sizes")
        if any(not 0 <= b < 1 << 64 for b in block_bits):
            raise ValueError("block_bits must be in [1, 2^40)")
        self.guard, self.block_bits, self.device = int(guard), block_bits, int(device)
        cfg = _lib.ErrstatCfg(self.guard, len(block_bits), (C.c_uint64 * 4)(*block_bits))
        o = C.c_void_p()
        _lib.check(_lib.lib().bbb_errstat_open(C.byref(cfg), self.device, self._open_stream(), C.byref(o)), "bbb_errstat_open")
        self._o = o

    def _packed(self, name, t):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int64 CUDA tensor")
        if t.device != torch.device("cuda", self.device):
            raise ValueError(f"{name} must be on cuda:{self.device}")
        return t

    def accumulate(self, err, mask=None, nbits=None):
        """The next nbits positions (default: all of err): bit t of the packed int64 CUDA tensor `err` is an error unless the
        same bit of `mask` is set.  Asynchronous on the current torch stream.  An nbits that is no multiple of 64 ends the
        record: further calls raise ValueError until `reset`."""
        err = self._packed("err", err)
        nbits = err.numel() * 64 if nbits is None else int(nbits)
        if not 0 <= nbits <= err.numel() * 64:
            raise ValueError("err holds fewer than nbits bits")
        if mask is not None:
            mask = self._packed("mask", mask)
            if mask.numel() * 64 < nbits:
                raise ValueError("mask holds fewer than nbits bits")
        self._bind_stream()
        _lib.check(_lib.lib().bbb_errstat_accumulate(self._o, C.c_void_p(err.data_ptr()),
                                                     C.c_void_p(mask.data_ptr() if mask is not None else None), nbits),
                   "bbb_errstat_accumulate")

    def skip(self, nbits):
        """nbits error-free positions that are not read."""
        nbits = int(nbits)
        if not 0 <= nbits < 1 << 64:
            raise ValueError("nbits must be in [0, 2^64)")
        self._bind_stream()
        _lib.check(_lib.lib().bbb_errstat_skip(self._o, nbits), "bbb_errstat_skip")

    def reset(self):
        """Back to position 0 with every counter cleared."""
        self._bind_stream()
        _lib.check(_lib.lib().bbb_errstat_reset(self._o), "bbb_errstat_reset")

    def read(self):
        """The raw bbb_errstat_result (waits for the calls queued so far)."""
        res = _lib.ErrstatResult()
        self._bind_stream()
        _lib.check(_lib.lib().bbb_errstat_read(self._o, C.byref(res)), "bbb_errstat_read")
        return res

    def result(self, close=True):
        """Everything counted so far (`summarise`); waits for the calls queued so far.  The device state is untouched: more
        data may follow, and a later result closes whatever burst is open then."""
        return summarise(self.read(), self.block_bits, close)
