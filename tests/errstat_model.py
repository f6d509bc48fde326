"""numpy model of the error statistics of include/bbb.h (bbb_errstat_*): gaps, bursts and errored blocks of the error
positions e_0 < e_1 < ... of a record.

  bin(v)  = v below 256, 256 + floor(log2 v) - 8 above (NBINS bins, bin 0 stays empty)
  gaps    g_i = e_i - e_(i-1): gap_hist, max_gap
  bursts  one starts at e_0 and at every e_i with g_i > guard; closed when the next one starts; the last one stays open
  blocks  errored_blocks[j] = number of distinct e_i // block_bits[j]

Two forms: `Walk` takes the record call by call, error by error, with the state a call hands to the next (the previous error
and the open burst); `direct` takes all positions at once, in array arithmetic.  tests/test_errstat_host.py holds them to
each other."""
import numpy as np

NBINS = 312
SCALARS = ("bits", "errors", "first_error", "last_error", "max_gap", "bursts", "burst_len_sum", "max_burst_len",
           "max_burst_weight", "open_first", "open_last", "open_weight")
HISTS = ("gap_hist", "burst_len_hist", "burst_weight_hist")


def vbin(v):
    v = int(v)
    return v if v < 256 else 256 + (v.bit_length() - 1) - 8


def vbin_np(a):
    """vbin of an int64 array of values >= 1 (exact: shifts and compares only)."""
    a = np.asarray(a, dtype=np.int64)
    v, log2 = a.copy(), np.zeros(a.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        m = v >= (1 << s)
        log2 += m * s
        v = np.where(m, v >> s, v)
    return np.where(a < 256, a, 256 + log2 - 8)


def empty_result(nblocks):
    r = {n: 0 for n in SCALARS}
    r["errored_blocks"] = [0] * nblocks
    for n in HISTS:
        r[n] = np.zeros(NBINS, dtype=np.uint64)
    return r


class Walk:
    """The record call by call."""

    def __init__(self, guard=0, blocks=()):
        self.guard, self.blocks = guard, list(blocks)
        self.reset()

    def reset(self):
        self.r = empty_result(len(self.blocks))
        self.prev, self.bf, self.bw, self.pos = None, 0, 0, 0

    def accumulate(self, rel_positions, nbits):
        """The next nbits positions, with errors at the ascending rel_positions (counted from the call's first bit)."""
        r, guard = self.r, self.guard
        for t in rel_positions:
            t = int(t) + self.pos
            r["errors"] += 1
            p = self.prev
            for j, B in enumerate(self.blocks):
                if B and (p is None or t // B != p // B):
                    r["errored_blocks"][j] += 1
            if p is None:
                r["first_error"] = t
                self.bf, self.bw = t, 0
            else:
                g = t - p
                r["gap_hist"][vbin(g)] += 1
                r["max_gap"] = max(r["max_gap"], g)
                if g > guard:                      # closes the burst [bf, p] of weight bw
                    L = p - self.bf + 1
                    r["burst_len_hist"][vbin(L)] += 1
                    r["burst_weight_hist"][vbin(self.bw)] += 1
                    r["bursts"] += 1
                    r["burst_len_sum"] += L
                    r["max_burst_len"] = max(r["max_burst_len"], L)
                    r["max_burst_weight"] = max(r["max_burst_weight"], self.bw)
                    self.bf, self.bw = t, 0
            self.prev = t
            self.bw += 1
            r["last_error"] = t
        self.pos += int(nbits)

    def skip(self, nbits):
        self.pos += int(nbits)

    def result(self):
        r = dict(self.r)
        r["errored_blocks"] = list(r["errored_blocks"])
        for n in HISTS:
            r[n] = r[n].copy()
        r["bits"] = self.pos
        if self.prev is not None:
            r["open_first"], r["open_last"], r["open_weight"] = self.bf, self.prev, self.bw
        return r


def direct(e, bits, guard=0, blocks=()):
    """All of a record at once: e = the ascending absolute error positions (below 2^62), bits = its length."""
    e = np.asarray(e, dtype=np.int64)
    r = empty_result(len(blocks))
    r["bits"] = int(bits)
    r["errors"] = len(e)
    if len(e) == 0:
        return r
    r["first_error"], r["last_error"] = int(e[0]), int(e[-1])
    g = np.diff(e)
    if len(g):
        r["gap_hist"] = np.bincount(vbin_np(g), minlength=NBINS).astype(np.uint64)
        r["max_gap"] = int(g.max())
    for j, B in enumerate(blocks):
        if B:
            r["errored_blocks"][j] = 1 + int(np.count_nonzero(e[1:] // B != e[:-1] // B))
    starts = np.concatenate([[0], np.flatnonzero(g > guard) + 1])      # index of every burst's first error
    ends = np.concatenate([starts[1:] - 1, [len(e) - 1]])              # ... and of its last
    length, weight = e[ends] - e[starts] + 1, ends - starts + 1
    r["open_first"], r["open_last"], r["open_weight"] = int(e[starts[-1]]), int(e[-1]), int(weight[-1])
    length, weight = length[:-1], weight[:-1]                          # the closed ones
    if len(length):
        r["burst_len_hist"] = np.bincount(vbin_np(length), minlength=NBINS).astype(np.uint64)
        r["burst_weight_hist"] = np.bincount(vbin_np(weight), minlength=NBINS).astype(np.uint64)
        r["bursts"] = len(length)
        r["burst_len_sum"] = int(length.sum())
        r["max_burst_len"], r["max_burst_weight"] = int(length.max()), int(weight.max())
    return r


def positions(words, nbits, mask=None):
    """The error positions of a packed stream (bit t at word t // 64, bit t % 64), counted from its first bit."""
    w = np.ascontiguousarray(words).view(np.uint64)
    if mask is not None:
        w = w & ~np.ascontiguousarray(mask).view(np.uint64)
    return np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little")[:nbits])


def pack(nbits, pos):
    """A packed stream of nbits bits (uint64 words) with ones at the positions pos."""
    b = np.zeros((nbits + 63) // 64 * 64, dtype=np.uint8)
    b[np.asarray(pos, dtype=np.int64)] = 1
    return np.packbits(b, bitorder="little").view(np.uint64)


def differences(got, want):
    """The names of the fields in which two results differ (got may be a ctypes bbb_errstat_result or a dict)."""
    get = (lambda n: got[n]) if isinstance(got, dict) else (lambda n: getattr(got, n))
    bad = [n for n in SCALARS if int(get(n)) != int(want[n])]
    bad += [n for n in HISTS if not np.array_equal(np.array(get(n), dtype=np.uint64), want[n])]
    eb = [int(v) for v in get("errored_blocks")]
    if eb[:len(want["errored_blocks"])] != want["errored_blocks"] or any(eb[len(want["errored_blocks"]):]):
        bad.append("errored_blocks")
    return bad
