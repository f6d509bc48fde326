"""numpy int64 model of the filtered link of include/bbb.h (bbb_link_sweep_*), applied to a waveform the caller supplies
(the oracle's TX.x, or far out the product's own TX.generate output):

  acc(n) = sum_{i < ntaps} h[i] * x(n - i), x(n) = 0 for n < 0        z(n) = sat16(acc(n) >> shift)
  stream sample n is acc(n + delay) / z(n + delay)
  bathtub: phase p decides data bit m >= 0 from stream sample 8m + 45 + p, acc >= threshold (> when strict)
  histogram: row = 127 - clamp(z >> eye.shift, -128, 127), column = (n - col_origin) mod ncols of stream sample n
"""
import numpy as np

BIT_SAMPLE0 = 45


def wave_range(first, n, ntaps, delay):
    """(lo, count): the waveform samples [lo, lo + count) that stream samples [first, first + n) need; lo >= 0"""
    lo = max(0, first + delay - (ntaps - 1))
    return lo, first + n + delay - lo


def stream_acc(x, x0, first, n, taps, delay):
    """acc of stream samples first .. first + n - 1 (int64).  x holds waveform samples x0 .. x0 + len(x) - 1 and must cover
    wave_range(first, n, len(taps), delay); samples below 0 are 0."""
    h = np.asarray(taps, dtype=np.int64)
    lo, count = wave_range(first, n, len(h), delay)
    assert x0 <= lo and x0 + len(x) >= lo + count
    x = np.asarray(x, dtype=np.int64)[lo - x0:lo - x0 + count]
    below = first + delay - (len(h) - 1)                       # the first sample the first output reads
    xe = np.concatenate([np.zeros(lo - below, dtype=np.int64), x])          # xe[i] is sample below + i
    out = np.zeros(n, dtype=np.int64)
    for i, c in enumerate(h):
        if c:
            out += c * xe[len(h) - 1 - i:len(h) - 1 - i + n]
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out


def stream_z(acc, shift):
    return np.clip(acc >> shift, -32768, 32767)


def hist(z, first, ncols, eye_shift, col_origin):
    rows = 127 - np.clip(np.asarray(z, dtype=np.int64) >> eye_shift, -128, 127)
    cols = (first + np.arange(len(z), dtype=np.int64) - col_origin) % ncols
    h = np.zeros((256, ncols), dtype=np.uint64)
    np.add.at(h, (rows, cols), 1)
    return h


def bathtub(acc, first, threshold, strict, bit_of):
    """[8, 2] uint64 = bits, errors per phase.  bit_of(m_lo, count) gives data bits m_lo .. m_lo + count - 1."""
    acc = np.asarray(acc, dtype=np.int64)
    r = first + np.arange(len(acc), dtype=np.int64) - BIT_SAMPLE0
    m, p = r // 8, r % 8
    ok = m >= 0
    tub = np.zeros((8, 2), dtype=np.uint64)
    if not ok.any():
        return tub
    m_lo = int(m[ok].min())
    b = np.asarray(bit_of(m_lo, int(m[ok].max()) - m_lo + 1))[m[ok] - m_lo]
    dec = (acc[ok] > threshold) if strict else (acc[ok] >= threshold)
    np.add.at(tub[:, 0], p[ok], 1)
    np.add.at(tub[:, 1], p[ok], (dec != b.astype(bool)).astype(np.uint64))
    return tub


def link(x, x0, first, n, taps, delay, shift, threshold, strict, bit_of, eye=None):
    """(bathtub, hist or None) of stream samples [first, first + n); eye = (ncols, eye_shift, col_origin)"""
    a = stream_acc(x, x0, first, n, taps, delay)
    tub = bathtub(a, first, threshold, strict, bit_of)
    return tub, (hist(stream_z(a, shift), first, *eye) if eye is not None else None)
