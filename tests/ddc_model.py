"""numpy int64 model of the digital down-converter of include/bbb.h (bbb_ddc_*), written from the formulas alone.

  j(n)  = (first + n) mod 2^24            pa(n) = (pa0 + j(n) fcw) mod 2^24            adr(n) = pa(n) >> 14
  c(n)  = ROM[(adr + 256) mod 1024]       s(n)  = ROM[adr]
  mi(n) = (x(n) c(n)) >> 15               mq(n) = (x(n) (-s(n))) >> 15
  ai(n) = sum_i h[i] mi(n - i)            I[q]  = sat16(ai(phase + q decim) >> shift)              (aq, Q likewise)
  x(n), n < 0: before[n] while n >= -len(before), 0 beyond

The ROM is tests/nco_model.py's; the accumulation is np.convolve in int64, which tests/test_ddc_host.py holds to the accumulate
rule of tests/fir_model.py.  `phase` may be any non-negative number here (the C ABI wants phase < decim).
"""
import numpy as np

from nco_model import ROM

MASK = (1 << 24) - 1
IQ16, IQ32, POLAR = 0, 1, 2

ANGLES = [int(round(np.arctan(2.0 ** -k) / (2 * np.pi) * 2 ** 32)) for k in range(16)]
assert ANGLES == [536870912, 316933406, 167458907, 85004756, 42667331, 21354465, 10679838, 5340245, 2670163, 1335087, 667544,
                  333772, 166886, 83443, 41722, 20861]


def lo(first, n0, n, fcw, pa0):
    """(c, s) of the samples n0 .. n0 + n - 1 (n0 may be negative) of a record whose sample 0 has the absolute number first."""
    j = (first + n0 + np.arange(n, dtype=np.int64)) & MASK
    adr = ((pa0 + j * fcw) & MASK) >> 14
    return ROM[(adr + 256) & 1023], ROM[adr]


def mix(x, first, fcw, pa0, n0=0):
    x = np.asarray(x, dtype=np.int64)
    c, s = lo(first, n0, len(x), fcw, pa0)
    return (x * c) >> 15, (x * -s) >> 15


def acc(m, taps, before=()):
    """sum_i h[i] m(n - i) for n in [0, len(m)), int64; `before`: the values of m in front (the nearest len(h) - 1 count)."""
    h = np.asarray(taps, dtype=np.int64)
    b = np.asarray(before, dtype=np.int64)[len(before) - min(len(before), len(h) - 1):]
    full = np.convolve(np.concatenate([b, np.asarray(m, dtype=np.int64)]), h)
    return full[len(b):len(b) + len(m)]


def baseband(x, fcw, taps, first=0, pa0=0, before=()):
    """(ai, aq) for every input sample, int64."""
    nb = len(before)
    mi, mq = mix(x, first, fcw, pa0)
    bi, bq = mix(before, first, fcw, pa0, n0=-nb)
    return acc(mi, taps, bi), acc(mq, taps, bq)


def cordic(i, q):
    """(mag, phase) of int16 pairs, vectorised in int64 with the int32 bound asserted."""
    i, q = np.atleast_1d(np.asarray(i, dtype=np.int64)), np.atleast_1d(np.asarray(q, dtype=np.int64))
    neg = i < 0
    X, Y = np.where(neg, -i, i) << 14, np.where(neg, -q, q) << 14
    Z = np.where(neg, 1 << 31, 0).astype(np.int64)
    for k in range(16):
        d = Y >= 0
        X, Y = np.where(d, X + (Y >> k), X - (Y >> k)), np.where(d, Y - (X >> k), Y + (X >> k))
        Z = (Z + np.where(d, ANGLES[k], -ANGLES[k])) & 0xFFFFFFFF
        assert max(np.abs(X).max(initial=0), np.abs(Y).max(initial=0)) < 2 ** 31
    mag = (X * 39797 + (1 << 29)) >> 30
    ph = ((Z + (1 << 15)) >> 16) & 0xFFFF
    ph = np.where(ph >= 32768, ph - 65536, ph)
    zero = (i == 0) & (q == 0)
    return np.where(zero, 0, mag).astype(np.uint16), np.where(zero, 0, ph).astype(np.int16)


def nout(nin, decim=1, phase=0):
    return (nin - phase + decim - 1) // decim if phase < nin else 0


def ddc(x, fcw, taps, shift=0, decim=1, phase=0, first=0, pa0=0, before=(), mode=IQ16):
    """[nout, 2]: int16 (I, Q), int32 (ai >> shift, aq >> shift), or (mag as the bits of an int16, phase) -- the layout of
    out_dev."""
    ai, aq = baseband(x, fcw, taps, first, pa0, before)
    ai, aq = ai[phase::decim] >> shift, aq[phase::decim] >> shift
    assert len(ai) == nout(len(x), decim, phase)
    if mode == IQ32:
        assert max(np.abs(ai).max(initial=0), np.abs(aq).max(initial=0)) < 2 ** 31
        return np.stack([ai, aq], axis=1).astype(np.int32)
    i, q = np.clip(ai, -32768, 32767), np.clip(aq, -32768, 32767)
    if mode == IQ16:
        return np.stack([i, q], axis=1).astype(np.int16)
    mag, ph = cordic(i, q) if len(i) else (np.zeros(0, np.uint16), np.zeros(0, np.int16))
    return np.stack([mag.view(np.int16), ph], axis=1)


def stream(x, fcw, taps, cuts, shift=0, decim=1, phase=0, first=0, pa0=0, mode=IQ16):
    """The record converted piece by piece as DDCStream does: ntaps - 1 samples of history, the phase and the sample number
    carried."""
    x = np.asarray(x, dtype=np.int64)
    parts, edges = [], [0] + list(cuts) + [len(x)]
    for a, b in zip(edges[:-1], edges[1:]):
        parts.append(ddc(x[a:b], fcw, taps, shift, decim, phase, first + a, pa0, before=x[max(0, a - (len(taps) - 1)):a], mode=mode))
        phase = (phase - (b - a)) % decim
    return np.concatenate(parts)
