"""The numpy model of gateware/bbb/sinc.py that the sinc tests compare against: the coefficient table, the stream form
y[16 m + c] = (sum_i h[16 i + c] x[m - i]) >> 8, the module's batch, a literal evaluation of its 16-bit adder tree, and the
raised-cosine capture whose sub-sample timing the interpolated phase search recovers."""
import numpy as np

UP, TAPS, OFFSET = 16, 8, 109


def coefficients():
    """sinc.py:38-41 with numpy.hamming (scipy's window differs by one ulp and quantises identically)."""
    return (np.sinc(np.linspace(-4, 4, 128)) * np.hamming(128) * 127.0).astype(np.int8)


H = coefficients().astype(np.int64)


def unpack(words):
    """The table from the 32 BRAM words (sinc.py:42-48): tap i of phase c at h[16 i + c]."""
    h = np.zeros(128, dtype=np.int64)
    for c in range(16):
        for half in range(2):
            for i in range(4):
                h[64 * half + 16 * i + c] = np.int8(np.uint8((int(words[2 * c + half]) >> (24 - 8 * i)) & 0xFF))
    return h


def to8(x, shift=0):
    """The input rule: int16 samples are clamp(x >> shift, -128, 127)."""
    return np.clip(np.asarray(x, dtype=np.int64) >> shift, -128, 127)


def acc(x, before=()):
    """acc(m, c) as int64 [16 len(x)]; `before`: the record's samples in front of x (the nearest 7 count, 0 beyond)."""
    x = np.asarray(x, dtype=np.int64)
    b = np.asarray(before, dtype=np.int64)[-(TAPS - 1):] if len(before) else np.zeros(0, dtype=np.int64)
    xe = np.concatenate([np.zeros(TAPS - 1 - len(b), dtype=np.int64), b, x])
    a = np.zeros(UP * len(x), dtype=np.int64)
    for i in range(TAPS):
        xi = xe[TAPS - 1 - i:TAPS - 1 - i + len(x)]
        for c in range(UP):
            a[c::UP] += H[UP * i + c] * xi
    return a


def interpolate(x, before=(), shift=0):
    """The stream form, int64 values in -102 .. 101."""
    return acc(to8(x, shift), to8(before, shift) if len(before) else ()) >> 8


def batch(x):
    """The module: 72 inputs, no history -> 1024 outputs."""
    assert len(x) == 72
    return interpolate(x)[OFFSET:OFFSET + 1024]


def _w16(v):
    return ((np.asarray(v, dtype=np.int64) + 32768) % 65536) - 32768


def adder_tree(window, c):
    """sinc.py:91-98 literally: window[..., i] = x[m - i]; every register wraps at 16 bits, the last keeps bits 8..15."""
    w = np.asarray(window, dtype=np.int64)
    muls = [_w16(H[UP * i + c] * w[..., i]) for i in range(8)]
    add0 = [_w16(muls[2 * i] + muls[2 * i + 1]) for i in range(4)]
    add1 = [_w16(add0[2 * i] + add0[2 * i + 1]) for i in range(2)]
    s = add1[0] + add1[1]                     # a 17-bit sum in the expression; add2 takes 8 bits of s >> 8
    return ((((s >> 8) + 128) % 256) - 128)


def eye_hist(y, first_sample, ncols, shift, col_origin):
    """bbb_eye_accumulate_i16 over int samples y whose sample numbers start at first_sample: [256, ncols] counts."""
    y = np.asarray(y, dtype=np.int64)
    row = 127 - np.clip(y >> shift, -128, 127)
    col = (first_sample + np.arange(len(y), dtype=np.int64) - col_origin) % ncols
    return np.bincount(row * ncols + col, minlength=256 * ncols).reshape(256, ncols)


def prbs7(n):
    s, out = 1, np.empty(n, dtype=np.int64)
    for j in range(n):
        b = ((s >> 6) ^ (s >> 5)) & 1
        s = ((s << 1) | b) & 0x7F
        out[j] = b
    return out


def rc_capture(nbits, frac, spb=4, beta=0.5, amp=100):
    """A PRBS-7 stream through raised-cosine pulses (bit j centred at j + 0.5 bit periods), sampled at
    t = (n + frac) / spb, as int8 of amplitude `amp`.  Returns (samples, bits)."""
    bits = prbs7(nbits)
    a = 2.0 * bits - 1
    t = (np.arange(nbits * spb) + frac) / spb
    w = np.zeros(len(t))
    for k in range(-4, 5):
        idx = np.floor(t).astype(int) + k
        ok = (idx >= 0) & (idx < nbits)
        tau = t - idx - 0.5
        den = 1 - (2 * beta * tau) ** 2
        den[np.abs(den) < 1e-9] = 1e-9
        p = np.sinc(tau) * np.cos(np.pi * beta * tau) / den
        w += np.where(ok, a[np.clip(idx, 0, nbits - 1)] * p, 0)
    return np.clip(np.round(amp * w), -128, 127).astype(np.int8), bits
