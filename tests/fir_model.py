"""numpy int64 model of the FIR filter of include/bbb.h (bbb_fir_*), and a clock-by-clock restatement of the reference's
MovingAverage (gateware/bbb/average.py:26-33).

  acc(n) = sum_{i < ntaps} h[i] * x[n - i]       x[j], j < 0: before[j] while j >= -len(before), 0 beyond
  y[q]   = sat(acc(phase + q * decim) >> shift)   q in [0, nout),  nout = phase < nin ? ceil((nin - phase) / decim) : 0
"""
import numpy as np


def nout(nin, decim=1, phase=0):
    return (nin - phase + decim - 1) // decim if phase < nin else 0


def acc(x, taps, before=()):
    """acc(n) for n in [0, len(x)) as int64; `before` are the record's earlier samples (all of them are used)."""
    h = np.asarray(taps, dtype=np.int64)
    x = np.asarray(x, dtype=np.int64)
    b = np.asarray(before, dtype=np.int64)[-(len(h) - 1):] if len(h) > 1 else np.zeros(0, dtype=np.int64)
    xe = np.concatenate([np.zeros(len(h) - 1 - len(b), dtype=np.int64), b, x])
    out = np.zeros(len(x), dtype=np.int64)
    for i, c in enumerate(h):
        if c:
            out += c * xe[len(h) - 1 - i:len(h) - 1 - i + len(x)]
    return out


def acc_fast(x, taps):
    """acc of a long record with no history, through numpy's float64 convolution: every product is below 2^31 and so is
    every partial sum (sum |h| <= 65535, |x| <= 32768), far inside the 53 bits float64 holds exactly, whatever the order
    of the additions.  tests/test_fir_host.py holds it to acc."""
    y = np.convolve(np.asarray(x, dtype=np.float64), np.asarray(taps, dtype=np.float64))[:len(x)]
    return y.astype(np.int64)


def filt(x, taps, shift=0, decim=1, phase=0, before=(), out_bytes=2):
    """y as int16 (saturating) or int32."""
    a = acc(x, taps, before)[phase::decim] >> shift
    assert len(a) == nout(len(x), decim, phase)
    if out_bytes == 2:
        return np.clip(a, -32768, 32767).astype(np.int16)
    assert a.min(initial=0) >= -2 ** 31 and a.max(initial=0) < 2 ** 31
    return a.astype(np.int32)


def pack(bits):
    """0/1 values packed LSB first into u64 words, the unused bits of the last word 0."""
    b = np.zeros((len(bits) + 63) // 64 * 64, dtype=np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint64)


def decisions(x, taps, stride=1, phase=0, threshold=0, strict=False, before=()):
    a = acc(x, taps, before)[phase::stride]
    return (a > threshold if strict else a >= threshold).astype(np.uint8)


def slice_packed(x, taps, stride=1, phase=0, threshold=0, strict=False, before=()):
    """(packed u64 words, nbits) of bbb_fir_slice."""
    d = decisions(x, taps, stride, phase, threshold, strict, before)
    return pack(d), len(d)


def next_phase(phase, decim, nin):
    return (phase - nin) % decim


def stream(x, taps, cuts, shift=0, decim=1, phase=0, out_bytes=2):
    """The record filtered piece by piece as FIRStream does: history of len(taps) - 1 samples, phase carried."""
    parts, hist = [], np.zeros(0, dtype=np.int64)
    edges = [0] + list(cuts) + [len(x)]
    for a, b in zip(edges[:-1], edges[1:]):
        parts.append(filt(x[a:b], taps, shift, decim, phase, before=hist, out_bytes=out_bytes))
        hist = np.concatenate([hist, np.asarray(x[a:b], dtype=np.int64)])[-(len(taps) - 1):] if len(taps) > 1 else hist
        phase = next_phase(phase, decim, b - a)
    return np.concatenate(parts)


def moving_average_clocked(samples):
    """average.py:26-33 stepped clock by clock: every register takes, on a clock edge, the value its expression had before
    the edge.  Returns x as the testbench of average.py:45-49 reads it: out[t] is x after t edges, while sample[t] is
    being presented (all registers start at 0)."""
    sr = [0, 0, 0, 0]
    sum11 = sum12 = x = 0
    out = []
    for s in samples:
        out.append(x)
        sr, sum11, sum12, x = [int(s), sr[0], sr[1], sr[2]], sr[0] + sr[1], sr[2] + sr[3], sum11 + sum12
    return np.array(out, dtype=np.int64)


def moving_average_expected(wave):
    """What the module's test compares out[6:] with (average.py:50-53)."""
    e = np.cumsum(np.asarray(wave, dtype=np.int64))
    e[4:] = e[4:] - e[:-4]
    return e[3:-3] >> 2
