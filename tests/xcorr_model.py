"""numpy int64 model of the data-to-waveform correlation of include/bbb.h (bbb_xcorr_accumulate_i16), written from the
definition: lag by lag, the samples of the lag's residue gathered with one strided slice.

  for every sample n in [first_sample, first_sample + len(x)) and every lag l < nlags with n - origin - l = spb * m, m >= 0:
      xc[l] += s[m] * x[n]        s[m] = +1 for data bit 1, -1 for data bit 0
"""
import numpy as np


def pack(bits):
    """0/1 values packed LSB first into u64 words, the unused bits of the last word 0."""
    b = np.zeros((len(bits) + 63) // 64 * 64, dtype=np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint64)


def needed_bits(first_sample, nsamples, spb, origin, nlags):
    """(lo, hi) inclusive: the data bits the samples need; hi < lo: none."""
    hi = (first_sample + nsamples - 1 - origin) // spb
    lo = max(0, (first_sample - origin - (nlags - 1)) // spb)
    return lo, hi


def xcorr(x, first_sample, bits, bit0, spb, origin, nlags):
    """(xc, counts), int64 [nlags] each.  x: the samples first_sample ..; bits: 0/1 values of data bits bit0 .. (unpacked)."""
    x = np.asarray(x, dtype=np.int64)
    bits = np.asarray(bits, dtype=np.int64)
    xc, counts = np.zeros(nlags, dtype=np.int64), np.zeros(nlags, dtype=np.int64)
    for l in range(nlags):
        # the first sample of the call that lag l takes: at or above origin + l (bit 0) and congruent to it modulo spb
        n0 = max(first_sample, origin + l)
        n0 += (origin + l - n0) % spb
        i0 = n0 - first_sample
        if i0 >= len(x):
            continue
        xs = x[i0::spb]
        m0 = (n0 - origin - l) // spb
        assert (n0 - origin - l) % spb == 0 and m0 >= 0
        s = 2 * bits[m0 - bit0:m0 - bit0 + len(xs)] - 1
        assert len(s) == len(xs), "the bits do not cover the samples"
        xc[l] = int((s * xs).sum())
        counts[l] = len(xs)
    return xc, counts


def brute(x, first_sample, bits, bit0, spb, origin, nlags):
    """The definition, term by term (small cases only)."""
    xc, counts = [0] * nlags, [0] * nlags
    for i, v in enumerate(x):
        n = first_sample + i
        for l in range(nlags):
            d = n - origin - l
            if d % spb == 0 and d >= 0:
                xc[l] += (1 if bits[d // spb - bit0] else -1) * int(v)
                counts[l] += 1
    return np.array(xc, dtype=np.int64), np.array(counts, dtype=np.int64)


# The closed loop measure -> design -> apply -> verify at the README's setting (PRBS-7, roll-off 0.5, noise_var 15, samples
# [0, 2^20)) and what it gives on the CPU oracle's waveform (tests/test_xcorr_host.py computes and asserts these): the designed
# taps, their delay, and the errors per bathtub phase behind them.  tests/test_gpu_xcorr.py holds the GPU's closed loop to the same.
LOOP = dict(k=7, beta=0.5, noise_var=15, n=1 << 20, nlags=64, ntaps=12, cursor=37)
LOOP_RAW_BEST, LOOP_MA_BEST = 2491, 3
LOOP_DESIGNED = [33900, 7657, 367, 0, 0, 4, 343, 7000]
LOOP_TAPS = [-42, 40, 121, 190, 236, 256, 244, 205, 142, 68, -9, -79]
LOOP_DELAY = 5
