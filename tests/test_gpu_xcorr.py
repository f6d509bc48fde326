"""The data-to-waveform correlation on the GPU, exact: the capture side against the numpy model of tests/xcorr_model.py (every
spb, sizes around the tile and vector edges, lag counts around the lag-group edges, placements with terms below bit 0, bits
that begin above 0, an unaligned sample pointer), additivity, full-scale samples, the transmitter side against the capture
side over TX.generate, the noise-free pulse response against the coefficients, and the closed loop measure -> design ->
apply -> verify against what the CPU closed loop of tests/test_xcorr_host.py records."""
import numpy as np
import pytest
import torch

import basebandboard_amd as bbb
from basebandboard_amd import equalizer
from basebandboard_amd.bitshaper import PRBSShaper, rcf_coefficients
from basebandboard_amd.txsweep import TxSetting

import xcorr_model as M
from xcorr_model import LOOP, LOOP_DELAY, LOOP_DESIGNED, LOOP_TAPS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

SIZES = (1, 7, 8, 63, 64, 65, 4097, (1 << 16) + 3, (1 << 20) + 5)


def i64(t):
    return t.cpu().numpy()


def packed(bits):
    return torch.from_numpy(M.pack(bits).view(np.int64)).to(DEV)


def gpu_xcorr(x, bits, spb, origin, nlags, first, bit0, off=0, xc=None):
    """x: int16 numpy samples first ..; bits: 0/1 values of data bits bit0 ..; off: elements in front of the samples in
    their tensor, which moves the pointer off the 16-byte boundary"""
    t = torch.from_numpy(np.concatenate([np.zeros(off, dtype=np.int16), x])).to(DEV)
    return bbb.capture_xcorr(t[off:], packed(bits), spb, origin, nlags, first, bit0, xc)


@pytest.fixture(scope="module")
def record():
    """One random full-range record and one random bit stream, shared and never changed."""
    rng = np.random.default_rng(2024)
    x = rng.integers(-32768, 32768, (1 << 20) + 5, dtype=np.int64).astype(np.int16)
    x[::1001] = -32768
    x[7::997] = 32767
    bits = rng.integers(0, 2, (1 << 20) + 2048).astype(np.uint8)
    x.setflags(write=False)
    bits.setflags(write=False)
    return x, bits


def lag_counts(spb):
    # 8 spb + 1 and 16 spb + 1: the first lag counts of the 16- and the 32-group kernel
    return sorted({1, spb, spb + 1, 8 * spb + 1, 16 * spb + 1, min(64, 64 * spb), min(65, 64 * spb), min(256, 64 * spb)} | ({512} if spb == 8 else set())
                  | ({1024} if spb == 16 else set()))


@pytest.mark.parametrize("spb", (1, 4, 8, 16, 32))
def test_capture_vs_model(gpu, record, spb):
    x, bits = record
    for n in SIZES:
        for nlags in lag_counts(spb):
            # A: far from bit 0, first_sample no multiple of spb, the bits handed over from one bit below the first needed
            #    one (bit0 > 0), the sample pointer 2 bytes off;  B: the origin above first_sample, so that terms below bit 0
            #    exist (for the smallest sizes every sample lies below it)
            for first, origin, off in ((1000 * spb + 3, 17, 1), (3, 3 + 2 * spb + 1, 0)):
                lo, hi = M.needed_bits(first, n, spb, origin, nlags)
                bit0 = max(0, lo - 1)
                b = bits[:max(0, hi - bit0 + 1)]
                want = M.xcorr(x[:n], first, b, bit0, spb, origin, nlags)[0]
                got = gpu_xcorr(x[:n], b, spb, origin, nlags, first, bit0, off)
                assert np.array_equal(i64(got), want), (n, nlags, first, origin)


def test_first_bits_of_the_stream(gpu, record):
    """Ranges that begin at, just before and just after bit 0's first sample, and m = 0 at a call's first and last sample"""
    x, bits = record
    for spb, nlags in ((8, 64), (8, 512), (1, 64), (32, 1024), (16, 1024), (4, 5)):
        origin = 50
        for first, n in ((origin, 1), (origin - 1, 2), (origin - 1, 1), (origin + 1, 3 * spb), (0, origin + nlags + 5 * spb),
                         (origin + nlags - 1, 1), (origin + nlags - 1 - spb, spb + 1), (origin + 64 * spb - 3, 9000)):
            lo, hi = M.needed_bits(first, n, spb, origin, nlags)
            b = bits[:max(0, hi + 1)]
            want = M.xcorr(x[:n], first, b, 0, spb, origin, nlags)[0]
            got = gpu_xcorr(x[:n], b, spb, origin, nlags, first, 0)
            assert np.array_equal(i64(got), want), (spb, nlags, first, n)


def test_additivity_and_added_to(gpu, record):
    """One call = the range cut at three arbitrary points; the counters start nonzero and are added to"""
    x, bits = record
    for spb, nlags, first, origin in ((8, 256, 5, 17), (16, 1024, 12_345, 40), (1, 33, 0, 9)):
        n = 300_007
        lo, hi = M.needed_bits(first, n, spb, origin, nlags)
        b = bits[:hi + 1]
        start = np.arange(nlags, dtype=np.int64) * 1_000_003 - 77
        whole = gpu_xcorr(x[:n], b, spb, origin, nlags, first, 0, xc=torch.from_numpy(start.copy()).to(DEV))
        assert np.array_equal(i64(whole), start + M.xcorr(x[:n], first, b, 0, spb, origin, nlags)[0])
        acc = torch.from_numpy(start.copy()).to(DEV)
        cuts = (0, 1, 70_001, 200_002, n)
        for a, e in zip(cuts[:-1], cuts[1:]):
            plo, phi = M.needed_bits(first + a, e - a, spb, origin, nlags)
            gpu_xcorr(x[a:e], bits[plo:phi + 1], spb, origin, nlags, first + a, plo, off=a % 5, xc=acc)
        assert torch.equal(acc, whole)


@pytest.mark.parametrize("value", (-32768, 32767))
def test_full_scale_samples(gpu, value):
    """2^20 samples at full scale against bits all 1, all 0 and alternating: the true sums are +-2^35, so a sum kept in 32 bits
    anywhere between the lanes' partials and the counters fails here.  The grid spreads these samples over so many workgroups
    that no lane comes near the 2^16 steps after which unflushed int32 partials would wrap: the flush is covered by the host
    run of the same per-lane code under UBSan (tests/test_xcorr_host.py: every lane width, and a build without the flush
    that must fail), not by this test."""
    n, spb, origin, nlags = 1 << 20, 8, 17, 64
    x = np.full(n, value, dtype=np.int16)
    for name, b in (("ones", np.ones(n // 8 + 1, dtype=np.uint8)), ("zeros", np.zeros(n // 8 + 1, dtype=np.uint8)),
                    ("alternating", (np.arange(n // 8 + 1) & 1).astype(np.uint8))):
        want = M.xcorr(x, 0, b, 0, spb, origin, nlags)[0]
        got = gpu_xcorr(x, b, spb, origin, nlags, 0, 0)
        assert np.array_equal(i64(got), want), name
        if name != "alternating":
            assert abs(int(want[0])) > 1 << 31


# ---- transmitter side ------------------------------------------------------------------------------------------------

def make_tx(k=7, bit_en=1, src=0, shape=16, noise_en=1, nv=8, taps=None):
    tx = bbb.TX(k, bit_en, src, shape, noise_en, nv, device=0)
    if taps is not None:
        tx.prbs_shaper = PRBSShaper(tx.prbs, 0, [taps])
        tx.pulse_shaper = PRBSShaper(bbb.Pulser(), 0, [taps])
    return tx


def source_bits(tx, lo, count):
    """packed data bits lo .. lo + count - 1 of the TX's source, as an int64 CUDA tensor"""
    if tx.src_sel:
        return packed(((lo + np.arange(count)) & 255) == 0)
    return bbb.PRBS(tx.prbs.k, device=0).generate(count, first_bit=lo)


TX_CASES = [
    # (name, make_tx kwargs, first, nsamples, nlags, chunk)
    ("prbs7_noise", dict(k=7, nv=8), 0, 200_003, 64, 0),
    ("prbs31_noise_three_chunks", dict(k=31, nv=15, shape=31), 12_345, (1 << 15) + 77, 64, 1 << 14),
    ("prbs7_noise_off", dict(k=7, noise_en=0, shape=8), 3, 100_001, 512, 0),
    ("prbs31_noise_off_three_chunks", dict(k=31, noise_en=0), 1 << 20, (1 << 15) + 77, 65, 1 << 14),
    ("pulser", dict(src=1, nv=4, shape=20), 44, (1 << 15) + 77, 256, 1 << 14),
    ("pulser_noise_off", dict(src=1, noise_en=0, shape=20), 0, 70_000, 9, 0),
]


@pytest.mark.parametrize("name, kw, first, n, nlags, chunk", TX_CASES, ids=[c[0] for c in TX_CASES])
def test_tx_xcorr_equals_capture_over_generate(gpu, name, kw, first, n, nlags, chunk):
    start = torch.arange(nlags, dtype=torch.int64, device=DEV) * 12_347 - 5
    with bbb.TxXcorr(make_tx(**kw), nlags=nlags, chunk_samples=chunk) as t:
        got = t.run(n, first, xcorr=start.clone())
    tx = make_tx(**kw)
    x = tx.generate(n, first_sample=first)
    lo, hi = M.needed_bits(first, n, 8, bbb.TX_BIT_ORIGIN, nlags)
    want = bbb.capture_xcorr(x, source_bits(tx, lo, hi - lo + 1), 8, bbb.TX_BIT_ORIGIN, nlags, first, lo, xcorr=start.clone())
    assert torch.equal(got, want)
    assert i64(want - start).any()
    if chunk == 0 and first == 0:
        assert torch.equal(bbb.tx_xcorr(make_tx(**kw), n, nlags=nlags), got - start)


def test_pulser_bits_are_where_the_waveform_has_its_pulses(gpu):
    """What ties the Pulser's data bits, (m & 255) == 0, to the waveform itself: with the noise off every bit but each 256th
    is 0, so sample 17 + 8 m + l of a set bit m differs from the sample 800 earlier (same residue, only 0 bits in reach) by
    2 coeffs[l].  The counters of such a waveform then equal the model's for exactly those bits."""
    c = rcf_coefficients(0.5)
    tx = make_tx(src=1, noise_en=0, taps=c)
    first, n = bbb.TX_BIT_ORIGIN + 8 * 400, 8 * 300
    x = tx.generate(n, first_sample=first).cpu().numpy().astype(np.int64)
    idx = bbb.TX_BIT_ORIGIN + 8 * 512 + np.arange(64) - first
    assert np.array_equal(x[idx] - x[idx - 800], 2 * np.array(c))
    lo, hi = M.needed_bits(first, n, 8, bbb.TX_BIT_ORIGIN, 64)
    bits = ((lo + np.arange(hi - lo + 1)) & 255) == 0
    want = M.xcorr(x, first, bits, lo, 8, bbb.TX_BIT_ORIGIN, 64)[0]
    assert np.array_equal(i64(bbb.tx_xcorr(make_tx(src=1, noise_en=0, taps=c), n, first_sample=first, nlags=64)), want)
    flipped = M.xcorr(x, first, np.roll(bits, 1), lo, 8, bbb.TX_BIT_ORIGIN, 64)[0]
    assert not np.array_equal(flipped, want)


def test_noise_free_pulse_response_is_the_coefficient_set(gpu):
    """64 whole periods of PRBS-7 (127 * 64 bits), from a sample at which every lag has its bit: each lag has 127 * 64 terms,
    the m-sequence's off-peak correlation is -1 / 127, so h[l] = c[l] - sum_{k != 0} c[l + 8 k] / 127, within
    max |c| * 2 / 127 of c[l]"""
    c = rcf_coefficients(0.5)
    tx = make_tx(k=7, noise_en=0, taps=c)
    first, n = bbb.TX_BIT_ORIGIN + 8 * 8, 127 * 64 * 8
    assert np.array_equal(bbb.xcorr_counts(first, n, 8, bbb.TX_BIT_ORIGIN, 64), np.full(64, 127 * 64))
    h = tx.pulse_response(n, nlags=64, first_sample=first)
    assert h.dtype == np.float64 and h.shape == (64,)
    err = np.abs(h - np.array(c, dtype=np.float64))
    print("largest deviation", err.max(), "bound", max(abs(v) for v in c) * 2 / 127)
    assert err.max() <= max(abs(v) for v in c) * 2 / 127
    # RX.pulse_response over the generated waveform is the same estimate
    x = tx.generate(n, first_sample=first)
    lo, hi = M.needed_bits(first, n, 8, bbb.TX_BIT_ORIGIN, 64)
    h2 = bbb.RX(7, 8, 0).pulse_response(x, source_bits(tx, lo, hi - lo + 1), bbb.TX_BIT_ORIGIN, first_sample=first, bit0=lo)
    assert np.array_equal(h, h2)


def test_closed_loop(gpu):
    """Measure (TX.pulse_response, TX.acf), design (FIR.mmse), apply and verify (LinkSweep) at the README's setting: the same
    taps, delay and errors per phase as the CPU closed loop on the oracle's waveform records"""
    n = LOOP["n"]
    tx = make_tx(k=LOOP["k"], nv=LOOP["noise_var"], taps=rcf_coefficients(LOOP["beta"]))
    h = tx.pulse_response(n, nlags=LOOP["nlags"])
    acf0 = int(i64(tx.acf(n, nlags=1))[0])
    sigma2 = equalizer.noise_power(acf0, n, h, 8)
    fir = bbb.FIR.mmse(h, 8, LOOP["cursor"], LOOP["ntaps"], sigma2)
    assert fir.taps == LOOP_TAPS and fir.design_delay == LOOP_DELAY
    st = TxSetting(noise_var=tx.noise_var, bit_en=tx.bit_en, noise_en=tx.noise_en)
    with bbb.LinkSweep(tx, [st], fir) as s:                 # no delay given: the design's
        assert s.delay == LOOP_DELAY
        tub = i64(s.run(n)).view(np.uint64)[0]
    print("errors per phase", tub[:, 1].tolist())
    assert tub[:, 1].tolist() == LOOP_DESIGNED
    assert int(tub[:, 1].min()) == min(LOOP_DESIGNED)
