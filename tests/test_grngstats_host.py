"""basebandboard_amd.grngstats on the host: the exact law of the CLT tree, the moments, Pearson's chi-square with pooled
tails and the tail table -- the evaluation half of software/clt-grng/clt-grng-evaluate.py:18-50 -- held to rational
arithmetic, to a brute-force count, to the reference script's own 100 000 samples (tests/golden/ref_clt.npz) and to the
oracle's n256 stream.  No GPU: the counting kernel's tests are tests/test_gpu_hist.py."""
import ctypes as C
import json
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN

NS = (16, 32, 64, 128, 256, 512)
# the oracle's n256 stream, 10^6 samples: (init, first_step)
STREAMS = ((1, 16), (0x1234567, 1000))
P_MIN = 1e-4      # the condition of the chi-square test: a wrong bin convention, a lost tail or a shifted mean gives p << 1e-100


@pytest.fixture(scope="module")
def stats():
    import basebandboard_amd.grngstats as S
    return S


@pytest.fixture(scope="module")
def stream_hists(oracle):
    m = oracle.Lutopt(path=oracle.data_path(256))
    out = {}
    for init, first in STREAMS:
        x = m.awgn(init, first, 10 ** 6, fast=True).astype(np.int64)
        out[(init, first)] = np.bincount(x + 128, minlength=256)
    return out


@pytest.mark.parametrize("n", NS)
def test_clt_pmf_is_a_law_with_variance_n_over_4(stats, n):
    p = stats.clt_pmf(n)
    assert len(p) == n + 1 and all(isinstance(v, Fraction) for v in p)
    assert sum(p) == 1
    assert p == p[::-1]
    assert p[n // 2] == Fraction(math.comb(n, n // 2), 1 << n)
    xs = range(-n // 2, n // 2 + 1)
    assert sum(x * v for x, v in zip(xs, p)) == 0
    assert sum(x * x * v for x, v in zip(xs, p)) == Fraction(n, 4)
    # excess kurtosis -2/n, exactly
    assert sum(x ** 4 * v for x, v in zip(xs, p)) / Fraction(n, 4) ** 2 - 3 == Fraction(-2, n)
    d = stats.clt_pmf_delivered(n)
    assert len(d) == n and sum(d) == 1
    assert d[0] == p[0] + p[n] and d[1:] == p[1:n]


def test_clt_pmf_16_equals_the_count_over_all_words(stats, oracle):
    counts = [0] * 17
    for x in range(1 << 16):
        counts[oracle.py_clt_tree(x, 16) + 8] += 1
    assert [Fraction(c, 1 << 16) for c in counts] == stats.clt_pmf(16)


def test_moments_and_the_two_lines_on_the_reference_samples(stats):
    z = np.load(GOLDEN / "ref_clt.npz")
    samples = z["samples"]
    assert samples.shape == (100000,) and int(z["n"]) == 256
    hist = np.bincount(samples.astype(np.int64) + 128, minlength=256)
    m = stats.moments(hist)
    assert m.count == 100000
    x = samples.astype(np.int64)
    assert (m.sum1, m.sum2, m.sum3, m.sum4) == (int(x.sum()), int((x ** 2).sum()), int((x ** 3).sum()), int((x ** 4).sum()))
    assert m.mean == pytest.approx(np.mean(samples), rel=1e-12)
    assert m.variance == pytest.approx(np.var(samples), rel=1e-12)
    d = x - x.mean()
    assert m.skewness == pytest.approx((d ** 3).mean() / (d ** 2).mean() ** 1.5, rel=1e-9)
    assert m.excess_kurtosis == pytest.approx((d ** 4).mean() / (d ** 2).mean() ** 2 - 3, rel=1e-9)
    ev = stats.evaluate_samples(samples, 256)
    assert ev.moments == m and ev.nsamples == 100000 and ev.hist == tuple(hist.tolist())
    assert (ev.theoretical_mean, ev.theoretical_variance, ev.theoretical_excess_kurtosis) == (0.0, 64.0, -2 / 256)
    lines = str(ev).splitlines()
    # formatted exactly as the reference formats them (clt-grng-evaluate.py:30-31) ...
    assert lines[0] == "Theoretical mean μ={:.4e}, variance σ²={:.4e}.".format(0, 2 ** (8 - 2))
    assert lines[1] == "Sample mean μ={:.4e}, variance σ²={:.4e}.".format(np.mean(samples), np.sqrt(np.var(samples)) ** 2)
    # ... and equal to what the reference script itself printed for these samples
    assert lines[:2] == json.load(open(GOLDEN / "ref_clt_meta.json"))["printed"]
    # an un-truncated +128 is counted where the generator's port delivers it
    assert stats.evaluate_samples(np.array([128, -128, 0]), 256).hist[0] == 2
    pdf, cdf = stats.pdf_cdf(hist)
    assert pdf.shape == cdf.shape == (256,) and pdf.sum() == pytest.approx(1.0) and cdf[-1] == 1.0
    assert np.array_equal(pdf, hist / 100000) and np.allclose(cdf, np.cumsum(hist) / 100000, rtol=0, atol=1e-15)


@pytest.mark.parametrize("key", STREAMS)
def test_chi_square_accepts_the_oracle_stream(stats, stream_hists, key):
    hist = stream_hists[key]
    r = stats.chi_square(hist, 256, min_expected=5.0)
    stat, dof, p = r
    print(f"stream {key}: {r}")
    assert (stat, dof, p) == (r.statistic, r.dof, r.p_value) and r.method in ("scipy", "math")
    # the pooling rule: every cell expects at least min_expected; dof = cells - 1 (70 for n = 256 at this N)
    assert all(e >= 5.0 for _, _, _, e in r.cells)
    assert dof == len(r.cells) - 1 == 70
    assert sum(o for _, _, o, _ in r.cells) == 10 ** 6 and math.fsum(e for _, _, _, e in r.cells) == pytest.approx(1e6, rel=1e-12)
    assert r.cells[0][0] == 0 and r.cells[-1][1] == 255 and all(a == b for a, b, _, _ in r.cells[1:-1])
    assert p >= P_MIN


@pytest.mark.parametrize("key", STREAMS)
def test_chi_square_rejects_shifted_bins_and_a_lost_tail(stats, stream_hists, key):
    hist = stream_hists[key]
    shifted = np.roll(hist, 1)
    assert stats.chi_square(shifted, 256)[2] < P_MIN
    lost = hist.copy()
    x = np.arange(256) - 128
    lost[np.abs(x) >= 32] = 0
    assert lost.sum() < hist.sum()
    assert stats.chi_square(lost, 256)[2] < P_MIN


def test_chi_square_p_value_is_the_same_with_scipy_and_without(stats, stream_hists):
    pytest.importorskip("scipy.stats")
    for hist in stream_hists.values():
        a = stats.chi_square(hist, 256, use_scipy=True)
        b = stats.chi_square(hist, 256, use_scipy=False)
        assert (a.method, b.method) == ("scipy", "math")
        assert a.statistic == b.statistic and a.dof == b.dof
        assert b.p_value == pytest.approx(a.p_value, rel=1e-9)
    from scipy.stats import chi2
    for stat, dof in ((0.5, 1), (3.0, 2), (63.81, 70), (69.69, 70), (75.02, 84), (200.0, 70), (30.0, 84), (1000.0, 510), (400.0, 510)):
        assert stats.chi2_sf(stat, dof, use_scipy=False)[0] == pytest.approx(float(chi2.sf(stat, dof)), rel=1e-9), (stat, dof)


def test_tail_table_counts_and_expects_exactly(stats, stream_hists):
    hist = stream_hists[STREAMS[0]]
    rows = stats.tail_table(hist, 256)
    assert [r.t for r in rows] == list(range(1, 17))              # sigma = 8, the range ends at 16 sigma
    x = np.arange(256) - 128
    p = stats.clt_pmf_delivered(256)
    for r in rows:
        sel = np.abs(x) >= 8 * r.t
        assert r.observed == int(hist[sel].sum())
        assert r.expected_exact == 10 ** 6 * sum(p[b] for b in np.nonzero(sel)[0])
        assert r.expected == float(r.expected_exact)
    assert rows[0].expected == pytest.approx(0.3486e6, rel=0.01)   # |x| >= 8 of the lattice law: the Gaussian's 2 Q(7.5 / 8)
    # a sigma that is no integer (n = 32: sigma = 2.83): |x| >= t sigma is 4 x^2 >= t^2 n
    r32 = stats.tail_table([0] * 15 + [1, 1] + [0] * 15, 32)
    assert [r.t for r in r32] == [1, 2, 3, 4, 5] and r32[0].observed == 0
    assert r32[0].expected_exact == 2 * sum(stats.clt_pmf_delivered(32)[b] for b in range(32) if abs(b - 16) >= 3)


def test_awgn_hist_argument_checks_that_need_no_gpu():
    import basebandboard_amd as bbb
    from basebandboard_amd import _lib
    l = _lib.lib()
    u = bbb.LUTOPT.shipped(256, device=-1)
    counters = (C.c_uint64 * 256)()
    ptr = C.cast(counters, C.c_void_p)
    assert l.bbb_awgn_hist(u._h, ptr, 1000, 0) == _lib.BBB_ENODEV
    assert l.bbb_awgn_hist(u._h, None, 1000, 0) == _lib.BBB_EINVAL
    assert l.bbb_awgn_hist(None, ptr, 1000, 0) == _lib.BBB_EINVAL
    assert l.bbb_awgn_hist(u._h, C.c_void_p(ptr.value + 4), 1000, 0) == _lib.BBB_EINVAL
    assert l.bbb_awgn_hist(bbb.LUTOPT.shipped(192, device=-1)._h, ptr, 1000, 0) == _lib.BBB_EUNSUP
    assert not any(counters)
