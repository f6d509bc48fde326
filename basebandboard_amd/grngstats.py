"""Statistical evaluation of the CLT noise generator -- the second half of software/clt-grng/clt-grng-evaluate.py:18-50.

The reference draws 100 000 samples, prints the sample mean and variance beside the theoretical ones and plots the
empirical PDF and CDF.  Here the counting is the GPU's (`CLTGRNG.histogram`, bbb_awgn_hist: the samples never leave the
chip, so 1e12 of them -- the depth at which a BER of 1e-12 is decided -- take about a second), and what the counts are
held against is the EXACT law instead of a matched Gaussian:

  the tree is sum_i (-1)^popcount(i) x[i] (rng.py:96-105), for independent fair bits Binomial(n/2) - Binomial(n/2)
  = Binomial(n, 1/2) - n/2, so  P(v) = C(n, v + n/2) / 2^n,  v = -n/2 .. n/2:  mean 0, variance n/4 (the reference's
  2^(log2 n - 2)), excess kurtosis -2/n.  The DELIVERED sample is v truncated to log2(n) bits (rng.py:78): +n/2 reads -n/2.

  clt_pmf(n), clt_pmf_delivered(n)   the two laws as exact fractions
  moments(hist)                      exact integer sums; mean, variance (np.var's population form), skewness, excess kurtosis
  chi_square(hist, n)                Pearson's statistic against clt_pmf_delivered, tails pooled; (statistic, dof, p-value)
  tail_table(hist, n)                observed and exactly expected counts of |x| >= t sigma
  pdf_cdf(hist)                      the two normalised arrays the reference plots (plotting is the caller's business)
  evaluate(grng, nsamples)           all of it over a range of the stream, counted on the GPU
  evaluate_samples(samples, n)       the same from samples on the host (the reference's own 100 000, a capture)

Bin b of a histogram of n bins holds the delivered sample x = b - n/2.  Everything but `evaluate` is host arithmetic on the
counters in Python integers and fractions: no float enters before the last division.
"""
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

__all__ = ["clt_pmf", "clt_pmf_delivered", "moments", "chi_square", "tail_table", "pdf_cdf", "evaluate", "evaluate_samples",
           "Moments", "ChiSquare", "TailRow", "Evaluation", "chi2_sf"]


def _check_n(n):
    n = int(n)
    if n < 2 or n & (n - 1):
        raise ValueError("n must be a power of two >= 2 (rng.py:72-76)")
    return n


def clt_pmf(n):
    """The exact law of the UN-truncated tree value: a list of n + 1 Fractions, entry i = P(v = i - n/2) = C(n, i) / 2^n."""
    n = _check_n(n)
    return [Fraction(math.comb(n, i), 1 << n) for i in range(n + 1)]


def clt_pmf_delivered(n):
    """The law of the delivered sample, matching the histogram's bins: n Fractions, entry b = P(x = b - n/2), with the
    tree value +n/2 folded onto -n/2 (bin 0) as the log2(n)-bit Signal wraps it."""
    p = clt_pmf(n)
    return [p[0] + p[n]] + p[1:n]


def _counts(hist):
    """the counters as a tuple of Python integers (from a torch tensor on any device, a numpy array or a sequence)"""
    if hasattr(hist, "detach"):
        hist = hist.detach().cpu().numpy()
    a = np.asarray(hist)
    if a.dtype == np.int64:
        a = a.view(np.uint64)          # (counters handed over as an int64 tensor hold the same bit patterns)
    if a.ndim != 1:
        raise ValueError("hist must be one-dimensional: n counters")
    c = tuple(int(v) for v in a.tolist())
    _check_n(len(c))
    if any(v < 0 for v in c):
        raise ValueError("negative count")
    return c


@dataclass(frozen=True)
class Moments:
    """Exact sums over the histogram (x = bin - n/2) and what follows from them.  variance is the population form
    (np.var, as the reference prints it); skewness = m3 / m2^1.5, excess_kurtosis = m4 / m2^2 - 3 of the central moments."""
    count: int
    sum1: int
    sum2: int
    sum3: int
    sum4: int
    mean: float
    variance: float
    skewness: float
    excess_kurtosis: float


def moments(hist):
    c = _counts(hist)
    half = len(c) // 2
    N = sum(c)
    s1 = sum(v * (b - half) for b, v in enumerate(c))
    s2 = sum(v * (b - half) ** 2 for b, v in enumerate(c))
    s3 = sum(v * (b - half) ** 3 for b, v in enumerate(c))
    s4 = sum(v * (b - half) ** 4 for b, v in enumerate(c))
    if N == 0:
        return Moments(0, 0, 0, 0, 0, math.nan, math.nan, math.nan, math.nan)
    mu = Fraction(s1, N)
    m2 = Fraction(s2, N) - mu ** 2
    m3 = Fraction(s3, N) - 3 * mu * Fraction(s2, N) + 2 * mu ** 3
    m4 = Fraction(s4, N) - 4 * mu * Fraction(s3, N) + 6 * mu ** 2 * Fraction(s2, N) - 3 * mu ** 4
    skew = float(m3) / float(m2) ** 1.5 if m2 else math.nan
    kurt = float(m4 / (m2 * m2) - 3) if m2 else math.nan
    return Moments(N, s1, s2, s3, s4, float(mu), float(m2), skew, kurt)


def _gamma_q(a, x):
    """Regularised upper incomplete gamma Q(a, x) in `math` alone: the series of P for x < a + 1, Lentz's continued
    fraction of Q otherwise (both converge to the last bit in a few hundred terms for the a, x of a chi-square test)."""
    if x <= 0:
        return 1.0
    lead = -x + a * math.log(x) - math.lgamma(a)
    if x < a + 1:
        term = total = 1.0 / a
        k = a
        for _ in range(100000):
            k += 1
            term *= x / k
            total += term
            if term < total * 1e-17:
                break
        return max(0.0, 1.0 - total * math.exp(lead))
    tiny = 1e-300
    b = x + 1 - a
    c = 1 / tiny
    d = 1 / b
    h = d
    for i in range(1, 100000):
        an = -i * (i - a)
        b += 2
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1 / d
        delta = d * c
        h *= delta
        if abs(delta - 1) < 1e-16:
            break
    return h * math.exp(lead) if lead > -745 else 0.0


def chi2_sf(statistic, dof, use_scipy=None):
    """(p-value, method): the chi-square survival function from scipy.stats where it imports ("scipy"), from the
    incomplete gamma function written in `math` otherwise ("math").  use_scipy = False / True forces one of them."""
    if use_scipy is None or use_scipy:
        try:
            from scipy.stats import chi2
            return float(chi2.sf(statistic, dof)), "scipy"
        except ImportError:
            if use_scipy:
                raise
    return _gamma_q(dof / 2.0, statistic / 2.0), "math"


class ChiSquare(tuple):
    """(statistic, dof, p_value), with the same under their names, `method` ("scipy" or "math": what computed the
    p-value), and the pooled cells: `cells` = [(first bin, last bin, observed, expected)]."""

    def __new__(cls, statistic, dof, p_value, method, cells):
        self = super().__new__(cls, (statistic, dof, p_value))
        self.statistic, self.dof, self.p_value, self.method, self.cells = statistic, dof, p_value, method, cells
        return self

    def __str__(self):
        return f"chi-square = {self.statistic:.2f} at {self.dof} degrees of freedom, p = {self.p_value:.4g} ({self.method})"


def chi_square(hist, n=None, min_expected=5.0, use_scipy=None):
    """Pearson's statistic of the counters against clt_pmf_delivered(n).  The tail bins on each side are pooled from the
    outside inwards until the pooled expected count reaches min_expected; every bin between the two pools is a cell of
    its own; dof = cells - 1.  Returns ChiSquare = (statistic, dof, p-value)."""
    c = _counts(hist)
    n = len(c) if n is None else _check_n(n)
    if len(c) != n:
        raise ValueError(f"the histogram of the n = {n} generator has {n} bins (got {len(c)})")
    N = sum(c)
    if N == 0:
        raise ValueError("empty histogram")
    expected = [float(N * p) for p in clt_pmf_delivered(n)]
    lo, acc = 0, expected[0]
    while acc < min_expected and lo < n - 2:
        lo += 1
        acc += expected[lo]
    hi, acc = n - 1, expected[n - 1]
    while acc < min_expected and hi > lo + 1:          # (too few samples for two such pools: they meet, and two cells remain)
        hi -= 1
        acc += expected[hi]
    spans = [(0, lo)] + [(b, b) for b in range(lo + 1, hi)] + [(hi, n - 1)]
    cells = [(a, b, sum(c[a:b + 1]), math.fsum(expected[a:b + 1])) for a, b in spans]
    stat = math.fsum((o - e) ** 2 / e for _, _, o, e in cells)
    dof = len(cells) - 1
    p, method = chi2_sf(stat, dof, use_scipy)
    return ChiSquare(stat, dof, p, method, cells)


@dataclass(frozen=True)
class TailRow:
    """|x| >= t sigma (sigma^2 = n/4, i.e. 4 x^2 >= t^2 n): the samples seen there and the number the exact law expects"""
    t: int
    observed: int
    expected: float
    expected_exact: Fraction


def tail_table(hist, n=None):
    """For t = 1, 2, ... (while t sigma <= n/2): observed and exactly expected number of samples with |x| >= t sigma,
    under the delivered law (x = -n/2 holds the folded +n/2).  The table a reader looks at for the tails."""
    c = _counts(hist)
    n = len(c) if n is None else _check_n(n)
    if len(c) != n:
        raise ValueError(f"the histogram of the n = {n} generator has {n} bins (got {len(c)})")
    N = sum(c)
    p = clt_pmf_delivered(n)
    half = n // 2
    rows = []
    t = 1
    while t * t * n <= 4 * half * half:
        inside = [b for b in range(n) if 4 * (b - half) ** 2 >= t * t * n]
        exact = N * sum((p[b] for b in inside), Fraction(0))
        rows.append(TailRow(t, sum(c[b] for b in inside), float(exact), exact))
        t += 1
    return tuple(rows)


def pdf_cdf(hist):
    """(pdf, cdf): the counters normalised to sum 1 and their running sum, float64 arrays over x = -n/2 .. n/2 - 1: the
    empirical PDF and CDF the reference plots (clt-grng-evaluate.py:34-35, 43-44)."""
    c = _counts(hist)
    N = sum(c)
    if N == 0:
        raise ValueError("empty histogram")
    run, cum = 0, []
    for v in c:
        run += v
        cum.append(run)
    return np.array([v / N for v in c], dtype=np.float64), np.array([v / N for v in cum], dtype=np.float64)


@dataclass(frozen=True)
class Evaluation:
    """What clt-grng-evaluate.py shows of a generator, in numbers.  `hist`: the n counters (bin = x + n/2)."""
    n: int
    nsamples: int
    hist: tuple
    moments: Moments
    chi2: ChiSquare
    tails: tuple
    theoretical_mean: float
    theoretical_variance: float
    theoretical_excess_kurtosis: float

    def __str__(self):
        m = self.moments
        lines = [
            # the reference's own two lines (clt-grng-evaluate.py:30-31)
            "Theoretical mean μ={:.4e}, variance σ²={:.4e}.".format(self.theoretical_mean, self.theoretical_variance),
            "Sample mean μ={:.4e}, variance σ²={:.4e}.".format(m.mean, m.variance),
            f"{self.nsamples} samples of the n = {self.n} generator; skewness {m.skewness:.4e} (0), "
            f"excess kurtosis {m.excess_kurtosis:.4e} ({self.theoretical_excess_kurtosis:.4e})",
            str(self.chi2),
            "|x| >= t sigma:  t  observed  expected",
        ]
        lines += [f"  {r.t:2d}  {r.observed}  {r.expected:.6g}" for r in self.tails]
        return "\n".join(lines)


def _evaluation(c, n):
    return Evaluation(n, sum(c), c, moments(c), chi_square(c, n), tail_table(c, n), 0.0, n / 4.0, -2.0 / n)


def evaluate_samples(samples, n):
    """The evaluation of samples on the host (any integer array of tree values or delivered samples: a value is counted
    in bin (x + n/2) mod n, as the generator's output port truncates it)."""
    n = _check_n(n)
    x = np.asarray(samples.cpu() if hasattr(samples, "cpu") else samples).astype(np.int64).ravel()
    if x.size and (x.min() < -n // 2 or x.max() > n // 2):
        raise ValueError(f"samples outside the tree's range -{n // 2} .. {n // 2}")
    return _evaluation(tuple(int(v) for v in np.bincount((x + n // 2) % n, minlength=n).tolist()), n)


def evaluate(lutopt_or_grng, nsamples, first_step=0, chunk=1 << 36):
    """The evaluation of samples first_step .. first_step + nsamples - 1 of the generator's stream, counted on the GPU
    (`CLTGRNG.histogram` in calls of `chunk` samples, which add into one set of counters)."""
    from .rng import CLTGRNG
    g = lutopt_or_grng if isinstance(lutopt_or_grng, CLTGRNG) else CLTGRNG(lutopt_or_grng)
    nsamples, first_step, chunk = int(nsamples), int(first_step), int(chunk)
    if nsamples < 1 or chunk < 1:
        raise ValueError("nsamples and chunk must be positive")
    out = None
    for off in range(0, nsamples, chunk):
        out = g.histogram(min(chunk, nsamples - off), first_step + off, out=out)
    return _evaluation(_counts(out), g.n)
