"""Independent jump-ahead for the LUTOPT and PRBS streams -- TEST INFRASTRUCTURE ONLY (see oracle/bbb_oracle.h).

The product jumps with dense matrix powers A^(2^i) (csrc/gf2.hpp).  This module reaches the same positions by another
road, so that a test of a far stream position does not take its expected value from the code under test:

    A^N x0 = c(A) x0,   c = x^N mod p,   p the polynomial that annihilates A,

with c from oracle.gf2poly.modexp (Python integers) and c(A) x0 from at most k - 1 SINGLE steps of the sequential
oracle.  Nothing here imports the product package or calls its library; p itself is derived from the oracle's own
output by Berlekamp-Massey and its orientation is settled by stepping, not by convention.

For the short PRBS registers (k <= 23) there is a second route without any algebra: N mod (2^k - 1) oracle clocks.
"""
from . import gf2poly
from . import oracle as _o

MAX_N = 2 ** 64 - 1
_ann = {}
_basis = {}
_prbs_poly = {}
_prbs_basis = {}


def _annihilates(step, k, p, x0):
    """sum_j p_j A^j x0 == 0, by k single steps."""
    acc, x = 0, x0
    for j in range(k + 1):
        if (p >> j) & 1:
            acc ^= x
        if j < k:
            x = step(x)
    return acc == 0


def _derive(step, k, what):
    """The degree-k polynomial p with p(A) = 0 for the map `step` on k-bit states (bit j = coefficient of x^j)."""
    x, seq = (1 << k) - 1, []
    for _ in range(2 * k):
        x = step(x)
        seq.append(x & 1)
    c, L = gf2poly.berlekamp_massey(seq)
    if L != k:
        raise ValueError(f"{what}: linear complexity {L} != {k}: the minimal polynomial of bit 0 is not the "
                         "characteristic polynomial")
    rev = sum(((c >> i) & 1) << (k - i) for i in range(k + 1))
    starts = (1, ((0x9E3779B97F4A7C15 << max(0, k - 64)) | 5) & ((1 << k) - 1))
    good = [p for p in (c, rev) if gf2poly.degree(p) == k and all(_annihilates(step, k, p, x0) for x0 in starts)]
    if c == rev:
        good = good[:1]
    if len(good) != 1:
        raise ValueError(f"{what}: {len(good)} orientations of the connection polynomial annihilate the map")
    return good[0]


def _key(m):
    return (m.k, tuple(tuple(r) for r in m.packed))


def annihilator(m):
    """Characteristic polynomial of an oracle.Lutopt's matrix A as a Python int; cached per matrix."""
    key = _key(m)
    if key not in _ann:
        _ann[key] = _derive(m.step_int, m.k, f"LUTOPT k={m.k}")
    return _ann[key]


def _combine(c, basis):
    acc, j = 0, 0
    while c:
        if c & 1:
            acc ^= basis[j]
        c >>= 1
        j += 1
    return acc


def _krylov(step, k, init):
    b = [init]
    for _ in range(k - 1):
        b.append(step(b[-1]))
    return b


def _check_n(N):
    if not 0 <= N <= MAX_N:
        raise ValueError("position outside [0, 2^64)")


def lutopt_state(m, init, N):
    """A^N init for an oracle.Lutopt m, any init, 0 <= N < 2^64."""
    _check_n(N)
    p = annihilator(m)
    key = (_key(m), init)
    if key not in _basis:
        if len(_basis) > 64:
            _basis.clear()
        _basis[key] = _krylov(m.step_int, m.k, init)      # init, A init, ..., A^(k-1) init
    return _combine(gf2poly.modexp(p, N), _basis[key])


def prbs_step(k, s):
    return _o.prbs_bits(k, 1, state=s)[1]


def prbs_poly(k):
    """Annihilating polynomial of the PRBS-k register's state map, from the oracle's own clocks."""
    if k not in _prbs_poly:
        _prbs_poly[k] = _derive(lambda s: prbs_step(k, s), k, f"PRBS k={k}")
    return _prbs_poly[k]


def prbs_state_sequential(k, init, N):
    """The register after N clocks by clocking it: N mod (2^k - 1) oracle clocks (k <= 23)."""
    _check_n(N)
    if k > 23:
        raise ValueError("the sequential route is for k <= 23")
    return _o.prbs_bits(k, N % ((1 << k) - 1), state=init)[1]


def prbs_state(k, init, N, cross_check=False):
    """The PRBS-k register after N clocks from `init`; with cross_check (k <= 23) both routes must agree."""
    _check_n(N)
    p = prbs_poly(k)
    key = (k, init)
    if key not in _prbs_basis:
        if len(_prbs_basis) > 256:
            _prbs_basis.clear()
        _prbs_basis[key] = _krylov(lambda s: prbs_step(k, s), k, init)
    s = _combine(gf2poly.modexp(p, N), _prbs_basis[key])
    if cross_check and k <= 23:
        t = prbs_state_sequential(k, init, N)
        if s != t:
            raise AssertionError(f"PRBS{k}: polynomial route {s:#x} != sequential route {t:#x} at N={N}")
    return s
