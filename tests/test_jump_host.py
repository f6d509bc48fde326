"""The host jump-ahead (bbb_lutopt_state_at, bbb_prbs_state_at = GF2Powers in csrc/gf2.hpp) against an INDEPENDENT
jump: oracle/jump.py reaches A^N x0 as c(A) x0 with c = x^N mod p (Python integers, oracle.gf2poly) and single oracle
steps.  No matrix power is shared between the two.

Why composition alone (state_at(a + b) against state_at(b) from state_at(a)) is not enough: every polynomial in A
commutes with every other, so an exponent truncated consistently, a high A^(2^i) that repeats a lower one or a wrong
high table all compose.  The three MUTANTS at the end are such errors, put into a copy of gf2.hpp by exact text; the
comparison with the oracle must find each of them, and the test prints whether the composition identity would have.
"""
import subprocess

import pytest

import basebandboard_amd as bbb
import far
from conftest import ROOT
from oracle import jump

SIZES = (16, 32, 64, 128, 192, 256, 512)
PRBS_K = (7, 9, 11, 15, 20, 23, 31)


# ---- the oracle's own pins ----------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_oracle_annihilator(oracle, n):
    """L == k, and the polynomial annihilates A from start states the derivation did not use; the orientation is the
    one found by stepping: the bit reversal of gf2poly.lutopt_charpoly's value (whose index 0 is the leading term)."""
    m = oracle.Lutopt(path=oracle.data_path(n))
    p = jump.annihilator(m)
    assert p.bit_length() - 1 == n and p & 1
    for x0 in (2, (1 << n) - 1, far.high_init(n), 0xDEADBEEF & ((1 << n) - 1)):
        assert jump._annihilates(m.step_int, n, p, x0)
    assert not jump._annihilates(m.step_int, n, p ^ 2, 1)               # another polynomial does not
    q, L = oracle.gf2poly.lutopt_charpoly(m.packed)
    assert L == n and p == int(bin(q)[2:][::-1], 2)


@pytest.mark.parametrize("n", SIZES)
def test_oracle_jump_equals_the_sequential_oracle(oracle, n):
    m = oracle.Lutopt(path=oracle.data_path(n))
    for init in (1, far.high_init(n)):
        for N in (0, 1, 2, 63, 64, 1000, 20_011):
            assert jump.lutopt_state(m, init, N) == m.run_int(init, N), (init, N)
        if n <= 64:
            assert jump.lutopt_state(m, init, 2 ** n - 1) == init       # full period


@pytest.mark.parametrize("k", PRBS_K)
def test_oracle_prbs_jump(oracle, k):
    p = jump.prbs_poly(k)
    assert p == (1 << k) | (1 << oracle.PRBS_TAPS[k]) | 1 or p == (1 << k) | (1 << (k - oracle.PRBS_TAPS[k])) | 1
    for init in (1, (0x5A5A5A5A >> 1) & ((1 << k) - 1) | 1):
        for N in (0, 1, 2, 63, 64, 1000, 123_457):
            assert jump.prbs_state(k, init, N) == oracle.prbs_bits(k, N, state=init)[1], (init, N)
        assert jump.prbs_state(k, init, 2 ** k - 1) == init             # full period
        if k <= 23:
            assert oracle.prbs_bits(k, 2 ** k - 1, state=init)[1] == init           # ... which the sequential route relies on
            N = (5 << 48) + 12345
            assert jump.prbs_state(k, init, N) == jump.prbs_state_sequential(k, init, N)
            jump.prbs_state(k, init, 2 ** 64 - 1, cross_check=True)


# ---- the product against the oracle -------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_lutopt_state_at_equals_the_oracle_jump(oracle, n):
    m = oracle.Lutopt(path=oracle.data_path(n))
    for init in (1, far.high_init(n)):
        u = bbb.LUTOPT.shipped(n, device=-1, init=init)
        for N in far.positions():
            far.lutopt_state(u, m, N)


@pytest.mark.parametrize("k", PRBS_K)
def test_prbs_state_at_equals_the_oracle_jump(oracle, k):
    for init in (1, (0x7F6E5D4C3B2A1908 >> (64 - k)) | 1):
        p = bbb.PRBS(k, init=init)
        for N in far.positions():
            assert far.prbs_state(p, k, N) == jump.prbs_state(k, init, N, cross_check=k <= 15)


def test_state_at_of_a_matrix_that_is_not_shipped(oracle):
    """far.NONSHIPPED64 = (seed 293, candidate 3): the first full-period k = 64 matrix of that seed of the search, through
    from_packed."""
    rows = far.nonshipped64()
    m = oracle.Lutopt(packed=rows)
    assert jump.lutopt_state(m, 1, 2 ** 64 - 1) == 1
    for init in (1, far.high_init(64)):
        u = bbb.LUTOPT.from_packed(rows, device=-1, init=init)
        for N in (0, 1, 1000) + far.positions():
            far.lutopt_state(u, m, N)
        assert u.state_at(1000) == m.run_int(init, 1000)


# ---- mutants ------------------------------------------------------------------------------------

# each: (text in gf2.hpp that occurs once, its replacement, the route of jump_host that runs the mutated function)
MUTANTS = {
    # (a) GF2Powers::apply works on the low 32 bits of the exponent
    "apply_u32": ("        uint64_t v[8];\n", "        uint64_t v[8];\n        e = (uint32_t)e;\n", "apply"),
    # (b) pow2(i) returns A^(2^47) for every i above 47
    "pow2_cap47": ("return p2[(size_t)i];", "return p2[(size_t)(i < 47 ? i : 47)];", "apply"),
    # (c) GF2Powers::power drops bit 48 and up of the exponent
    "power_48": ("GF2Mat R = GF2Mat::identity(p2[0].n);", "GF2Mat R = GF2Mat::identity(p2[0].n);\n        e &= (1ull << 48) - 1;", "power"),
}
CASES = (("64", 1), ("256", 1), ("256", far.high_init(256)), ("prbs:31", 1), ("prbs:31", 0x2F00F00D))


def _target(what):
    return what if what.startswith("prbs:") else str(ROOT / "basebandboard_amd" / "data" / f"lutopt_{what}.taps")


def _run(exe, via, what, init, positions):
    r = subprocess.run([str(exe), via, _target(what), f"{init:x}"], input="".join(f"{N}\n" for N in positions), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = [int(l, 16) for l in r.stdout.split()]
    assert len(out) == len(positions)
    return out


def _oracle_states(oracle, what, init, positions):
    if what.startswith("prbs:"):
        return [jump.prbs_state(int(what[5:]), init, N) for N in positions]
    m = oracle.Lutopt(path=oracle.data_path(int(what)))
    return [jump.lutopt_state(m, init, N) for N in positions]


@pytest.fixture(scope="module")
def jump_exes(tmp_path_factory):
    text = (ROOT / "basebandboard_amd" / "csrc" / "gf2.hpp").read_text()
    exes = {}
    for name, (old, new, _) in [("as_is", ("", "", ""))] + list(MUTANTS.items()):
        d = tmp_path_factory.mktemp(name)
        if old:
            assert text.count(old) == 1, f"mutant {name}: its text occurs {text.count(old)} times in gf2.hpp (expected once)"
        (d / "gf2.hpp").write_text(text.replace(old, new) if old else text)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", str(d), str(ROOT / "tests" / "jump_host.cpp"), "-o", str(d / "jump_host")])
        exes[name] = d / "jump_host"
    return exes


@pytest.mark.parametrize("via", ("apply", "power"))
def test_unmutated_header_equals_the_oracle_at_every_position(oracle, jump_exes, via):
    """csrc/gf2.hpp as it is, outside the library: both of its jumps, every position of far.positions()."""
    cases = [(str(n), i) for n in SIZES for i in (1, far.high_init(n))] if via == "apply" else []
    for what, init in list(CASES) + cases:
        assert _run(jump_exes["as_is"], via, what, init, far.positions()) == _oracle_states(oracle, what, init, far.positions()), (what, init)


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_every_commuting_jump_error_is_found_by_the_oracle(oracle, jump_exes, name):
    """Each mutant differs from the oracle at some position of far.positions(), for every case; whether the composition
    identity of tests/test_abi.py (a = 10^17, b = 4242) notices it is printed, not asserted: a carry across the cut may
    betray a truncation, and the point is made either way."""
    via = MUTANTS[name][2]
    a, b = 10 ** 17, 4242
    for what, init in CASES:
        got = _run(jump_exes[name], via, what, init, far.positions())
        exp = _oracle_states(oracle, what, init, far.positions())
        wrong = [N for N, g, e in zip(far.positions(), got, exp) if g != e]
        assert wrong, f"mutant {name} passes the oracle comparison on {what}"
        s_a, s_ab = _run(jump_exes[name], via, what, init, [a, a + b])
        composed, = _run(jump_exes[name], via, what, s_a, [b])
        print(f"mutant {name} on {what} init {init:#x}: differs from the oracle at {len(wrong)} of {len(exp)} positions (first {min(wrong)}); "
              f"composition state_at(a+b) == state_at(b) from state_at(a): {'passes (blind)' if composed == s_ab else 'fails (notices)'}")
