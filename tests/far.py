"""Far stream positions for the tests: the oracle's independently derived state (oracle/jump.py: x^N mod p with Python
integers, applied by single oracle steps), with the product's own jump-ahead held to it on the way.

A test that needs the state at a position the sequential oracle cannot step to calls `lutopt_state` / `prbs_state` here
instead of the product's `state_at`: the expected value then starts from the oracle, and the product's host algebra --
the same GF2Powers that builds every table the device seeding reads -- is one more thing under test, not the referee.
"""
import functools
import random

from oracle import gf2poly, jump

# The matrix that is not shipped: candidate 3 of seed 293 of the search's candidate sequence for k = 64.  It is the first
# candidate of that seed that gf2poly.is_full_period accepts; nonshipped64() searches from candidate 0 and checks that.
NONSHIPPED64 = (293, 3)


def lutopt_state(u, m, N):
    """A^N u.init from the oracle `m` (an oracle.Lutopt of u's matrix); u.state_at(N) must equal it."""
    s = jump.lutopt_state(m, u.init, int(N))
    got = u.state_at(int(N))
    assert got == s, f"LUTOPT k={u.k}: state_at({N}) = {got:#x}, the oracle's jump gives {s:#x}"
    return s


def prbs_state(p, k, N):
    """The PRBS-k register N clocks after p.init from the oracle; p.state_at(N) must equal it."""
    assert p.k == k
    s = jump.prbs_state(k, p.init, int(N))
    got = p.state_at(int(N))
    assert got == s, f"PRBS{k}: state_at({N}) = {got:#x}, the oracle's jump gives {s:#x}"
    return s


def high_init(n):
    """A reset state with its high words set (tests/test_abi.py builds the same)."""
    return (0x0123456789ABCDEF << (n - 64 if n > 64 else 0) | 5) & ((1 << n) - 1)


@functools.lru_cache(maxsize=None)
def positions():
    """The far positions every host jump is held to the oracle at."""
    rng = random.Random(20260)
    p = [1 << i for i in range(64)]
    p += [s << 48 for s in range(1, 8)]
    p += [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    p += [2 ** 48 - 1, 10 ** 15, 10 ** 17, 2 ** 63 + 12345, 2 ** 64 - 1]
    p += [rng.getrandbits(64) for _ in range(32)]
    return tuple(p)


@functools.lru_cache(maxsize=None)
def nonshipped64(bound=16):
    """Tap lists of the k = 64 matrix NONSHIPPED64: the first candidate of its seed, searched from 0 over at most `bound`
    candidates, that the oracle's acceptance test takes."""
    from basebandboard_amd import gf2
    seed, want = NONSHIPPED64
    for cand in range(bound):
        rows = gf2.search_candidate(64, seed, cand)
        assert rows == gf2poly.search_candidate(64, seed, cand)
        if gf2poly.is_full_period(rows):
            assert cand == want, f"candidate {cand} of seed {seed} is accepted before {want}"
            return rows
    raise AssertionError(f"no full-period candidate of seed {seed} among the first {bound}")
