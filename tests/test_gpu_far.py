"""Every device consumer of a stream position, at positions the sequential oracle cannot step to.  The expected streams
start from the state oracle/jump.py derives independently (x^N mod p, single oracle steps: tests/far.py) and run through
the sequential oracle; the product's own jump-ahead -- the GF2Powers that builds every table the device seeding reads --
is never the referee.  Bit exact."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import far
from oracle import jump

pytestmark = pytest.mark.gpu

NS = 70_001                     # samples of a far fill: more than one wave's generators, odd
NB = 300_000                    # bits of a far PRBS fill
U64 = 2 ** 64


def positions(n):
    """P for a call of n positions: one that straddles 2^32, one beyond 2^48, and the largest the entry points' argument check
    (first + n must not wrap: `first_step + nsamples < first_step` in awgn_fill, bbb_lutopt_fill_words and launch_stream)
    accepts -- the call's last position is then 2^64 - 1."""
    return (2 ** 32 - n // 2, (3 << 48) + 5, U64 - 1 - n)


def matrix(gpu, oracle, name, init=1):
    """(product handle, oracle Lutopt) of a shipped order or of the k = 64 matrix that is not shipped (table-driven kernel)."""
    if name == "other64":
        rows = far.nonshipped64()
        u = gpu.LUTOPT.from_packed(rows, init=init)
        assert not u.specialised
        return u, oracle.Lutopt(packed=rows)
    return gpu.LUTOPT.shipped(name, init=init), oracle.Lutopt(path=oracle.data_path(name))


def samples(m, state, count):
    """`count` CLTGRNG samples of oracle `m` behind `state` (the first is that of the NEXT state), as int64."""
    if m.k == 512:
        return ((m.clt_tree_bulk(m.states(state, 0, count)).astype(np.int64) + 256) % 512) - 256
    return m.awgn(state, 0, count, fast=m.k == 256).astype(np.int64)


# ---- fills --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", (16, 32, 64, 128, 256, 512, "other64"))
def test_fill_at_far_positions(gpu, oracle, name):
    u, m = matrix(gpu, oracle, name, init=far.high_init(64 if name == "other64" else name))
    g = gpu.CLTGRNG(u)
    for F in positions(NS):
        got = g.generate(NS, first_step=F).cpu().numpy().astype(np.int64)
        assert np.array_equal(got, samples(m, far.lutopt_state(u, m, F), NS)), F
    # one past the largest position: refused, nothing written
    out = torch.full((NS + 64,), 77, dtype=g.dtype, device="cuda")
    fn = gpu._lib.lib().bbb_awgn_fill_i8 if g.dtype == torch.int8 else gpu._lib.lib().bbb_awgn_fill_i16
    assert fn(u._h, C.c_void_p(out.data_ptr()), NS, U64 - NS) == gpu._lib.BBB_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 77).all())


def test_word_fill_at_far_positions(gpu, oracle):
    u, m = matrix(gpu, oracle, 256, init=far.high_init(256))
    for F in positions(NS):
        got = u.generate_words(NS, first_step=F).cpu().numpy().view(np.uint32)
        assert np.array_equal(got, m.words_u32(far.lutopt_state(u, m, F), 0, NS)), F
    out = torch.full((8 * NS,), 77, dtype=torch.int32, device="cuda")
    assert gpu._lib.lib().bbb_lutopt_fill_words(u._h, C.c_void_p(out.data_ptr()), NS, U64 - NS, 0) == gpu._lib.BBB_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 77).all())


# ---- the device jump tables ---------------------------------------------------------------------

BIG = 1 << 27
FIRST = (5 << 48) + 16


PAIRS = [(e, j) for e in (1, 2, 3) for j in range(1, 16)]


def window_grid(tops=32, thin=1):
    """Generator numbers g = d 65536 + j 16^e + r whose start states are compared: r is random below 16^e, so radix-16 digit e
    of g is j and digits 4 and 5 are those of d.  thin = 1: every (e, j) for every d < tops.  thin > 1: every (e, j) pair
    still occurs -- pair number i keeps the d with d % thin == i % thin -- and so does every d."""
    rng = random.Random(5)
    return [d * 65536 + j * 16 ** e + rng.randrange(16 ** e) for i, (e, j) in enumerate(PAIRS) for d in range(tops) if d % thin == i % thin]


def check_windows(m, init, got, gs, seg=64):
    """Windows of 128 samples at offsets seg g -- generator g's first samples when segments are `seg` long, for seg = 64 also
    the next generator's -- then the last generator's segment and the last 5000 samples, each from one oracle jump."""
    n = got.numel()
    got = got.cpu().numpy()
    for off, cnt in [(seg * g, 128) for g in gs] + [(n - seg, seg), (n - 5000, 5000)]:
        assert 0 <= off < n
        cnt = min(cnt, n - off)
        exp = samples(m, jump.lutopt_state(m, init, FIRST + off), cnt)
        assert np.array_equal(got[off:off + cnt].astype(np.int64), exp), f"offset {off} = generator {off // seg} of segments of {seg}"


def digits_reached(gs):
    """{(e, digit)}: the non-zero radix-16 digits of the generator numbers, per level e >= 1."""
    return {(e, g >> (4 * e) & 15) for g in gs for e in range(1, 6)} - {(e, 0) for e in range(1, 6)}


def test_two_launch_seeding_reads_every_table(gpu, oracle):
    """One unannounced n256 fill of 2^27 samples at (5 << 48) + 16: the two-launch seeding (head kernel: the level tables
    j 16^e, e = 1 .. 3; tail kernel: the top tables d 65536, d = 1 .. 31).  On a part with 256 CUs the fill is cut into
    G = 2^21 generators of L = 64 samples, so window g starts at generator g's first sample; the 1440 windows are every
    (e, j) under every d, so every level table is read under every top table.  The assertions hold for any partition -- they
    compare samples at stream positions; only the placement of the windows on segment starts assumes 256 CUs."""
    u, m = matrix(gpu, oracle, 256)
    far.lutopt_state(u, m, FIRST)
    gs = window_grid()
    assert len(gs) == 1440 and max(gs) < BIG // 64
    assert digits_reached(g & 0xffff for g in gs) == {(e, j) for e, j in PAIRS} and {g >> 16 for g in gs} == set(range(32))
    got = gpu.CLTGRNG(u).generate(BIG, first_step=FIRST)
    check_windows(m, 1, got, gs)


@pytest.mark.parametrize("name,seg,thin", [(512, 128, 3), (128, 64, 5), ("announced256", 64, 5)])
def test_level_chain_seeding_reads_every_table(gpu, oracle, name, seg, thin):
    """The same fill on the seedings that walk the level chain (awgn_seed_launch, tables j 16^e for every radix-16 digit of the
    generator number): n512, n128, and n256 when the fill was announced with prefetch(n, first).  On a part with 256 CUs
    n128 and n256 are cut into G = 2^21 generators of 64 samples and n512 (partition512) into G = 2^20 of 128, which is
    where the windows are put: a thinned grid of 288 (n512: 240) windows in which every digit j = 1 .. 15 of every level
    e = 1 .. 4 occurs, and digit 1 of level 5 where G = 2^21 has one (n512 has no level 5); asserted below.  Levels above
    are not reached by a fill of this size.  As above, only the placement of the windows assumes 256 CUs."""
    u, m = matrix(gpu, oracle, 256 if name == "announced256" else name)
    far.lutopt_state(u, m, FIRST)
    gs = window_grid(BIG // seg // 65536, thin)
    assert max(gs) < BIG // seg
    assert digits_reached(gs) == {(e, j) for e in (1, 2, 3, 4) for j in range(1, 16)} | ({(5, 1)} if seg == 64 else set())
    g = gpu.CLTGRNG(u)
    if name == "announced256":
        g.prefetch(BIG, first_step=FIRST)
    got = g.generate(BIG, first_step=FIRST)
    check_windows(m, 1, got, gs, seg)


# ---- PRBS ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (7, 9, 11, 15, 20, 23, 31))
def test_prbs_fill_and_check_at_far_positions(gpu, oracle, k):
    p = gpu.PRBS(k)
    det = gpu.PRBSErrorDetector(k)
    for F in positions(NB) + ((5 << 48) + 12345,):
        buf = p.generate(NB, first_bit=F)
        exp, s_end = oracle.prbs_packed(k, NB, state=far.prbs_state(p, k, F), fast=True)
        assert np.array_equal(buf.cpu().numpy().view(np.uint64), exp), F
        assert far.prbs_state(p, k, F + NB) == s_end                        # the state behind the last bit
        assert det.count_errors(buf, NB, first_bit=F) == 0
        buf[NB // 128] ^= 1 << 33
        assert det.count_errors(buf, NB, first_bit=F) == 1
    # one past the largest position: refused by the fill and by the checker, nothing written
    l = gpu._lib.lib()
    out = torch.full((NB // 64 + 8,), 77, dtype=torch.int64, device="cuda")
    assert l.bbb_prbs_fill(k, 1, U64 - NB, NB, C.c_void_p(out.data_ptr()), 0, None) == gpu._lib.BBB_EINVAL
    nerr = C.c_uint64(99)
    assert l.bbb_prbs_check(k, 1, U64 - NB, NB, C.c_void_p(out.data_ptr()), C.byref(nerr), 0, None) == gpu._lib.BBB_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and nerr.value == 99


# ---- BER ----------------------------------------------------------------------------------------

AMPS = (91, 114, 143, 181)


@pytest.fixture(scope="module")
def sweep88(gpu):
    """BASELINE configs[4] in small, with all of its eight seeds: stretches of the one cycle 2^48 apart, four points each,
    as one grouped sweep -- and the same trials through bbb_ber_trials."""
    from basebandboard_amd.channel import sweep_multi
    u = gpu.LUTOPT.shipped(256)
    ts = [gpu.Trial(nbits=300_011, amp=a, noise_var=8, warmup=16 + (s << 48)) for s in range(8) for a in AMPS]
    got = sweep_multi([u], ts, mode=gpu._lib.SHARD_GROUPS)
    assert got == gpu.run_trials(u, ts)
    return u, got


@pytest.mark.parametrize("s", range(8))
def test_every_seed_of_the_grouped_sweep(gpu, oracle, sweep88, s):
    """Seed s starts at stream position 16 + s 2^48: the literal trial of the oracle from the oracle's own state there."""
    u, got = sweep88
    m = oracle.Lutopt(path=oracle.data_path(256))
    x = far.lutopt_state(u, m, 16 + (s << 48))
    assert got[4 * s:4 * s + 4] == [m.ber_trial(x, 31, 1, a, 8, 0, 0, 300_011) for a in AMPS]


def test_trial_at_a_far_first_bit(gpu, oracle):
    u, m = matrix(gpu, oracle, 256, init=far.high_init(256))
    first = (1 << 40) + 3
    for k in (31, 9):
        t = gpu.Trial(nbits=300_011, amp=114, noise_var=8, prbs_k=k, prbs_state=5, warmup=16, first_bit=first)
        ps = far.prbs_state(gpu.PRBS(k, init=5), k, first)
        x = far.lutopt_state(u, m, 16 + first)
        assert gpu.run_trials(u, [t]) == [m.ber_trial(x, k, ps, 114, 8, 0, 0, 300_011)]


# ---- noise stream and histogram -----------------------------------------------------------------

def test_noise_stream_seek_to_a_far_position(gpu, oracle):
    u, m = matrix(gpu, oracle, 256, init=0xC0FFEE)
    n = (1 << 24) + 4096 + 16
    pos = (2 << 48) + 9
    with gpu.CLTGRNG(u).stream(n, first_step=16) as st:
        st.seek(pos)
        parts = [st.next() for _ in range(3)]
        assert st.tell() == pos + 3 * n
        torch.cuda.synchronize()
    for i, p in enumerate(parts):
        assert np.array_equal(p[:200_000].cpu().numpy(), samples(m, far.lutopt_state(u, m, pos + i * n), 200_000)), i
        assert np.array_equal(p[-4096:].cpu().numpy(), samples(m, far.lutopt_state(u, m, pos + (i + 1) * n - 4096), 4096)), i


def test_histogram_at_a_far_position(gpu, oracle):
    u, m = matrix(gpu, oracle, 256)
    first = (3 << 48) + 5
    got = gpu.CLTGRNG(u).histogram(1 << 20, first_step=first).cpu().numpy().view(np.uint64)
    exp = np.bincount(samples(m, far.lutopt_state(u, m, first), 1 << 20) + 128, minlength=256)
    assert np.array_equal(got, exp)
