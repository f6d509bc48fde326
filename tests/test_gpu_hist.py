"""bbb_awgn_hist / CLTGRNG.histogram vs the oracle (through the C ABI): the histogram of the delivered samples of a range
of the stream, counted on the GPU without the samples reaching the caller.  All exact, no tolerances.

On the shipped n256 matrix pieces of 2^24 samples and more are counted by the histogram mover, a guest kernel that reads
the sample kernel's staging slot (segment lengths 64: every unit short; 144, 480: full and short units; 512: full units
only); everything else goes through the generator's fill and a plain histogram kernel."""
import numpy as np
import pytest
import torch

import far

pytestmark = pytest.mark.gpu

# the ragged list of the stream tests
SIZES = (1, 15, 16, 17, 63, 64, 65, 4099, 1_000_003, (1 << 24) + 16)
FIRSTS = (0, 7, 16, 2_345_678)
INITS = {16: (1, 0xBEEF), 32: (1, 0xBEEF), 64: (1, 0xBEEF), 128: (1, 0xBEEF), 256: (1, 0x1234567)}


def counts(x, k):
    """np.bincount(x + k/2, minlength=k) of int8 / int16 samples, in slices (bincount works on intp copies)"""
    out = np.zeros(k, dtype=np.int64)
    for off in range(0, len(x), 1 << 26):
        out += np.bincount(x[off:off + (1 << 26)].astype(np.int64) + k // 2, minlength=k)
    return out


def hist_of(g, n, first=0, out=None):
    h = g.histogram(n, first_step=first, out=out)
    assert h.dtype in (torch.uint64, torch.int64) and h.shape == (g.n,)
    return h.cpu().numpy().view(np.uint64).astype(np.int64)


def oracle_stream(oracle, k, init, first, n):
    m = oracle.Lutopt(path=oracle.data_path(k))
    return m.awgn(init, first, n, fast=(k == 256))


@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("k", (16, 32, 64, 128, 256))
def test_histogram_equals_bincount_of_the_oracle_stream(gpu, oracle, k, first):
    """Every ragged size, two reset states.  The oracle's stream is generated once per (k, init, first) at the largest
    size; the smaller sizes are its prefixes."""
    for init in INITS[k]:
        g = gpu.CLTGRNG(gpu.LUTOPT.shipped(k, init=init))
        x = oracle_stream(oracle, k, init, first, SIZES[-1])
        assert x.min() >= -(k // 2) and x.max() < k // 2
        for n in SIZES:
            got = hist_of(g, n, first)
            assert got.sum() == n, (k, init, first, n)
            assert np.array_equal(got, counts(x[:n], k)), (k, init, first, n)


def test_zero_samples_is_a_no_op_and_arguments_are_checked(gpu):
    import ctypes as C
    from basebandboard_amd import _lib
    u = gpu.LUTOPT.shipped(256)
    g = gpu.CLTGRNG(u)
    out = torch.arange(256, dtype=torch.int64, device="cuda")
    assert torch.equal(g.histogram(0, out=out).cpu(), torch.arange(256, dtype=torch.int64))
    l = _lib.lib()
    assert l.bbb_awgn_hist(u._h, None, 10, 0) == _lib.BBB_EINVAL
    assert l.bbb_awgn_hist(u._h, C.c_void_p(out.data_ptr() + 4), 10, 0) == _lib.BBB_EINVAL
    assert l.bbb_awgn_hist(u._h, C.c_void_p(out.data_ptr()), 10, 2 ** 64 - 5) == _lib.BBB_EINVAL
    with pytest.raises(ValueError):
        g.histogram(10, out=torch.zeros(128, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        g.histogram(10, out=torch.zeros(256, dtype=torch.int32, device="cuda"))
    v = gpu.LUTOPT.from_packed([[0]] * 24)          # k = 24: no CLTGRNG (rng.py:72-76)
    assert l.bbb_awgn_hist(v._h, C.c_void_p(out.data_ptr()), 10, 0) == _lib.BBB_EUNSUP


@pytest.mark.parametrize("nsamples,first", [(1, 0), (7, 3), (8, 0), (9, 16), (63, 1), (64, 0), (65, 5), (4099, 18),
                                            (1_000_003, 18), (3_000_000, 2_345_678)])
def test_n512_histogram_equals_the_oracle_tree(gpu, oracle, nsamples, first):
    """k = 512 (9-bit samples, 512 bins): the bincount of the oracle's clt_tree_bulk of its states, wrapped to 9 bits, as
    test_n512_generated_kernel_matches_oracle builds the stream."""
    m = oracle.Lutopt(path=oracle.data_path(512))
    for init in (1, int("0123456789abcdef" * 8, 16)):
        u = gpu.LUTOPT.shipped(512, init=init)
        got = hist_of(gpu.CLTGRNG(u), nsamples, first)
        exp = np.zeros(512, dtype=np.int64)
        for off in range(0, nsamples, 1 << 20):
            st = m.states(far.lutopt_state(u, m, first + off), 0, min(1 << 20, nsamples - off))
            v = ((m.clt_tree_bulk(st).astype(np.int64) + 256) % 512) - 256
            exp += np.bincount(v + 256, minlength=512)
        assert got.shape == (512,) and np.array_equal(got, exp)


def test_more_than_one_buffered_chunk(gpu, oracle):
    """A generator without the planes form beyond the internal buffer's 2^26 samples: two chunks, the second announced."""
    n = (1 << 26) + 4099
    g = gpu.CLTGRNG(gpu.LUTOPT.shipped(64, init=5))
    assert np.array_equal(hist_of(g, n, 12), counts(oracle_stream(oracle, 64, 5, 12, n), 64))


@pytest.mark.parametrize("n,first", [(1 << 24, 16), (300_000_007, 3), ((1 << 30) + (1 << 25) + 1_000_003, 2_345_678)])
def test_n256_mover_segment_lengths(gpu, oracle, n, first):
    """The histogram mover on segments of 64 steps (short units only), of 144 (a full and a short unit) and, in the third
    case, a range cut into a piece of 2^30 (512: full units), one of 2^25 + ... (64) -- against the oracle's whole stream."""
    g = gpu.CLTGRNG(gpu.LUTOPT.shipped(256, init=0x1234567))
    got = hist_of(g, n, first)
    assert np.array_equal(got, counts(oracle_stream(oracle, 256, 0x1234567, first, n), 256))


def test_n256_one_billion_samples_equal_the_oracle_stream(gpu, oracle):
    """The size of BASELINE.json configs[1]: 10^9 samples from 16 warm-up steps, every one of them against the oracle's
    single sequential pass (segments of 480 steps: three full units and a short one each)."""
    n = 1_000_000_000
    g = gpu.CLTGRNG(gpu.LUTOPT.shipped(256))
    got = hist_of(g, n, 16)
    exp = counts(oracle_stream(oracle, 256, 1, 16, n), 256)
    assert got.sum() == n and np.array_equal(got, exp)
    # twice in a row on the same handle (the second call's first chunk is not announced): the same counters again
    assert np.array_equal(hist_of(g, n, 16), exp)


def test_a_call_adds_and_a_range_may_be_cut_anywhere(gpu, oracle):
    first, n = 1000, 60_000_011
    x = oracle_stream(oracle, 256, 1, first, n)
    g = gpu.CLTGRNG(gpu.LUTOPT.shipped(256))
    whole = hist_of(g, n, first)
    assert np.array_equal(whole, counts(x, 256))
    start = torch.arange(1000, 1256, dtype=torch.int64, device="cuda").view(torch.uint64)
    out = start.clone()
    cuts = [0, 1, 4100, 17_000_003, 17_000_004, 40_000_001, n]         # pieces for the mover and pieces through memory
    for a, b in zip(cuts, cuts[1:]):
        r = g.histogram(b - a, first_step=first + a, out=out)
        assert r.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy().view(np.uint64).astype(np.int64), whole + np.arange(1000, 1256))
    # int64 counters are taken as well
    out64 = torch.zeros(256, dtype=torch.int64, device="cuda")
    g.histogram(4100, first_step=first, out=out64)
    assert np.array_equal(out64.cpu().numpy(), counts(x[:4100], 256))


def test_a_range_longer_than_one_internal_launch(gpu):
    """n = 2^31 + 12 345: two staged pieces of 2^30 and a ragged rest.  Held to the bincount of the LIBRARY'S OWN FILL over
    the same range (generate, whose bytes the stream tests hold to the oracle), not to the oracle: its sequential pass over
    2^31 samples would take minutes.  The fill goes through a fresh handle in pieces of 2^28."""
    n, first = (1 << 31) + 12_345, 16
    got = hist_of(gpu.CLTGRNG(gpu.LUTOPT.shipped(256)), n, first)
    assert got.sum() == n
    f = gpu.CLTGRNG(gpu.LUTOPT.shipped(256))
    exp = torch.zeros(256, dtype=torch.int64, device="cuda")
    buf = torch.empty(1 << 28, dtype=torch.int8, device="cuda")
    for off in range(0, n, 1 << 28):
        m = min(1 << 28, n - off)
        x = f.generate(m, first_step=first + off, out=buf)
        exp += torch.bincount(x.to(torch.int32) + 128, minlength=256)
    assert np.array_equal(got, exp.cpu().numpy())


def test_identical_in_every_mode_of_the_handle(gpu, oracle):
    n, first = (1 << 25) + 4099, 16
    exp = counts(oracle_stream(oracle, 256, 1, first, n), 256)
    for level in (0, 1, 4):
        u = gpu.LUTOPT.shipped(256)
        if level:
            u.set_staged(True, look_ahead=level if level > 1 else False)
        g = gpu.CLTGRNG(u)
        assert np.array_equal(hist_of(g, n, first), exp), level
        # ... and the mode is the caller's again: the fills of the mode still deliver the oracle's bytes
        got = g.generate(1 << 24, first_step=first).cpu().numpy()
        assert np.array_equal(got, oracle_stream(oracle, 256, 1, first, 1 << 24)), level
        assert np.array_equal(hist_of(g, n, first), exp), level
    # with an open stream object on another handle
    other = gpu.CLTGRNG(gpu.LUTOPT.shipped(256, init=77))
    with other.stream(1 << 24, first_step=0) as st:
        a = st.next().cpu().numpy()
        assert np.array_equal(hist_of(gpu.CLTGRNG(gpu.LUTOPT.shipped(256)), n, first), exp)
        b = st.next().cpu().numpy()
    assert np.array_equal(np.concatenate([a, b]), oracle_stream(oracle, 256, 77, 0, 1 << 25))
    # on a stream of the handle's own opened over it: reads and histograms in turn
    u = gpu.LUTOPT.shipped(256)
    g = gpu.CLTGRNG(u)
    with g.stream(1 << 24, first_step=first) as st:
        a = st.next().cpu().numpy()
        assert np.array_equal(hist_of(g, n, first), exp)
        b = st.next().cpu().numpy()
    assert np.array_equal(np.concatenate([a, b]), oracle_stream(oracle, 256, 1, first, 1 << 25))
    # on a non-default HIP stream (bbb_lutopt_set_stream binds the current torch stream)
    s = torch.cuda.Stream()
    g = gpu.CLTGRNG(gpu.LUTOPT.shipped(256))
    with torch.cuda.stream(s):
        h1 = g.histogram(n, first_step=first)
        h2 = g.histogram(4099, first_step=first)
    s.synchronize()
    assert np.array_equal(h1.cpu().numpy().view(np.uint64).astype(np.int64), exp)
    assert np.array_equal(h2.cpu().numpy().view(np.uint64).astype(np.int64), counts(oracle_stream(oracle, 256, 1, first, 4099), 256))


@pytest.mark.parametrize("level", (0, 1, 2))
def test_fills_and_histograms_interleaved_on_one_handle(gpu, oracle, level):
    """A small random mix of fills, announcements and histograms on one handle: every fill delivers the oracle's bytes and
    every histogram its counts."""
    rng = np.random.default_rng(20 + level)
    m = oracle.Lutopt(path=oracle.data_path(256))
    u = gpu.LUTOPT.shipped(256)
    if level:
        u.set_staged(True, look_ahead=level if level > 1 else False)
    g = gpu.CLTGRNG(u)
    sizes = (4099, 1 << 20, 1 << 24, (1 << 24) + 16, (1 << 25) + 48)
    pos = 16
    for step in range(14):
        n = int(sizes[rng.integers(len(sizes))])
        what = int(rng.integers(4))
        first = pos if rng.integers(3) else int(rng.integers(1 << 30))
        exp = m.awgn(far.lutopt_state(u, m, first), 0, n, fast=True)
        if what == 0:
            g.prefetch(n, first_step=first)
        if what <= 1:
            assert np.array_equal(g.generate(n, first_step=first).cpu().numpy(), exp), (step, n, first)
        else:
            if what == 3:
                g.prefetch(n, first_step=first)           # an announcement meant for a fill, met by a histogram
            assert np.array_equal(hist_of(g, n, first), counts(exp, 256)), (step, n, first)
        pos = first + n
    assert np.array_equal(g.generate(1 << 24, first_step=pos).cpu().numpy(), m.awgn(far.lutopt_state(u, m, pos), 0, 1 << 24, fast=True))


def test_table_driven_n256_handle(gpu, oracle):
    """The n256 matrix with one row changed has no generated kernel (is_specialised 0): the table-driven fill and the plain
    histogram kernel, against the oracle built from the same taps -- also at a size the shipped matrix gives to the mover."""
    packed = [list(r) for r in gpu.recurrences.n256]
    packed[5] = sorted(set(packed[5]) ^ {0, 1})
    u = gpu.LUTOPT.from_packed(packed, init=12345)
    assert not u.specialised
    m = oracle.Lutopt(packed=packed)
    g = gpu.CLTGRNG(u)
    for n, first in ((1_000_003, 3), ((1 << 24) + 16, 0)):
        assert np.array_equal(hist_of(g, n, first), counts(m.awgn(12345, first, n), 256)), n


def test_evaluate_equals_evaluate_samples_of_the_oracle_stream(gpu, oracle):
    from basebandboard_amd import grngstats
    n = 10 ** 7
    u = gpu.LUTOPT.shipped(256)
    a = grngstats.evaluate(u, n)
    b = grngstats.evaluate_samples(oracle_stream(oracle, 256, 1, 0, n), 256)
    assert a == b and a.nsamples == n and sum(a.hist) == n
    assert a.chi2.p_value >= 1e-4
    assert str(a).splitlines()[0] == "Theoretical mean μ=0.0000e+00, variance σ²=6.4000e+01."
    # through a CLTGRNG, from another position, in several calls that add into one set of counters
    c = grngstats.evaluate(gpu.CLTGRNG(u), n, first_step=16, chunk=3_000_001)
    assert c == grngstats.evaluate_samples(oracle_stream(oracle, 256, 1, 16, n), 256)


def test_smoke_line(gpu, oracle):
    """__graft_entry__.smoke()'s line: the histogram of the 1 000 003 samples it generates equals np.bincount of them."""
    u = gpu.LUTOPT.shipped(256)
    n = 1_000_003
    got = gpu.CLTGRNG(u).generate(n, first_step=16).cpu().numpy()
    h = gpu.CLTGRNG(u).histogram(n, first_step=16).cpu().numpy()
    assert np.array_equal(h.view(np.uint64), np.bincount(got.astype(np.int64) + 128, minlength=256).astype(np.uint64))
