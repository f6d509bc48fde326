"""The two-kernel ("staged") form of the k = 256 sample stream (bbb_lutopt_set_staged): the sample kernel leaves its
pieces in a staging buffer as full lines, a second kernel moves them to their place on an internal stream, the next
fill's arithmetic overlaps that.  Same bytes as the one-kernel form and as the oracle, whatever is interleaved."""
import os

import numpy as np
import pytest
import torch

import far

pytestmark = pytest.mark.gpu

BIG = 1 << 24          # fills of at least this many samples take the staged form


def test_staged_fill_equals_oracle_and_one_kernel_form(gpu, oracle):
    m = oracle.Lutopt(path=oracle.data_path(256))
    u = gpu.LUTOPT.shipped(256)
    u.set_staged(True)
    g = gpu.CLTGRNG(u)
    d = gpu.CLTGRNG(gpu.LUTOPT.shipped(256))
    for n, first in ((BIG, 0), (BIG + 5, 16), (30_000_017, 12_345), (BIG - 16, 3)):       # the last one is below the threshold
        got = g.generate(n, first_step=first)
        snap = got.clone()                              # queued on the caller's stream right behind the fill
        exp = m.awgn(far.lutopt_state(u, m, first), 0, 300_000, fast=True)
        assert np.array_equal(snap[:300_000].cpu().numpy(), exp)
        tail = m.awgn(far.lutopt_state(u, m, first + n - 4096), 0, 4096, fast=True)
        assert np.array_equal(snap[-4096:].cpu().numpy(), tail)
        assert torch.equal(snap, d.generate(n, first_step=first))
        assert torch.equal(got, snap)


def test_back_to_back_staged_fills_with_prefetch(gpu, oracle):
    """The streaming pattern of bench.py: every fill announces the next one; the movers and the seedings run beside
    the following fill's arithmetic.  Four different buffers, all checked at the end."""
    m = oracle.Lutopt(path=oracle.data_path(256))
    u = gpu.LUTOPT.shipped(256, init=0x1234567)
    u.set_staged(True)
    g = gpu.CLTGRNG(u)
    n = BIG + 4096
    bufs = []
    for s in range(4):
        bufs.append(g.generate(n, first_step=16 + s * n))
        g.prefetch(n, first_step=16 + (s + 1) * n)
    torch.cuda.synchronize()
    ref = m.awgn(0x1234567, 16, 4 * n, fast=True)
    for s, b in enumerate(bufs):
        assert np.array_equal(b.cpu().numpy(), ref[s * n:(s + 1) * n])
    # the same buffer again and again (what the bench does): the mover of fill s must not overtake a reader of fill s-1
    buf = torch.empty(n, dtype=torch.int8, device="cuda")
    sums = []
    for s in range(4):
        g.generate(n, first_step=16 + s * n, out=buf)
        sums.append(buf.to(torch.int64).sum())          # a reader on the caller's stream between two fills
    assert [int(x) for x in sums] == [int(ref[s * n:(s + 1) * n].astype(np.int64).sum()) for s in range(4)]


def test_staged_fills_interleaved_with_other_calls(gpu, oracle):
    """Staged fills run on an internal stream, everything else on the caller's: the hand-over between them."""
    m = oracle.Lutopt(path=oracle.data_path(256))
    u = gpu.LUTOPT.shipped(256)
    u.set_staged(True)
    g = gpu.CLTGRNG(u)
    n = BIG + 48
    a = g.generate(n, first_step=16)
    t = gpu.Trial(nbits=400_003, amp=100, noise_var=8)
    assert gpu.run_trials(u, [t])[0] == m.ber_trial(1, 31, 1, 100, 8, 16, 0, 400_003)
    b = g.generate(n, first_step=16 + n)
    w = u.generate_words(1000, first_step=7)
    small = g.generate(5000, first_step=99)               # one-kernel form on the caller's stream
    c = g.generate(n, first_step=16 + 2 * n)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                          # the caller re-binds the handle to another stream
        dd = g.generate(n, first_step=16 + 3 * n)
        dsum = dd.to(torch.int64).sum()
    torch.cuda.synchronize()
    ref = m.awgn(1, 16, 4 * n, fast=True)
    for s, x in enumerate((a, b, c, dd)):
        assert np.array_equal(x.cpu().numpy(), ref[s * n:(s + 1) * n])
    assert int(dsum) == int(ref[3 * n:].astype(np.int64).sum())
    assert np.array_equal(small.cpu().numpy(), m.awgn(1, 99, 5000, fast=True))
    assert np.array_equal(w.cpu().numpy().view(np.uint32), m.words_u32(1, 7, 1000))


def test_staged_tx_equals_one_kernel_form(gpu, oracle, golden_shaper):
    n = BIG + 1000
    x = gpu.TX(31, 1, 0, 16, 1, 8)
    x.urng.set_staged(True)
    y = gpu.TX(31, 1, 0, 16, 1, 8)
    outs = [x.generate(n, first_sample=i * n) for i in range(3)]
    refs = [y.generate(n, first_sample=i * n) for i in range(3)]
    torch.cuda.synchronize()
    for a, b in zip(outs, refs):
        assert torch.equal(a, b)
    m = oracle.Lutopt(path=oracle.data_path(256))
    exp = oracle.tx(m, 1, golden_shaper["rcf_coeffs"][16], 31, 200_000, first_sample=n, noise_var=8, warmup=16)
    assert np.array_equal(outs[1][:200_000].cpu().numpy(), exp)


def _look_ahead_gen(gpu, init=1, fills=True):
    u = gpu.LUTOPT.shipped(256, init=init)
    u.set_staged(True, look_ahead=fills)
    return u, gpu.CLTGRNG(u)


@pytest.mark.parametrize("prefetch", [False, True])
@pytest.mark.parametrize("fills", [2, 3, 4])
def test_look_ahead_stream_equals_oracle(gpu, oracle, prefetch, fills):
    """Look-ahead: one sample kernel per `fills` sequential fills; the others are only piece movers.  Seven fills (the
    last sample kernel's output is not asked for in full), whole buffers against the oracle."""
    m = oracle.Lutopt(path=oracle.data_path(256))
    u, g = _look_ahead_gen(gpu, init=0xABCDE, fills=fills)
    n = BIG + 4096 + 16          # 16-sample aligned, segment boundaries do not fall on n
    bufs = []
    for s in range(7):
        bufs.append(g.generate(n, first_step=16 + s * n))
        if prefetch:
            g.prefetch(n, first_step=16 + (s + 1) * n)
    torch.cuda.synchronize()
    ref = m.awgn(0xABCDE, 16, 7 * n, fast=True)
    for s, b in enumerate(bufs):
        assert np.array_equal(b.cpu().numpy(), ref[s * n:(s + 1) * n]), s
    # one buffer reused, with a reader on the caller's stream between fills
    buf = torch.empty(n, dtype=torch.int8, device="cuda")
    sums = []
    for s in range(5):
        g.generate(n, first_step=16 + s * n, out=buf)
        if prefetch:
            g.prefetch(n, first_step=16 + (s + 1) * n)
        sums.append(buf.to(torch.int64).sum())
    assert [int(x) for x in sums] == [int(ref[s * n:(s + 1) * n].astype(np.int64).sum()) for s in range(5)]


@pytest.mark.parametrize("fills", [2, 4])
def test_look_ahead_broken_chains(gpu, oracle, fills):
    """The next fill is NOT the announced continuation: another position, another size, a size that is not a multiple
    of 16 (no look-ahead for it), a repeat of the same range, and wrong prefetch hints.  Every buffer exact."""
    m = oracle.Lutopt(path=oracle.data_path(256))
    u, g = _look_ahead_gen(gpu, fills=fills)
    d = gpu.CLTGRNG(gpu.LUTOPT.shipped(256))
    n = BIG + 160
    plan = [(n, 16), (n, 16 + n),                 # miss, hit
            (n, 16 + n),                          # the same range again: miss (that part was consumed)
            (n, 16 + 3 * n),                      # a skip: miss, discards the waiting half
            (n + 16, 16 + 4 * n),                 # continuation position but another size: miss
            (n + 5, 1000),                        # not a multiple of 16: plain staged fill
            (n + 5, 1000 + n + 5),
            (n, 7), (n, 7 + n), (n, 7 + 2 * n), (n, 7 + 3 * n)]        # a clean chain from an odd position
    outs = []
    for i, (cnt, first) in enumerate(plan):
        outs.append(g.generate(cnt, first_step=first))
        if i % 3 == 0:
            g.prefetch(cnt, first_step=first + cnt)           # right hint
        elif i % 3 == 1:
            g.prefetch(cnt, first_step=first + 12345)         # wrong hint
    torch.cuda.synchronize()
    for (cnt, first), got in zip(plan, outs):
        assert torch.equal(got, d.generate(cnt, first_step=first)), (cnt, first)
        assert np.array_equal(got[:100_000].cpu().numpy(), m.awgn(far.lutopt_state(u, m, first), 0, 100_000, fast=True))


def test_look_ahead_interleaved_with_other_calls(gpu, oracle, golden_shaper):
    """Between a fill and its continuation: a BER trial, raw words, a small fill, a TX fill on the same handle (it shares
    the staging slots), a level change.  The continuation is exact whether or not its half survived."""
    m = oracle.Lutopt(path=oracle.data_path(256))
    x = gpu.TX(31, 1, 0, 16, 1, 8)
    u = x.urng
    u.set_staged(True, look_ahead=True)
    g = gpu.CLTGRNG(u)
    n = BIG + 320
    ref = m.awgn(1, 16, 8 * n, fast=True)
    a0 = g.generate(n, first_step=16)
    t = gpu.Trial(nbits=300_001, amp=100, noise_var=8)
    assert gpu.run_trials(u, [t])[0] == m.ber_trial(1, 31, 1, 100, 8, 16, 0, 300_001)
    w = u.generate_words(500, first_step=3)
    small = g.generate(4096, first_step=5)
    a1 = g.generate(n, first_step=16 + n)                      # hit
    a2 = g.generate(n, first_step=16 + 2 * n)                  # miss, leaves a half
    tx1 = x.generate(BIG + 64, first_sample=0)                 # staged TX takes the other slot
    tx2 = x.generate(BIG + 64, first_sample=BIG + 64)          # ... and then the slot of the waiting half
    a3 = g.generate(n, first_step=16 + 3 * n)                  # must notice its half is gone
    a4 = g.generate(n, first_step=16 + 4 * n)
    u.set_staged(True)                                         # level 1: drops whatever waits
    a5 = g.generate(n, first_step=16 + 5 * n)
    u.set_staged(True, look_ahead=True)
    a6 = g.generate(n, first_step=16 + 6 * n)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                              # the continuation on another caller stream
        a7 = g.generate(n, first_step=16 + 7 * n)
        s7 = a7.to(torch.int64).sum()
    torch.cuda.synchronize()
    for s, b in enumerate((a0, a1, a2, a3, a4, a5, a6, a7)):
        assert np.array_equal(b.cpu().numpy(), ref[s * n:(s + 1) * n]), s
    assert int(s7) == int(ref[7 * n:].astype(np.int64).sum())
    assert np.array_equal(small.cpu().numpy(), m.awgn(1, 5, 4096, fast=True))
    assert np.array_equal(w.cpu().numpy().view(np.uint32), m.words_u32(1, 3, 500))
    y = gpu.TX(31, 1, 0, 16, 1, 8)
    assert torch.equal(tx1, y.generate(BIG + 64, first_sample=0))
    assert torch.equal(tx2, y.generate(BIG + 64, first_sample=BIG + 64))


def test_look_ahead_level_is_checked(gpu):
    u = gpu.LUTOPT.shipped(256)
    for bad in (9, 100):
        with pytest.raises(ValueError):
            u.set_staged(True, look_ahead=bad)


@pytest.mark.parametrize("fills,launches", [(2, 3), (3, 2), (4, 2)])
def test_look_ahead_costs_one_sample_kernel_per_m_fills(gpu, fills, launches):
    u, g = _look_ahead_gen(gpu, fills=fills)
    n = 1 << 26
    buf = torch.empty(n, dtype=torch.int8, device="cuda")
    g.generate(n, first_step=0, out=buf)
    u.set_staged(True, look_ahead=fills)           # drop what waits: the counted fills start on a miss
    u.profile(True)
    u.profile_read(reset=True)
    for s in range(6):
        g.generate(n, first_step=(1 + s) * n, out=buf)
    torch.cuda.synchronize()
    _, _, calls = u.profile_read(reset=True)
    u.profile(False)
    assert calls == launches


@pytest.mark.parametrize("fills", [2, 3])
def test_tx_look_ahead_equals_one_kernel_form(gpu, oracle, golden_shaper, fills):
    """bbb_tx_fill_i16 on a look-ahead handle: one TX sample kernel per `fills` consecutive calls of one configuration;
    a changed configuration, position or size falls back to its own kernel.  Against the one-kernel form, and a stretch
    of a later call against the oracle."""
    n = BIG + 4096
    x = gpu.TX(31, 1, 0, 16, 1, 8)
    x.urng.set_staged(True, look_ahead=fills)
    y = gpu.TX(31, 1, 0, 16, 1, 8)
    pos = [i * n for i in range(5)]
    outs = [x.generate(n, first_sample=p) for p in pos]
    x.noise_var = 3                                            # the waiting samples were made with 8: must not be used
    outs.append(x.generate(n, first_sample=5 * n))
    outs.append(x.generate(n, first_sample=6 * n))
    outs.append(x.generate(n + 16, first_sample=7 * n))        # another size
    outs.append(x.generate(n, first_sample=100))               # another position
    outs.append(x.generate(n, first_sample=100 + n, stream_on=False))
    u = x.urng
    a = gpu.CLTGRNG(u).generate(n, first_step=16)              # the noise stream on the same handle in between
    outs.append(x.generate(n, first_sample=100 + 2 * n))
    torch.cuda.synchronize()
    refs = [y.generate(n, first_sample=p) for p in pos]
    y.noise_var = 3
    refs += [y.generate(n, first_sample=5 * n), y.generate(n, first_sample=6 * n), y.generate(n + 16, first_sample=7 * n),
             y.generate(n, first_sample=100), y.generate(n, first_sample=100 + n), y.generate(n, first_sample=100 + 2 * n)]
    torch.cuda.synchronize()
    for i, (g_, r_) in enumerate(zip(outs, refs)):
        assert torch.equal(g_, r_), i
    m = oracle.Lutopt(path=oracle.data_path(256))
    exp = oracle.tx(m, 1, golden_shaper["rcf_coeffs"][16], 31, 100_000, first_sample=3 * n, noise_var=8, warmup=16)
    assert np.array_equal(outs[3][:100_000].cpu().numpy(), exp)
    assert np.array_equal(a[:100_000].cpu().numpy(), m.awgn(1, 16, 100_000, fast=True))


def test_look_ahead_at_the_bench_size(gpu):
    """BASELINE configs[1] as bench.py runs it: 1e9 samples per step, look-ahead 2, prefetch hints, one output buffer.
    Every step's whole buffer against the one-kernel form (which tests/test_gpu_awgn.py holds to the oracle byte for
    byte at this size)."""
    n = 1_000_000_000
    u, g = _look_ahead_gen(gpu, fills=2)
    d = gpu.CLTGRNG(gpu.LUTOPT.shipped(256))
    buf = torch.empty(n, dtype=torch.int8, device="cuda")
    ref = torch.empty(n, dtype=torch.int8, device="cuda")
    first = lambda s: 16 + s * n
    for s in range(5):
        g.generate(n, first_step=first(s), out=buf)
        g.prefetch(n, first_step=first(s + 1))
        d.generate(n, first_step=first(s), out=ref)
        assert torch.equal(buf, ref), s
    # per-rank stretches of bench.py: a position 2^48 steps in
    far_step = (3 << 48) + 16
    g.generate(n, first_step=far_step, out=buf)
    d.generate(n, first_step=far_step, out=ref)
    assert torch.equal(buf, ref)


# (BBB_SOAK_SEEDS=N: seeds 1..N instead of the three of a normal run -- after a change of the scheduler, once, on the GPU;
# BBB_SOAK_FIRST=F: seeds F..F+N-1, for a soak split over several calls)
@pytest.mark.parametrize("seed", list(range(int(os.environ.get("BBB_SOAK_FIRST", "1")),
                                            int(os.environ.get("BBB_SOAK_FIRST", "1")) + int(os.environ.get("BBB_SOAK_SEEDS", "3")))))
def test_random_mix_of_calls_on_one_staged_handle(gpu, oracle, seed):
    """Soak: a random sequence of noise fills (sequential and not, hinted and not, two output buffers and two caller
    streams), TX fills, BER trials and level changes on ONE handle; every output equals what a fresh handle in the
    one-kernel form produces.  Aimed at the stream / event plumbing between the arithmetic streams, the movers on the caller's streams, the
    seeding stream and the caller's."""
    rng = np.random.default_rng(seed)
    m = oracle.Lutopt(path=oracle.data_path(256))
    x = gpu.TX(31, 1, 0, 16, 1, 8)
    u = x.urng
    g = gpu.CLTGRNG(u)
    y = gpu.TX(31, 1, 0, 16, 1, 8)
    d = gpu.CLTGRNG(y.urng)
    side = torch.cuda.Stream()
    bufs = [torch.empty(BIG + 8192, dtype=torch.int8, device="cuda") for _ in range(2)]
    # The library orders ITS OWN work when the caller moves to another stream (include/bbb.h, bbb_lutopt_set_stream); the caller's own
    # reads of a buffer are the caller's to order, as with any stream-ordered library: a fill into bufs[b] first waits for the copy that
    # last read bufs[b] -- on whichever stream that was.  (Round 5's 300-seed soak failed on seed 202 without this: the snapshot of a
    # fill on the main stream, queued behind two transmitter calls, held the samples of the fill after next, made on the idle side
    # stream into the same buffer: profiles/r05_fail_soak_seed.log.)
    buf_read = [None, None]
    pos, checks = 16, []
    u.set_staged(True, look_ahead=2)
    for it in range(120):
        op = rng.integers(0, 10)
        n = BIG + 16 * int(rng.integers(0, 512))
        if op < 5:                                          # the next stretch of the stream, usually hinted
            out = bufs[it & 1][:n]
            st = side if rng.integers(0, 4) == 0 else torch.cuda.current_stream()
            with torch.cuda.stream(st):
                if buf_read[it & 1] is not None:
                    st.wait_event(buf_read[it & 1])
                g.generate(n, first_step=pos, out=out)
                snap = out.clone()
                buf_read[it & 1] = torch.cuda.Event()
                buf_read[it & 1].record(st)
            if rng.integers(0, 3):
                g.prefetch(n, first_step=pos + n)
            checks.append(("awgn", n, pos, snap))
            pos += n
        elif op == 5:                                       # somewhere else, odd size
            n2 = n + int(rng.integers(1, 16))
            p2 = int(rng.integers(0, 1 << 40))
            checks.append(("awgn", n2, p2, g.generate(n2, first_step=p2)))
        elif op == 6:
            checks.append(("tx", n, pos, x.generate(n, first_sample=pos)))
        elif op == 7:
            t = gpu.Trial(nbits=200_000 + it, amp=90, noise_var=8, first_bit=it)
            if rng.integers(0, 2):
                got = gpu.run_trials(u, [t])[0]
                assert got == m.ber_trial(1, 31, 1, 90, 8, 16, it, 200_000 + it)
            else:                                           # two trials queued back to back, nothing synchronises (checked at the end)
                t2 = gpu.Trial(nbits=150_000 + it, amp=70, noise_var=8, first_bit=3 * it + 1, prbs_k=23)
                c = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
                gpu.run_trials_into(u, [t], c[0:1])
                gpu.run_trials_into(u, [t2], c[1:2])
                checks.append(("ber", (t, t2), 0, c))
        elif op == 8:
            u.set_staged(True, look_ahead=int(rng.integers(1, 4)) if rng.integers(0, 2) else False)
        else:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    for kind, n, p, got in checks:
        if kind == "ber":
            exp = [m.ber_trial(1, t.prbs_k, 1, t.amp, t.noise_var, t.warmup, t.first_bit, t.nbits) for t in n]
            assert [tuple(r) for r in got.cpu().tolist()] == exp
            continue
        ref = d.generate(n, first_step=p) if kind == "awgn" else y.generate(n, first_sample=p)
        assert torch.equal(got, ref), (kind, n, p)


@pytest.mark.parametrize("bit_en,src,nv,first,shape", [(1, 0, 8, 0, 16), (1, 0, 15, 5, 16), (0, 0, 3, 1001, 16), (1, 1, 1, 17, 16), (1, 0, 0, 12345, 16),
                                                       (1, 1, 8, 2047, 16), (1, 0, 8, (1 << 31) + 3, 16),
                                                       # the shaping mover's two instances (round 5): without the 12-bit wrap where the host can rule it out
                                                       # (max over the phases of sum |coeffs| + 128 noise_var <= 2047), with it otherwise.  Coefficient set 0
                                                       # has the largest sum the reference ships (538): noise_var 11 is the last without, 12 the first with;
                                                       # set 31 the smallest (266): 13 / 14
                                                       (1, 0, 11, 3, 0), (1, 0, 12, 3, 0), (1, 0, 13, 6, 31), (1, 0, 14, 6, 31), (0, 0, 15, 9, 0), (0, 0, 15, 9, 31)])
def test_staged_tx_configurations(gpu, bit_en, src, nv, first, shape):
    """The noise kernel + shaping mover form of bbb_tx_fill_i16 over the transmitter's switches (bits off, pulse source,
    every phase c0 = (first - 17) & 7 through the start positions, noise_var 0 .. 15, a ragged length) against the
    one-kernel form, which tests/test_gpu_tx.py holds to the oracle."""
    n = BIG + 16 * 37 + 5
    x = gpu.TX(31, bit_en, src, shape, 1, nv)
    x.urng.set_staged(True)
    y = gpu.TX(31, bit_en, src, shape, 1, nv)
    for i in range(2):
        a = x.generate(n, first_sample=first + i * n)
        b = y.generate(n, first_sample=first + i * n)
        assert torch.equal(a, b), i


def test_prefetch_survives_unrelated_fills_on_its_slot(gpu, oracle):
    """A prefetch stays valid across fills that do not match it (bbb.h).  Its seeding waited for the mover that read the
    staging slot at the time; the unrelated fills in between put NEW movers on both slots, so the announced fill must
    wait for those again before its sample kernel overwrites the slot (round-2 advisor finding: a stale skip let it
    overwrite a buffer the newer mover was still reading)."""
    m = oracle.Lutopt(path=oracle.data_path(256))
    u = gpu.LUTOPT.shipped(256, init=0x5EED)
    u.set_staged(True)
    g = gpu.CLTGRNG(u)
    n = BIG + 4096
    big = 8 * BIG                      # long movers: still running when the announced fill's kernel is queued
    a = g.generate(n, first_step=16)
    g.prefetch(n, first_step=16 + n)                   # P: announced, its seeding waits for the mover of `a`'s slot partner
    x = g.generate(big, first_step=10_000_000_019)     # unrelated: slot 0 / 1 get new movers
    y = g.generate(big, first_step=20_000_000_033)
    b = g.generate(n, first_step=16 + n)               # the announced fill, straight behind them
    torch.cuda.synchronize()
    ref = m.awgn(0x5EED, 16, 2 * n, fast=True)
    assert np.array_equal(a.cpu().numpy(), ref[:n])
    assert np.array_equal(b.cpu().numpy(), ref[n:])
    for buf, first in ((x, 10_000_000_019), (y, 20_000_000_033)):
        got = buf.cpu().numpy()
        for off in (0, big // 2 - 77, big - 300_000):
            assert np.array_equal(got[off:off + 300_000], m.awgn(far.lutopt_state(u, m, first + off), 0, 300_000, fast=True)), (first, off)


def test_an_untaken_hint_does_not_race_the_next_one(gpu, oracle):
    """A hint whose fill comes with another partition is never taken: its seeding stays queued on the arithmetic stream of the
    fill it expected.  The next hint seeds the same buffers from the OTHER arithmetic stream and must queue behind it (round
    3: seeding moved from one side stream to the two arithmetic streams; the soak's seed 3 found the two writing side by
    side).  Several rounds of: hinted fill with a size of another partition, hint, fill that takes it."""
    m = oracle.Lutopt(path=oracle.data_path(256))
    u = gpu.LUTOPT.shipped(256, init=0xBEEF)
    u.set_staged(True)
    g = gpu.CLTGRNG(u)
    pos, outs = 16, []
    for r in range(6):
        n1 = BIG + 16 * (100 + r)
        n2 = BIG + 16 * (400 + 7 * r)            # another number of generators: the hint for (n1, pos) does not match it
        g.prefetch(n1, first_step=pos)
        outs.append((pos, g.generate(n2, first_step=pos)))
        pos += n2
        g.prefetch(n2, first_step=pos)             # seeds the same buffers as the untaken hint, from the other stream
        outs.append((pos, g.generate(n2, first_step=pos)))
        pos += n2
    torch.cuda.synchronize()
    for p, x in outs:
        assert np.array_equal(x[:200_000].cpu().numpy(), m.awgn(far.lutopt_state(u, m, p), 0, 200_000, fast=True)), p
        tail = m.awgn(far.lutopt_state(u, m, p + x.numel() - 4096), 0, 4096, fast=True)
        assert np.array_equal(x[-4096:].cpu().numpy(), tail), p


# The movers' STRAIGHT-LINE DMA path (stage_common.hpp, stage_dma_unit: a unit whose 128 steps all exist).  The shapes above, near
# 2^24, give L = 64: every unit is a segment's short last one.  With 256 CUs (1024 source waves at most) 300 000 032 samples give
# L = 144 -- per lane group one full unit and one short one of 16 steps -- and G = 2 083 334 generators, whose last wave holds 518.
N144 = 300_000_032


@pytest.fixture(scope="module")
def one_kernel_144(gpu):
    """the one-kernel form of the N144 samples from step 16, on a handle of its own: computed once, never written"""
    return gpu.CLTGRNG(gpu.LUTOPT.shipped(256)).generate(N144, first_step=16)


def test_full_unit_byte_fill_equals_oracle_and_one_kernel_form(gpu, oracle, one_kernel_144):
    m = oracle.Lutopt(path=oracle.data_path(256))
    u = gpu.LUTOPT.shipped(256)
    u.set_staged(True)
    got = gpu.CLTGRNG(u).generate(N144, first_step=16)
    assert torch.equal(got, one_kernel_144)
    assert np.array_equal(got[:4096].cpu().numpy(), m.awgn(far.lutopt_state(u, m, 16), 0, 4096, fast=True))
    assert np.array_equal(got[-4096:].cpu().numpy(), m.awgn(far.lutopt_state(u, m, 16 + N144 - 4096), 0, 4096, fast=True))


def test_full_unit_look_ahead_window_starts_inside_a_segment(gpu, one_kernel_144):
    """the same stream as two fills of one sample kernel: the second is a delivery whose window starts inside a segment"""
    u, g = _look_ahead_gen(gpu, fills=2)
    half = N144 // 2
    assert half % 16 == 0 and half % 144 != 0
    a = g.generate(half, first_step=16)
    b = g.generate(half, first_step=16 + half)
    assert torch.equal(a, one_kernel_144[:half])
    assert torch.equal(b, one_kernel_144[half:])


def test_full_unit_staged_tx_equals_one_kernel_form(gpu):
    """the shaping mover: one call of 300 000 021 samples (a ragged end), and two look-ahead calls of 150 000 016"""
    y = gpu.TX(31, 1, 0, 16, 1, 8)
    x = gpu.TX(31, 1, 0, 16, 1, 8)
    x.urng.set_staged(True)
    n = 300_000_021
    ref = y.generate(N144, first_sample=0)
    assert torch.equal(x.generate(n, first_sample=0), ref[:n])
    x.urng.set_staged(True, look_ahead=2)
    half = N144 // 2
    a = x.generate(half, first_sample=0)
    b = x.generate(half, first_sample=half)
    assert torch.equal(a, ref[:half])
    assert torch.equal(b, ref[half:])
