"""bbb_conv_encode and bbb_conv_decode on the GPU, bit for bit against tests/conv_model.py: every constraint length, two and
three coded bits, punctured periods, small and default windows, records around the block sizes, soft and hard values, calls
that start inside a block with more and less history than wanted, calls that are not final, a stream cut at random points,
the tie rules, the metrics' bound, termination, more than two passes of the decoder's grid, and the closed loop of tests/test_conv_host.py.

Out of reach at a test's cost: more than one pass of the encoder's grid, which is capped at 2^20 workgroups of one output word a
thread (2^34 transmitted bits a pass)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fir_model
import grid
import conv_model as M
import test_conv_host as H

pytestmark = pytest.mark.gpu

GUARD = -0x0123456789ABCDEF
GEOMS = ((5, 2, 3), (64, 0, 0), (0, 0, 0), (256, 128, 128))
G171 = (0o171, 0o133)


def _cfg(code, B=0, W=0, D=0):
    from basebandboard_amd import _lib
    c = _lib.ConvCfg()
    c.K, c.n, c.init_state, c.period, c.terminated = code.K, code.n, code.init_state, code.period, int(code.terminated)
    for i in range(code.n):
        c.gen[i], c.keep[i] = code.gens[i], code.keep[i]
    c.block_steps, c.warmup_steps, c.lookahead_steps = B, W, D
    return c


def _random_code(rng, K, n, period, **kw):
    while True:
        keep = rng.integers(0, 1 << period, n).tolist()
        if all(any(k >> r & 1 for k in keep) for r in range(period)):
            break
    return M.Code(K, rng.integers(1, 1 << K, n).tolist(), period, keep, int(rng.integers(0, 1 << (K - 1))), **kw)


def _noisy(rng, code, nsteps, first=0, sigma=40):
    bits = rng.integers(0, 2, nsteps)
    tx, _ = M.encode(code, bits, first, int(rng.integers(0, code.ns)))
    return ((2 * tx.astype(np.int64) - 1) * 64 + np.rint(rng.normal(0, sigma, len(tx)))).astype(np.int16)


def _unpack(t, n):
    return np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[:n]


def _pack_at(bits, off):
    b = np.zeros((off + len(bits) + 63) // 64 * 64 + 64, dtype=np.uint8)
    b[off:off + len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.int64)


def _decode(gpu, code, vals, nb=0, first=0, final=True, B=0, W=0, D=0, hard=False, in_off=0, bits_off=0, unaligned=False):
    """One bbb_conv_decode through the C ABI: the values (bits 0 / 1 with hard) sit `in_off` elements or bits behind the buffer's
    base, the output `bits_off` words behind an aligned address between guard words.  Returns (bits uint8, stats dict)."""
    from basebandboard_amd import _lib
    dev = torch.device("cuda", 0)
    vals = np.asarray(vals)
    nin = len(vals) - nb
    _, nd, _ = M.plan(code, nin, first, final, B, W, D)
    nwords = (nd + 63) // 64
    if hard:
        buf = torch.from_numpy(_pack_at(vals, in_off)).to(dev)
        p_in = buf.data_ptr()
    else:
        buf = torch.full((in_off + len(vals) + 8,), 0x7ABC, dtype=torch.int16, device=dev)
        buf[in_off:in_off + len(vals)] = torch.from_numpy(vals.astype(np.int16)).to(dev)
        p_in = buf.data_ptr() + 2 * (in_off & 7)         # the base need not be aligned either
        in_off -= in_off & 7
    bits = torch.full((bits_off + nwords + 2,), GUARD, dtype=torch.int64, device=dev)
    stats = torch.tensor([1000, 2000], dtype=torch.int64, device=dev)
    got = C.c_uint64()
    p_bits = bits.data_ptr() + 8 * (bits_off + 1)
    if unaligned:
        assert p_bits % 16 and (hard or p_in % 16), (p_in % 16, p_bits % 16)
    _lib.check(_lib.lib().bbb_conv_decode(C.c_void_p(p_in), in_off + nb, nin, nb, first, int(final), int(hard), C.byref(_cfg(code, B, W, D)),
                                          C.c_void_p(p_bits), C.c_void_p(stats.data_ptr()), C.byref(got), 0,
                                          C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "bbb_conv_decode")
    assert got.value == nd, "ndecided is not bbb_conv_plan's"
    w = bits.cpu().numpy()
    assert (w[:bits_off + 1] == GUARD).all() and w[-1] == GUARD, "a word next to bits_packed_dev was written"
    got_bits = np.unpackbits(w[bits_off + 1:-1].view(np.uint8), bitorder="little")
    assert not got_bits[nd:].any(), "the unused bits of the last word are not 0"
    stv = (stats.cpu().numpy() - np.array([1000, 2000])).tolist()
    return got_bits[:nd], dict(zip(("windows", "steps"), stv))


def _check(gpu, code, vals, nb=0, first=0, final=True, B=0, W=0, D=0, hard=False, **off):
    bits, stats = _decode(gpu, code, vals, nb, first, final, B, W, D, hard, **off)
    want, windows = M.run(code, vals, nb, first, final, B, W, D, hard)
    bad = np.flatnonzero(bits != want)
    assert len(bits) == len(want) and len(bad) == 0, f"{len(bad)} bits differ, the first at step {bad[0]} of {len(want)}"
    assert stats == (dict(windows=windows, steps=len(want)) if len(want) else dict(windows=0, steps=0))
    return bits


def _encode(gpu, code, bits, first=0, state=None, off=0):
    """One bbb_conv_encode through the C ABI, the output between guard words.  (transmitted bits, count, state behind)."""
    from basebandboard_amd import _lib
    dev = torch.device("cuda", 0)
    nout = M.idx(code, first + len(bits)) - M.idx(code, first)
    src = torch.from_numpy(np.concatenate([np.zeros(off, dtype=np.int64), _pack_at(bits, 0)])).to(dev)
    out = torch.full((off + (nout + 63) // 64 + 2,), GUARD, dtype=torch.int64, device=dev)
    st = torch.tensor([7, state if state is not None else 0, 7], dtype=torch.int32, device=dev)
    got = C.c_uint64()
    _lib.check(_lib.lib().bbb_conv_encode(C.c_void_p(src.data_ptr() + 8 * off), len(bits), first, C.byref(_cfg(code)),
                                          C.c_void_p(st.data_ptr() + 4) if state is not None else None, C.c_void_p(out.data_ptr() + 8 * (off + 1)),
                                          C.byref(got), 0, C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "bbb_conv_encode")
    assert got.value == nout
    w = out.cpu().numpy()
    assert (w[:off + 1] == GUARD).all() and w[-1] == GUARD, "a word next to out_dev was written"
    tx = np.unpackbits(w[off + 1:-1].view(np.uint8), bitorder="little")
    assert not tx[nout:].any(), "the unused bits of the last word are not 0"
    s = st.cpu().tolist()
    assert s[0] == 7 and s[2] == 7
    return tx[:nout], nout, s[1]


# ---- the encoder -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", (3, 4, 5, 6, 7))
def test_encode_every_code_period_and_length(gpu, K):
    rng = np.random.default_rng(300 + K)
    for n in (2, 3):
        for period in (1, 2, 3, 7, 16):
            code = _random_code(rng, K, n, period)
            for nsteps in (1, 63, 64, 65, 4099):
                first = int(rng.choice([0, 1, period + 1, 5 * period + period // 2, (1 << 40) + 3]))
                bits = rng.integers(0, 2, nsteps)
                want, _ = M.encode(code, bits, first)
                got, nout, _ = _encode(gpu, code, bits, first, off=nsteps & 1)
                assert nout == len(want) and np.array_equal(got, want), (n, period, nsteps, first)
            # a record in pieces with the state word
            bits = rng.integers(0, 2, 1000)
            want, end = M.encode(code, bits)
            state, out = code.init_state, []
            for lo, hi in ((0, 1), (1, 3), (3, 3), (3, 130), (130, 1000)):
                got, _, state = _encode(gpu, code, bits[lo:hi], lo, state)
                out.append(got)
            assert np.array_equal(np.concatenate(out), want) and state == end


# ---- the decoder -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", (3, 4, 5, 6, 7))
def test_every_code_geometry_and_record_length(gpu, K):
    """n 2 and 3 under the four geometries (a tiny window, B = 64 with the default edges, the defaults, B + W + D = 512), records
    of 1, B - 1, B, B + 1, 1000 and 4099 steps of noisy encoded data, soft and hard, the periods 1, 3, 7, 16 in turn, every
    pointer off 16-byte alignment."""
    rng = np.random.default_rng(400 + K)
    turn = 0
    for n in (2, 3):
        for B, W, D in GEOMS:
            Bq = B or 192
            for nsteps in (1, Bq - 1, Bq, Bq + 1, 1000, 4099):
                code = _random_code(rng, K, n, (1, 3, 7, 16)[turn % 4])
                turn += 1
                rx = _noisy(rng, code, nsteps)
                _check(gpu, code, rx, B=B, W=W, D=D, in_off=1 + 2 * n, bits_off=2 * (n & 1), unaligned=True)
                _check(gpu, code, (rx >= 0).astype(np.int64), B=B, W=W, D=D, hard=True, in_off=int(rng.integers(1, 130)), bits_off=2 * (n & 1),
                       unaligned=True)


def test_first_step_anywhere_with_full_and_short_history(gpu):
    """A call that starts at step 1, at a block boundary, inside a block and at 2^40 + 3 decides from the block's absolute window:
    with the history the window reaches (and more), with less, where the rest counts as 0, and with none; final and not."""
    rng = np.random.default_rng(12)
    for K, n, period, (B, W, D) in ((7, 2, 3, (0, 0, 0)), (5, 3, 7, (5, 2, 3)), (3, 2, 16, (64, 0, 0)), (7, 3, 1, (5, 2, 3))):
        code = _random_code(rng, K, n, period)
        Bq = B or 192
        for first in (0, 1, Bq, Bq + 1, 3 * Bq - 1, 7 * Bq + Bq // 2, (1 << 40) + 3):
            wanted = M.nbefore_wanted(code, first, B, W, D)
            for nb in sorted({wanted + 13, wanted // 2, 0}):
                nb = min(nb, M.idx(code, first))
                for final in (True, False):
                    for hard in (False, True):
                        vals = np.concatenate([rng.integers(-90, 91, nb).astype(np.int16), _noisy(rng, code, 2 * Bq + 40, first)])
                        if hard:
                            vals = (vals >= 0).astype(np.int64)
                        _check(gpu, code, vals, nb, first, final, B, W, D, hard, in_off=1 + (nb & 7))


@pytest.mark.parametrize("K", (3, 4, 5, 6, 7))
def test_ties_on_all_zero_input(gpu, K):
    """Every ACS of every window ties: c = 0 survives, the lowest end state wins."""
    rng = np.random.default_rng(500 + K)
    for n, geom in ((2, (5, 2, 3)), (3, (0, 0, 0)), (2, (64, 0, 0))):
        code = _random_code(rng, K, n, 1)
        got = _check(gpu, code, np.zeros(n * 3000, dtype=np.int16), B=geom[0], W=geom[1], D=geom[2])
        assert not got[geom[0] or 192:].any()
    assert not _check(gpu, M.Code(K, rng.integers(1, 1 << K, 2).tolist()), np.zeros(2000, dtype=np.int16), B=5, W=2, D=3).any()


def test_the_metrics_bound(gpu):
    """Every value +-32767 / -32768 at n = 3 over windows of 512 steps: the metrics reach their bound of 2^26 and the barred
    states of the first window stay barred."""
    rng = np.random.default_rng(13)
    for K in (3, 7):
        code = M.Code(K, (0o133, 0o171, 0o165) if K == 7 else (7, 5, 7), init_state=1)
        for runs in (1, 7, 1800):
            vals = np.repeat(rng.choice([-32768, 32767], 3600 // runs + 1), runs)[:3600]
            _check(gpu, code, vals, B=256, W=128, D=128)
            _check(gpu, code, vals, B=510, W=1, D=1)
        tx, _ = M.encode(code, rng.integers(0, 2, 1200))
        _check(gpu, code, np.where(tx == 1, 32767, -32768), B=256, W=128, D=128)          # one path earns all of it


def test_calls_that_are_not_final_and_terminated(gpu):
    """ndecided is bbb_conv_plan's (asserted in _decode), the words beyond it are untouched (the guards), and a call too short for
    one whole window decides nothing; a terminated record's last window ends in state 0, in a final call only."""
    rng = np.random.default_rng(14)
    code = M.Code(7, G171, *M.PRESETS["3/4"])
    for nsteps in (1, 255, 256, 257, 1000):
        bits = _check(gpu, code, _noisy(rng, code, nsteps), final=False)
        assert len(bits) == (0 if nsteps < 256 else (nsteps - 64) // 192 * 192)
    assert len(_check(gpu, code, _noisy(rng, code, 100, 95), 0, 95, False, 5, 2, 3)) == 95
    assert len(_check(gpu, code, np.zeros(0, dtype=np.int16))) == 0                    # nin = 0 writes nothing
    assert len(_check(gpu, code, np.zeros(1, dtype=np.int16))) == 0                    # one value does not make step 0, which sends two
    for K in (3, 5, 7):
        plain = _random_code(rng, K, 2, 1)
        term = M.Code(K, plain.gens, plain.period, plain.keep, plain.init_state, terminated=True)
        vals = rng.integers(-100, 101, 2 * 500).astype(np.int16)
        a, b = _check(gpu, plain, vals), _check(gpu, term, vals)
        assert not b[-(K - 1):].any() and np.array_equal(a[:384], b[:384])
        assert np.array_equal(_check(gpu, term, vals, final=False), _check(gpu, plain, vals, final=False))
        _check(gpu, term, (vals >= 0).astype(np.int64), hard=True, B=5, W=2, D=3)


@pytest.mark.parametrize("punct,geom", (("3/4", (0, 0, 0)), (None, (5, 2, 3)), ("7/8", (64, 0, 0))))
def test_conv_code_and_a_stream_cut_at_random_points(gpu, punct, geom):
    """ConvCode.encode and .decode are the C calls, and a ConvStream cut at random points gives the bits of one call."""
    rng = np.random.default_rng(15 + geom[0])
    code = M.Code(7, G171, *(M.PRESETS[punct] if punct else (1, None)))
    cc = gpu.ConvCode(7, G171, punct, geometry=geom)
    data = rng.integers(0, 2, 5000)
    packed = torch.from_numpy(_pack_at(data, 0)).to("cuda:0")
    tx, ntx = cc.encode(packed, len(data))
    want_tx, _ = M.encode(code, data)
    assert ntx == len(want_tx) == cc.idx(len(data)) and np.array_equal(_unpack(tx, ntx), want_tx)
    # in two pieces through the state tensor
    st = torch.tensor([cc.init_state], dtype=torch.int32, device="cuda:0")
    t1, n1 = cc.encode(packed[:10], 640, 0, st)
    t2, n2 = cc.encode(packed[10:], len(data) - 640, 640, st)
    assert np.array_equal(np.concatenate([_unpack(t1, n1), _unpack(t2, n2)]), want_tx) and st.item() == M.encode(code, data)[1]
    rx = ((2 * want_tx.astype(np.int64) - 1) * 64 + np.rint(rng.normal(0, 45, ntx))).astype(np.int16)
    want, windows = M.run(code, rx, B=geom[0], W=geom[1], D=geom[2])
    rt = torch.from_numpy(rx).to("cuda:0")
    bits, nd = cc.decode(rt)
    assert nd == len(want) and np.array_equal(_unpack(bits, nd), want)
    assert cc.stats() == dict(windows=windows, steps=len(want))
    hard = (rx >= 0).astype(np.int64)
    hb, hn = cc.decode(torch.from_numpy(_pack_at(hard, 0)).to("cuda:0"), hard=True, nbits=len(hard))
    assert np.array_equal(_unpack(hb, hn), M.run(code, hard, B=geom[0], W=geom[1], D=geom[2], hard=True)[0])
    s = cc.stream()
    cuts = sorted(rng.integers(0, len(rx), 12).tolist() + [0, 7, 7, len(rx)])
    got = []
    for lo, hi in zip([0] + cuts, cuts + [len(rx)]):
        b, nb = s.push(rt[lo:hi])
        got.append(_unpack(b, nb))
    b, nb = s.finish()
    got.append(_unpack(b, nb))
    assert np.array_equal(np.concatenate(got), want)
    assert np.array_equal(M.stream(code, rx, cuts, *geom), want)                       # the same cuts in the model


def test_rx_count_errors_with_fec(gpu):
    """PRBS-15 data through (0171, 0133) at rate 3/4 onto a noisy two-level waveform: RX.count_errors(fec=...) decodes the hard
    decisions of RX.slice in one final call and counts the decoded bits against the PRBS, behind whichever path made the decisions."""
    rng = np.random.default_rng(16)
    n = 6000
    cc = gpu.ConvCode(7, G171, "3/4")
    code = M.Code(7, G171, *M.PRESETS["3/4"])
    data = gpu.PRBS(15, device=0).generate(n)
    tx, ntx = cc.encode(data, n)
    txb = _unpack(tx, ntx)
    x = ((2 * txb.astype(np.int64) - 1) * 64 + np.rint(rng.normal(0, 30, ntx))).astype(np.int16)
    xt = torch.from_numpy(x).to("cuda:0")
    rx = gpu.RX(15, 1, 0)
    uncoded = (x >= 0) != txb
    raw, nraw = rx.slice(xt)
    assert nraw == ntx and np.array_equal(_unpack(raw, nraw), x >= 0)
    dec, nd = rx.slice(xt, fec=cc)
    own, n2 = cc.decode(raw, hard=True, nbits=nraw)
    want, _ = M.run(code, (x >= 0).astype(np.int64), hard=True)
    assert nd == n2 == n and torch.equal(dec, own) and np.array_equal(_unpack(dec, nd), want)
    errors = int((want != _unpack(data, n)).sum())
    assert rx.count_errors(xt, fec=cc) == (errors, n) and 0 < errors < int(uncoded.sum())
    assert rx.detect(xt, fec=cc)["errors"] == rx.prbsdet.run_stream(own, n2)["errors"]
    assert rx.count_errors(xt, rx_filter=gpu.FIR([1]), fec=cc) == (errors, n)           # the filter {1} is the plain slicer


@pytest.mark.parametrize("name", sorted(H.MULTIPASS))
def test_more_than_two_passes_of_the_grid(gpu, name):
    """ceil(nblocks / wpg) = 2 * 16 * cus + 5 groups of windows at B = W = D = 8 (tests/test_conv_host.py builds the records and
    holds bbb_conv_model_host, the expected bits here, to the model on three stretches): workgroup 0 takes three turns of its
    loop over the groups, re-using the stage and the survivor words, and the last pass does not fill the grid.  The encoder's
    loop is out of reach at this cost: its grid is capped at 2^20 workgroups of 256 words a pass."""
    code, vals, hard, nblocks, want = H.multipass_expected(name, grid.cus())
    B, W, D = H.MULTIPASS_GEOM
    bits, stats = _decode(gpu, code, vals, B=B, W=W, D=D, hard=hard, in_off=3, bits_off=1)
    bad = np.flatnonzero(bits != want)
    assert len(bits) == len(want) and len(bad) == 0, f"{len(bad)} bits differ, the first at step {bad[0]} of {len(want)}"
    assert stats == dict(windows=nblocks, steps=len(want))


# ---- the closed loop ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("1/2", "3/4"))
def test_closed_loop_counts_equal_the_cpu(gpu, name):
    """The recipe of tests/test_conv_host.py through ConvCode on the GPU: encode, the same noise, hard and soft decoding leave
    what the model found, soft < hard < the channel's errors."""
    code, data, tx, rx = M.loop_record(name)
    want = M.LOOP_COUNTS[name]
    cc = gpu.ConvCode(7, G171, M.LOOP[name]["puncture"])
    packed = torch.from_numpy(_pack_at(data, 0)).to("cuda:0")
    t, ntx = cc.encode(packed, len(data))
    assert ntx == want["ncoded"] and np.array_equal(_unpack(t, ntx), tx)
    rt = torch.from_numpy(rx).to("cuda:0")
    hard_bits, nh = gpu.RX(7, 1, 0).slice(rt)
    channel = int((_unpack(hard_bits, nh) != tx).sum())
    hb, hn = cc.decode(hard_bits, hard=True, nbits=nh)
    sb, sn = cc.decode(rt)
    got = dict(ncoded=ntx, channel=channel, hard=int((_unpack(hb, hn) != data).sum()), soft=int((_unpack(sb, sn) != data).sum()))
    print(name, got)
    assert hn == sn == len(data) and got == want
    assert got["soft"] < got["hard"] < got["channel"]
