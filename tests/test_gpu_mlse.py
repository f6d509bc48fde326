"""bbb_mlse_run on the GPU, bit for bit against tests/mlse_model.py: every memory and decimation, small and default windows,
records around the block sizes, calls that start inside a block, calls that are not final, a stream cut at random points, the
tie rules, the metrics' bound, more than two passes of the grid, and the closed loop of tests/test_mlse_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import fir_model
import grid
import dfe_model
import mlse_model as M
import test_mlse_host as H

pytestmark = pytest.mark.gpu

GUARD = -0x0123456789ABCDEF
GEOMS = ((5, 2, 3), (64, 0, 0), (0, 0, 0), (256, 128, 128))


def _call(gpu, x, nb, taps, g, spb, phase=0, shift=0, first=0, final=True, init=0, B=0, W=0, D=0, in_off=0, bits_off=0, unaligned=False):
    """One bbb_mlse_run through the C ABI on tensors placed `*_off` elements behind an aligned address; the words next to the
    output must stay as they were.  Returns (bits uint8, stats dict)."""
    from basebandboard_amd import _lib
    dev = torch.device("cuda", 0)
    x = np.asarray(x, dtype=np.int16)
    nin = len(x) - nb
    nsym, nd, _ = M.plan(nin, spb, phase, len(taps), first, final, B, W, D)
    nwords = (nd + 63) // 64
    buf = torch.zeros(in_off + len(x) + 8, dtype=torch.int16, device=dev)
    buf[in_off:in_off + len(x)] = torch.from_numpy(x).to(dev)
    bits = torch.full((bits_off + nwords + 2,), GUARD, dtype=torch.int64, device=dev)
    stats = torch.tensor([1000, 2000], dtype=torch.int64, device=dev)
    c = _lib.MlseCfg()
    c.ff.ntaps = len(taps)
    for i, v in enumerate(taps):
        c.ff.taps[i] = v
    c.ff.shift, c.ff.decim, c.ff.phase, c.ff.out_bytes = shift, spb, phase, 2
    c.mem = len(g) - 1
    for i, v in enumerate(g):
        c.g[i] = v
    c.init_state, c.block_symbols, c.warmup_symbols, c.lookahead_symbols = init, B, W, D
    got = C.c_uint64()
    p_in, p_bits = buf.data_ptr() + 2 * (in_off + nb), bits.data_ptr() + 8 * (bits_off + 1)
    if unaligned:
        assert p_in % 16 and p_bits % 16, (p_in % 16, p_bits % 16)
    _lib.check(_lib.lib().bbb_mlse_run(C.c_void_p(p_in), nin, nb, first, int(final), C.byref(c), C.c_void_p(p_bits),
                                       C.c_void_p(stats.data_ptr()), C.byref(got), 0,
                                       C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "bbb_mlse_run")
    assert got.value == nd, "ndecided is not bbb_mlse_plan's"
    w = bits.cpu().numpy()
    assert (w[:bits_off + 1] == GUARD).all() and w[-1] == GUARD, "a word next to bits_packed_dev was written"
    words = w[bits_off + 1:-1].view(np.uint64)
    got_bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    assert not got_bits[nd:].any(), "the unused bits of the last word are not 0"
    stv = (stats.cpu().numpy() - np.array([1000, 2000])).tolist()
    return got_bits[:nd], dict(zip(("windows", "symbols"), stv))


def _check(gpu, x, nb, taps, g, spb, phase=0, shift=0, first=0, final=True, init=0, B=0, W=0, D=0, **off):
    x = np.asarray(x)
    bits, stats = _call(gpu, x, nb, taps, g, spb, phase, shift, first, final, init, B, W, D, **off)
    want, windows = M.run(x[nb:], taps, g, spb, phase, shift, x[:nb], first, final, init, B, W, D)
    bad = np.flatnonzero(bits != want)
    assert len(bits) == len(want) and len(bad) == 0, f"{len(bad)} bits differ, the first at symbol {bad[0]} of {len(want)}"
    assert stats == (dict(windows=windows, symbols=len(want)) if len(want) else dict(windows=0, symbols=0))
    return bits


def _record(rng, nsym, spb, g, extra=0):
    """Noisy +-1 data through the target itself at `spb` samples per symbol, so that the detector has something to decide and
    noise enough to make the windows matter."""
    a = sum(abs(v) for v in g)
    d = rng.choice([-1, 1], nsym + len(g))
    sym = sum(g[i] * d[len(g) - i:len(g) - i + nsym] for i in range(len(g)))
    return np.repeat(sym, spb)[:nsym * spb - extra] + rng.integers(-a, a + 1, nsym * spb - extra)


@pytest.mark.parametrize("spb", (1, 2, 3, 8, 256))
def test_every_mem_geometry_and_record_length(gpu, spb):
    """mem 1..4 under the four geometries (a tiny window, B = 64 with the default edges, the defaults, B + W + D = 512), records of
    1, B - 1, B, B + 1, 1000 and 4099 symbols, ragged nin, every pointer off 16-byte alignment."""
    rng = np.random.default_rng(200 + spb)
    for mem in (1, 2, 3, 4):
        for B, W, D in GEOMS:
            g = (rng.integers(20, 60, mem + 1) * rng.choice([-1, 1], mem + 1)).tolist()
            ntaps = int(rng.choice([1, 7, 8, 9, 33]))
            taps = [1] + rng.integers(-1, 2, ntaps - 1).tolist()                  # y stays of the target's size
            Bq = B or 192
            for nsym in (1, Bq - 1, Bq, Bq + 1, 1000, 4099):
                phase = int(rng.integers(0, spb))
                x = _record(rng, nsym, spb, g, extra=int(rng.integers(0, spb - phase)))
                assert fir_model.nout(len(x), spb, phase) == nsym
                _check(gpu, x, 0, taps, g, spb, phase, shift=int(rng.integers(0, 2)), init=int(rng.integers(0, 16)), B=B, W=W, D=D,
                       in_off=1 + 2 * mem, bits_off=2 * (mem & 1), unaligned=True)


def test_first_symbol_anywhere_with_full_and_short_history(gpu):
    """A call that starts at symbol 1, at a block boundary and inside a block decides from the block's absolute window: with
    the history the window reaches (and more), and with less, where the rest counts as 0."""
    rng = np.random.default_rng(12)
    taps, g = [1] + rng.integers(-1, 2, 8).tolist(), [50, -30, 20]
    for spb, (B, W, D) in ((8, (5, 2, 3)), (3, (0, 0, 0)), (1, (64, 0, 0)), (256, (5, 2, 3))):
        Bq = B or 192
        for first in (0, 1, Bq, Bq + 1, 3 * Bq - 1, 7 * Bq + Bq // 2, (1 << 40) + 3):
            phase = int(rng.integers(0, spb))
            wanted = M.nbefore_wanted(first, spb, len(taps), phase, B, W, D)
            for nb in sorted({wanted + 13, wanted // 2, 0}):
                for final in (True, False):
                    x = _record(rng, 2 * Bq + 40 + (nb + spb - 1) // spb, spb, g)
                    _check(gpu, x, nb, taps, g, spb, phase, first=first, final=final, init=2, B=B, W=W, D=D, in_off=nb & 7)


def test_tie_rules_on_all_zero_records(gpu):
    z = np.zeros(12 * 8, dtype=np.int16)
    assert _check(gpu, z, 0, [1, 1], [3, 3], 8, B=12, W=1, D=1).tolist() == [1, 0] * 6
    assert _check(gpu, z, 0, [1, 1], [3, -3, 0], 8, init=1, B=12, W=1, D=1).tolist() == [1] * 12
    # every ACS ties in every window
    for mem, geom in ((1, (5, 2, 3)), (2, (0, 0, 0)), (3, (64, 0, 0)), (4, (5, 2, 3))):
        assert not _check(gpu, np.zeros(3000, dtype=np.int16), 0, [1], [0] * (mem + 1), 3, 1, init=5, B=geom[0], W=geom[1], D=geom[2]).any()
    assert _check(gpu, np.zeros(1000, dtype=np.int16), 0, [1], [3, 3], 1, B=5, W=2, D=3)[:5].tolist() == [1, 0, 1, 0, 1]


def test_the_metrics_bound(gpu):
    """y = +-32768 through a saturating shift against sum |g| = 2^20 over windows of 512 symbols: the metrics reach their
    bound of 2^50 and the barred states of the first window stay barred."""
    rng = np.random.default_rng(13)
    taps = [32767, 32767]
    for g in ([1 << 20, 0], [1 << 19, -(1 << 19)], [1 << 18, -(1 << 18), 1 << 18, -(1 << 18)], [-(1 << 18), 1 << 18, 1 << 17, 1 << 17, 1 << 18]):
        for runs in (1, 7, 600):
            x = np.repeat(rng.choice([-32768, 32767], 2400 // runs + 1), runs)[:2400]
            y = M.y_values(x, taps, 2, 1, 3, (), 0, 1200)
            assert set(y.tolist()) >= {-32768, 32767}
            _check(gpu, x, 0, taps, g, 2, 1, shift=3, init=1, B=448, W=32, D=32)
            _check(gpu, x, 0, taps, g, 2, 1, shift=3, init=1, B=510, W=1, D=1)


def test_calls_that_are_not_final(gpu):
    """ndecided is bbb_mlse_plan's (asserted in _call), the words beyond it are untouched (the guards), and a call too short for
    one whole window decides nothing."""
    rng = np.random.default_rng(14)
    taps, g = [1, 2, 1], [40, 25]
    for nsym in (1, 223, 224, 225, 1000):
        bits = _check(gpu, _record(rng, nsym, 4, g), 0, taps, g, 4, 3, final=False)
        assert len(bits) == (0 if nsym < 224 else (nsym - 32) // 192 * 192)
    assert len(_check(gpu, _record(rng, 100, 4, g), 0, taps, g, 4, first=95, final=False, B=5, W=2, D=3)) == 95
    assert len(_check(gpu, np.zeros(0, dtype=np.int16), 0, taps, g, 4)) == 0           # nin = 0 writes nothing
    assert len(_check(gpu, np.zeros(2, dtype=np.int16), 0, taps, g, 4, 3)) == 0        # a record that ends in front of its first symbol


@pytest.mark.parametrize("spb,geom", ((8, (0, 0, 0)), (3, (5, 2, 3)), (1, (64, 0, 0))))
def test_a_capture_cut_at_random_points_equals_one_call(gpu, spb, geom):
    rng = np.random.default_rng(15 + spb)
    g = [60, 45, -20]
    nsym = 5000
    x = _record(rng, nsym, spb, g).astype(np.int16)
    taps = [2] + rng.integers(-2, 3, 18).tolist()
    want, windows = M.run(x, taps, g, spb, spb - 1, 2, B=geom[0], W=geom[1], D=geom[2])
    d = gpu.MLSE(gpu.FIR(taps, shift=2), g, spb, spb - 1, block_symbols=geom[0], warmup_symbols=geom[1], lookahead_symbols=geom[2])
    xt = torch.from_numpy(x).to("cuda:0")
    bits, nbits = d.slice(xt)
    assert nbits == len(want) and np.array_equal(np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:nbits], want)
    assert d.stats() == dict(windows=windows, symbols=nsym)
    s = d.stream()
    cuts = sorted(rng.integers(0, len(x), 12).tolist() + [0, 7, 7, len(x)])
    got = []
    for lo, hi in zip([0] + cuts, cuts + [len(x)]):
        b, nb = s.push(xt[lo:hi])
        got.append(np.unpackbits(b.cpu().numpy().view(np.uint8), bitorder="little")[:nb])
    b, nb = s.finish()
    got.append(np.unpackbits(b.cpu().numpy().view(np.uint8), bitorder="little")[:nb])
    assert np.array_equal(np.concatenate(got), want)
    assert d.stats()["symbols"] == 2 * nsym
    # the same cuts in the model
    assert np.array_equal(M.stream(x, taps, g, spb, cuts, spb - 1, 2, B=geom[0], W=geom[1], D=geom[2]), want)


@pytest.mark.parametrize("name", sorted(H.MULTIPASS))
def test_more_than_two_passes_of_the_grid(gpu, name):
    """ceil(nblocks / wpg) = 2 * 16 * cus + 5 groups of windows (tests/test_mlse_host.py builds the records and holds
    bbb_mlse_model_host, the expected bits here, to the model on three stretches): workgroup 0 takes three turns of its loop over
    the groups, re-using the image, the span and the survivor words, and the last pass does not fill the grid.  Sixteen and two
    states at B = W = D = 8 in the 256-thread kernel, and B + W + D = 512 at four states, which mlse_shape gives the 64-thread
    kernel with two steps in flight."""
    x, g, (B, W, D), nblocks, want = H.multipass_expected(name, grid.cus())
    bits, stats = _call(gpu, x, 0, H.MULTIPASS_TAPS, g, 1, 0, H.MULTIPASS_SHIFT, init=1, B=B, W=W, D=D, in_off=3, bits_off=1)
    bad = np.flatnonzero(bits != want)
    assert len(bits) == len(want) and len(bad) == 0, f"{len(bad)} bits differ, the first at symbol {bad[0]} of {len(want)}"
    assert stats == dict(windows=nblocks, symbols=len(want))


def test_closed_loop_counts_equal_the_cpu(gpu, oracle):
    """The echo channel's noisy record through RX.count_errors: the linear receiver, the DFE and the sequence detector leave
    what tests/test_mlse_host.py found on the CPU, and the sequence detector strictly fewer than the DFE."""
    L = M.LOOP
    y, h, sigma2, _ = M.loop_record(oracle)
    yt = torch.from_numpy(y).to("cuda:0")
    phase = (17 + L["cursor"]) % 8
    m = gpu.MLSE.mmse(h, 8, L["cursor"], L["nff"], L["mem"], sigma2)
    d = gpu.DFE.mmse(h, 8, L["cursor"], L["nff"], L["mem"], sigma2)
    assert m.ff.taps == d.ff.taps == M.LOOP_FF and m.g == M.LOOP_G and m.ff.shift == M.LOOP_SHIFT and d.fb == M.LOOP_FB
    rx = gpu.RX(dfe_model.LOOP["k"], 8, phase)
    first = (17 + L["cursor"]) // 8 * 8
    e_mlse = rx.count_errors(yt, first_sample=first, mlse=m)
    e_dfe = rx.count_errors(yt, first_sample=first, dfe=d)
    e_lin = rx.count_errors(yt, first_sample=first, rx_filter=gpu.FIR.mmse(h, 8, L["cursor"], L["nff"], sigma2))
    print("linear", e_lin, "dfe", e_dfe, "mlse", e_mlse)
    assert e_mlse == (M.LOOP_MLSE_ERRORS, M.LOOP_BITS) and e_dfe == (M.LOOP_DFE_ERRORS, M.LOOP_BITS) and e_lin == (M.LOOP_LINEAR_ERRORS, M.LOOP_BITS)
    assert e_mlse[0] < e_dfe[0] and e_dfe[0] >= 50
    # RX.slice(mlse=...) is the detector's own call on the samples from the first bit on, and RX.detect reads the same bits
    bits, nbits = rx.slice(yt, first_sample=first, mlse=m)
    own, n2 = m.slice(yt[first - 11:], nbefore=11, phase=phase)
    assert nbits == n2 == M.LOOP_BITS and torch.equal(bits, own)
    want, _ = M.run(y[first:], M.LOOP_FF, M.LOOP_G, 8, phase, M.LOOP_SHIFT, y[:first])
    assert np.array_equal(np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:nbits], want)
    assert rx.detect(yt, first_sample=first, mlse=m)["errors"] == rx.prbsdet.run_stream(own, n2)["errors"]
    with pytest.raises(ValueError, match="not both"):
        rx.slice(yt, dfe=d, mlse=m)
    with pytest.raises(ValueError, match="spb"):
        rx.slice(yt, stride=4, mlse=m)
