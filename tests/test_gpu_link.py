"""The filtered link on the GPU, bit-exact: bbb_link_sweep_* / LinkSweep against the raw analysers (identity filter), against
the numpy model of tests/link_model.py on the oracle's waveform, against the product's own composition (TX.generate ->
FIR.slice / FIR.filter -> capture_eye), over thresholds in units of acc, cuts of a range, the start of the stream, a range
far out, more than two passes of the kernel's grid, many settings at once, the handle left as it was, and the C++ example."""
import functools
import json
import subprocess

import numpy as np
import pytest
import torch

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from basebandboard_amd.eye import BIT_SAMPLE0, EyeConfig, capture_eye
from basebandboard_amd.txsweep import TxSetting
from conftest import ROOT

import grid
import link_model
from test_gpu_eye import CONFIGS, make_tx, source_bits, tx_taps, u64

pytestmark = pytest.mark.gpu
CHUNK = (1 << 16) + 8
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

TAPS256 = [256, -256] * 127 + [256, -255]                 # sum |h| = 65535, mixed signs


def own_setting(tx, threshold=0, strict=False):
    return TxSetting(noise_var=tx.noise_var, bit_en=tx.bit_en, noise_en=tx.noise_en, threshold=threshold, strict=strict)


def run_link(tx, fir, delay, first, n, settings=None, eye=None, chunk=0):
    with bbb.LinkSweep(tx, settings or [own_setting(tx)], fir, delay, eye, chunk_samples=chunk) as s:
        r = s.run(n, first)
    return (u64(r[0]), u64(r[1])) if eye is not None else (u64(r), None)


@functools.lru_cache(maxsize=None)
def oracle_wave(kw_items, lo, count):
    """TX.x of make_tx(**kw), samples [lo, lo + count), from the CPU oracle (computed once per configuration and range)"""
    import oracle as O
    kw = dict(kw_items)
    tx = make_tx(**kw)
    lut = O.Lutopt(path=O.data_path(kw.get("lut", 256)))
    x = O.tx(lut, 1, tx_taps(tx), tx.prbs.k, count, first_sample=lo, source=tx.src_sel, bit_en=int(tx.bit_en),
             noise_en=int(tx.noise_en), noise_var=tx.noise_var, warmup=16)
    x.setflags(write=False)
    return x


def freeze(kw):
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items()))


def model(kw, fir, delay, first, n, threshold=0, strict=False, eye=None, x=None, x0=None):
    tx = make_tx(**kw)
    if x is None:
        x0, count = link_model.wave_range(first, n, len(fir.taps), delay)
        x = oracle_wave(freeze(kw), x0, count)
    bit_of = lambda lo, cnt: source_bits(tx.prbs.k, tx.src_sel == 1, lo, cnt)          # noqa: E731
    e = (eye.ncols, eye.shift, eye.col_origin) if eye is not None else None
    return link_model.link(x, x0, first, n, fir.taps, delay, fir.shift, threshold, strict, bit_of, e)


# ---- 1. the identity filter gives the raw analysers' results ---------------------------------------------------------

@pytest.mark.parametrize("name, kw, first, n, ekw, chunk", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_identity_filter_equals_the_raw_analysers(gpu, name, kw, first, n, ekw, chunk):
    eye = EyeConfig(**{**dict(col_origin=BIT_SAMPLE0), **ekw})
    st = own_setting(make_tx(**kw), eye.threshold, eye.strict)
    cnt, hist = run_link(make_tx(**kw), bbb.FIR([1]), 0, first, n, [st], eye, chunk)
    with bbb.TxBerSweep(make_tx(**kw), [st], chunk_samples=chunk) as s:
        assert np.array_equal(cnt, u64(s.run(n, first)))
    h, tub = make_tx(**kw).eye(n, first_sample=first, eye=eye, chunk_samples=chunk)
    assert np.array_equal(hist[0], u64(h)) and np.array_equal(cnt[0], u64(tub))
    # ... and TX.eye / TX.ber_sweep take the same road when they are given the filter
    h2, t2 = make_tx(**kw).eye(n, first_sample=first, eye=eye, chunk_samples=chunk, rx_filter=bbb.FIR([1]))
    assert np.array_equal(u64(h2), u64(h)) and np.array_equal(u64(t2), u64(tub))


def test_tx_ber_sweep_with_filter(gpu):
    tx = make_tx(k=7, nv=3)
    n, fir = 100_003, bbb.FIR.moving_average()
    grid = u64(tx.ber_sweep(n, noise_vars=[0, 9, 15], shape_sels=[4, 16], first_sample=5, rx_filter=fir, delay=2, threshold=7))
    assert grid.shape == (2, 3, 8, 2)
    for i, sel in enumerate((4, 16)):
        for j, v in enumerate((0, 9, 15)):
            want, _ = model(dict(k=7, nv=v, shape=sel), fir, 2, 5, n, threshold=7)
            assert np.array_equal(grid[i, j], want), (sel, v)
    assert np.array_equal(u64(tx.ber_sweep(n, noise_vars=[9], first_sample=5, rx_filter=fir))[0, 0],
                          run_link(make_tx(k=7, nv=9), fir, 1, 5, n)[0][0])               # delay None: FIR.delay() = 1
    with pytest.raises(ValueError):
        tx.ber_sweep(1000, delay=2)
    with pytest.raises(ValueError):
        tx.eye(1000, delay=2)


# ---- 2. against the model on the oracle's waveform -------------------------------------------------------------------

MA, MA_PIPE = [1, 1, 1, 1], [0, 0, 0, 1, 1, 1, 1]
NINE = [3, -1, 4, 1, -5, 9, 2, -6, 5]
BASE = dict(k=7, nv=8)
MODEL_CASES = [
    # (name, make_tx kwargs, taps (None: matched to the TX's set), fir shift, delay (None: FIR.delay()), first, n, ncols, threshold, strict, chunk)
    ("two_d0", BASE, [1, 1], 0, 0, 0, 100_003, 8, 0, False, 0),
    ("two_d1", BASE, [1, 1], 0, 1, 3, 90_001, 64, 0, False, CHUNK),
    ("two_d2", BASE, [1, 1], 1, 2, 44, 80_000, 8, -3, True, 0),
    ("two_d7", BASE, [1, 1], 0, 7, 45, 80_007, 64, 0, False, 0),
    ("ma_d0", BASE, MA, 0, 0, (1 << 16) + 5, 100_000, 64, 0, False, CHUNK),
    ("ma_d1", BASE, MA, 2, 1, 0, 150_001, 8, 0, False, CHUNK),
    ("ma_d2", dict(k=31, nv=15), MA, 0, 2, 3, 3 * (1 << 16) + 1234, 64, 5, False, CHUNK),
    ("ma_d7", BASE, MA, 0, 7, 44, 80_001, 8, 0, True, 0),
    ("ma_pipelined", BASE, MA_PIPE, 2, None, 45, 100_000, 64, 0, False, 0),
    ("nine", dict(k=31, nv=12, shape=4), NINE, 3, None, 3, 120_000, 16, 100, False, CHUNK),
    ("matched64", dict(k=7, nv=15, shape=16), None, 8, None, 0, 100_001, 64, 0, False, CHUNK),
    ("t256_shift0", dict(k=7, nv=15), TAPS256, 0, 128, 44, 90_000, 64, 0, False, CHUNK),
    ("t256_shift12", dict(k=31, nv=8), TAPS256, 12, 3, (1 << 16) + 5, 80_000, 8, -1000, False, 0),
    ("pulser", dict(src=1, nv=4, shape=20), MA, 0, 2, 44, 3 * (1 << 16) + 5, 64, 0, False, CHUNK),
    ("bit_en_0", dict(k=7, bit_en=0, nv=8), MA, 0, 1, 3, 80_001, 8, -3, False, 0),
    ("noise_off", dict(k=31, noise_en=0, shape=8), MA, 0, 2, 0, 150_000, 16, 0, False, CHUNK),
    ("nv0", dict(k=7, nv=0, shape=0), NINE, 0, 4, 45, 100_001, 8, 0, True, 0),
    ("nv15", dict(k=7, nv=15, shape=31), MA, 0, 2, 0, 100_000, 64, 0, False, 0),
    ("wrap12", dict(k=7, nv=15, taps=[255] * 64), MA, 1, 2, 0, 90_000, 64, 100, True, CHUNK),
    ("n16", dict(k=31, nv=8, lut=16), MA, 0, 2, 3, 120_000, 64, 0, False, CHUNK),
    ("n64", dict(k=7, nv=12, lut=64), [1, 1], 0, 0, 44, 100_000, 16, 0, False, 0),
]


@pytest.mark.parametrize("name, kw, taps, fshift, delay, first, n, ncols, threshold, strict, chunk", MODEL_CASES,
                         ids=[c[0] for c in MODEL_CASES])
def test_link_vs_model_on_the_oracle_waveform(gpu, name, kw, taps, fshift, delay, first, n, ncols, threshold, strict, chunk):
    fir = bbb.FIR(taps, shift=fshift) if taps is not None else bbb.FIR.matched(tx_taps(make_tx(**kw)), shift=fshift)
    delay = fir.delay() if delay is None else delay
    eye = EyeConfig(ncols=ncols, shift=4, col_origin=BIT_SAMPLE0)
    tx = make_tx(**kw)
    cnt, hist = run_link(tx, fir, delay, first, n, [own_setting(tx, threshold, strict)], eye, chunk)
    tub, h = model(kw, fir, delay, first, n, threshold, strict, eye)
    assert np.array_equal(cnt[0], tub), (cnt[0].tolist(), tub.tolist())
    assert np.array_equal(hist[0], h)
    assert hist[0].sum() == n and cnt[0][:, 0].sum() == sum(1 for s in range(first, first + n) if s >= BIT_SAMPLE0)
    if name == "t256_shift0":
        assert hist[0][0].sum() > 0 and hist[0][255].sum() > 0               # z saturates: rows 127 - 127 and 127 + 128


# ---- 3. against the GPU composition ----------------------------------------------------------------------------------

@pytest.mark.parametrize("taps, fshift, delay, first, n, threshold, strict", [
    (MA, 0, 2, 0, 200_000, 0, False), (MA_PIPE, 2, 4, 3, 100_001, -7, True), (TAPS256, 12, 100, (1 << 16) + 5, 120_000, 300, False)])
def test_link_vs_gpu_composition(gpu, taps, fshift, delay, first, n, threshold, strict):
    kw = dict(k=31, nv=11, shape=12)
    fir = bbb.FIR(taps, shift=fshift)
    eye = EyeConfig(ncols=32, shift=4, col_origin=BIT_SAMPLE0)
    tx = make_tx(**kw)
    cnt, hist = run_link(tx, fir, delay, first, n, [own_setting(tx, threshold, strict)], eye, CHUNK)
    lo, count = link_model.wave_range(first, n, len(taps), delay)
    x = make_tx(**kw).generate(count, first_sample=lo)                       # with its true history in front
    nbefore = first + delay - lo                                             # x[nbefore + r] is waveform sample first + delay + r
    for p in range(8):
        m_lo = max(0, -((first - BIT_SAMPLE0 - p) // -8))                    # the first bit decided at this phase inside the range
        r0 = 8 * m_lo + BIT_SAMPLE0 + p - first
        skip = r0 - r0 % 8
        w, nb = fir.slice(x, stride=8, phase=r0 % 8, threshold=threshold, strict=strict, nbefore=nbefore + skip)
        dec = np.unpackbits(w.cpu().numpy().view(np.uint8), bitorder="little")[:nb]
        errs = int((dec != source_bits(31, False, m_lo, nb)).sum())
        assert (int(cnt[0][p, 0]), int(cnt[0][p, 1])) == (nb, errs), p
    z = fir.filter(x, nbefore=nbefore)
    assert z.numel() == n
    assert np.array_equal(hist[0], u64(capture_eye(z, first_sample=first, eye=eye)))


# ---- 4. thresholds in units of acc -----------------------------------------------------------------------------------

def test_thresholds_in_acc_units(gpu):
    kw, fir, delay, first, n = dict(k=7, nv=10), bbb.FIR(MA), 2, 3, 100_000
    tx = make_tx(**kw)
    cases = [(0, False), (0, True), (1000, False), (-1000, False), (1000, True), (INT32_MIN, False), (INT32_MAX, True)]
    cnt, _ = run_link(tx, fir, delay, first, n, [own_setting(tx, t, s) for t, s in cases], chunk=CHUNK)
    for i, (t, s) in enumerate(cases):
        assert np.array_equal(cnt[i], model(kw, fir, delay, first, n, t, s)[0]), (t, s)
    assert not np.array_equal(cnt[2], cnt[0]) and not np.array_equal(cnt[3], cnt[0])
    # every decision 1: the errors are the zero bits; every decision 0: the one bits
    bits = source_bits(7, False, 0, (first + n) // 8 + 1)
    for p in range(8):
        nb = int(cnt[5][p, 0])
        assert int(cnt[5][p, 1]) == int((bits[:nb] == 0).sum()) and int(cnt[6][p, 1]) == int((bits[:nb] == 1).sum())


# ---- 5. split invariance ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("taps, delay", [(MA, 2), (TAPS256, 200)])
def test_split_invariance(gpu, taps, delay):
    kw, fir = dict(k=31, nv=10), bbb.FIR(taps, shift=6)
    eye = EyeConfig(ncols=16, shift=4, col_origin=BIT_SAMPLE0)
    first, n = 7, 200_003
    whole = run_link(make_tx(**kw), fir, delay, first, n, None, eye, CHUNK)
    sizes = [1, len(taps) - 1, 8 * 1000 + 3, CHUNK - 1, CHUNK + 1, 1, 7]
    with bbb.LinkSweep(make_tx(**kw), [own_setting(make_tx(**kw))], fir, delay, eye, chunk_samples=CHUNK) as s:
        at, cnt, hist = first, None, None
        for size in sizes + [first + n - (first + sum(sizes))]:
            cnt, hist = s.run(size, at, cnt, hist)
            at += size
        assert at == first + n
        assert np.array_equal(u64(cnt), whole[0]) and np.array_equal(u64(hist), whole[1])
        # one chunk for the whole range; and added to, never overwritten
    with bbb.LinkSweep(make_tx(**kw), [own_setting(make_tx(**kw))], fir, delay, eye) as s:
        s.run(n, first, cnt, hist)
    assert np.array_equal(u64(cnt), 2 * whole[0]) and np.array_equal(u64(hist), 2 * whole[1])


# ---- 6. the start of the stream --------------------------------------------------------------------------------------

def test_start_of_the_stream(gpu):
    """first = 0 with 256 taps and delay 200: zero history below sample 0, and only bits m >= 0"""
    kw, fir, delay, n = dict(k=7, nv=8), bbb.FIR(TAPS256, shift=8), 200, 80_000
    eye = EyeConfig(ncols=64, shift=4, col_origin=BIT_SAMPLE0)
    cnt, hist = run_link(make_tx(**kw), fir, delay, 0, n, None, eye, CHUNK)
    tub, h = model(kw, fir, delay, 0, n, eye=eye)
    assert np.array_equal(cnt[0], tub) and np.array_equal(hist[0], h)
    assert cnt[0][:, 0].sum() == n - BIT_SAMPLE0
    # a short range that ends before the first decided bit: a histogram and no bits
    cnt, hist = run_link(make_tx(**kw), fir, delay, 0, 40, None, eye)
    assert cnt[0].sum() == 0 and np.array_equal(hist[0], model(kw, fir, delay, 0, 40, eye=eye)[1])


# ---- 7. far out ------------------------------------------------------------------------------------------------------

def test_far_out(gpu):
    """first_sample beyond 2^33 (the oracle's serial shaper cannot go there): the model on TX.generate's output"""
    kw, fir, delay = dict(k=31, nv=8), bbb.FIR(NINE, shift=2), 4
    first, n = (1 << 33) + 12_345, 3 * (1 << 16) + 77
    eye = EyeConfig(ncols=64, shift=4, col_origin=BIT_SAMPLE0)
    cnt, hist = run_link(make_tx(**kw), fir, delay, first, n, None, eye, CHUNK)
    x0, count = link_model.wave_range(first, n, len(NINE), delay)
    x = make_tx(**kw).generate(count, first_sample=x0).cpu().numpy()
    tub, h = model(kw, fir, delay, first, n, eye=eye, x=x, x0=x0)
    assert np.array_equal(cnt[0], tub) and np.array_equal(hist[0], h)


# ---- 7b. more than two passes of the grid ----------------------------------------------------------------------------------------

def test_more_than_two_passes_of_the_grid(gpu):
    """2048 * (2 * 8 * cus + 5) + 77 samples behind the moving average from an odd first sample, in one chunk: the kernel's grid is
    at most 8 workgroups a compute unit (tests/grid.py), so workgroup 0 takes three or more steps of 2048, alternating its two
    LDS images with the inputs of the next step in flight, and the last pass is ragged.  One ber_sweep and one eye + bathtub call
    against the model on TX.generate's output, as test_far_out takes it."""
    kw, fir, delay, first = dict(k=7, nv=9, shape=16), bbb.FIR(MA), 2, 12_345
    n = 2048 * grid.passes(grid.LINK) + 77
    eye = EyeConfig(ncols=64, shift=4, col_origin=BIT_SAMPLE0)
    x0, count = link_model.wave_range(first, n, len(MA), delay)
    x = make_tx(**kw).generate(count, first_sample=x0).cpu().numpy()
    tub, h = model(kw, fir, delay, first, n, threshold=7, eye=eye, x=x, x0=x0)
    assert h.sum() == n and tub[:, 1].sum() > 0 and tub[:, 0].sum() == n
    sweep = u64(make_tx(k=7, nv=3).ber_sweep(n, noise_vars=[9], shape_sels=[16], first_sample=first, rx_filter=fir, delay=delay, threshold=7))
    assert sweep.shape == (1, 1, 8, 2) and np.array_equal(sweep[0, 0], tub), (sweep[0, 0].tolist(), tub.tolist())
    tx = make_tx(**kw)
    cnt, hist = run_link(tx, fir, delay, first, n, [own_setting(tx, 7)], eye)
    assert np.array_equal(cnt[0], tub), (cnt[0].tolist(), tub.tolist())
    assert np.array_equal(hist[0], h)


# ---- 8. many settings ------------------------------------------------------------------------------------------------

def test_many_settings(gpu):
    """40 settings over three coefficient sets, histograms on: every entry equals the single-setting result"""
    fir, delay, first, n = bbb.FIR(MA), 2, 3, 80_000
    eye = EyeConfig(ncols=8, shift=4, col_origin=BIT_SAMPLE0)
    sets = [4, 16, None]
    custom = [255] * 64
    settings = []
    for i in range(40):
        sel = sets[i % 3]
        settings.append(TxSetting(shape_sel=sel, coeffs=None if sel is not None else custom, noise_var=(5 * i) % 16, bit_en=i != 7,
                                  noise_en=i != 11, threshold=(-20, 0, 33)[i % 3], strict=bool(i & 1)))
    cnt, hist = run_link(make_tx(k=31), fir, delay, first, n, settings, eye, CHUNK)
    assert cnt.shape == (40, 8, 2) and hist.shape == (40, 256, 8)
    for i, st in enumerate(settings):
        c1, h1 = run_link(make_tx(k=31), fir, delay, first, n, [st], eye, CHUNK)
        assert np.array_equal(cnt[i], c1[0]) and np.array_equal(hist[i], h1[0]), i
    assert len({cnt[i, :, 1].tobytes() for i in range(40)}) > 20


# ---- 9. the handle is left as it was ---------------------------------------------------------------------------------

def test_handle_state(gpu):
    """After open / run / close, bbb_awgn_stream_next on the handle gives what it would have given without them"""
    def reads(with_link):
        tx = make_tx(k=7, nv=9)
        out = []
        with tx.grng.stream(50_000, first_step=1000) as s:
            out.append(s.next().clone())
            if with_link:
                run_link(tx, bbb.FIR(MA), 2, 5, 3 * (1 << 16) + 11, None, EyeConfig(col_origin=BIT_SAMPLE0), CHUNK)
            out.append(s.next().clone())
            out.append(s.read(1234).clone())
            pos = s.tell()
        out.append(tx.generate(100_000, first_sample=1000, stream_on=False))
        return out, pos
    a, pa = reads(True)
    b, pb = reads(False)
    assert pa == pb and all(torch.equal(x, y) for x, y in zip(a, b))


def test_unsupported_handle(gpu):
    """a handle bbb_tx_fill_i16 refuses with noise on (k = 512) is refused here too, and served with noise off"""
    with pytest.raises(_lib.BbbError) as e:
        run_link(make_tx(k=7, nv=8, lut=512), bbb.FIR(MA), 2, 0, 1000)
    assert e.value.code == _lib.BBB_EUNSUP
    quiet = make_tx(k=7, noise_en=0, lut=512)
    assert np.array_equal(run_link(quiet, bbb.FIR([1]), 0, 0, 5000)[0][0], u64(quiet.eye(5000)[1]))


# ---- 10. the C++ example ---------------------------------------------------------------------------------------------

def test_example_link(gpu):
    exe = ROOT / "examples" / "bbb_mc"
    n = 1_000_003
    r = subprocess.run([str(exe), "--link", "1", "--eye-samples", str(n), "--prbs", "7", "--nv", "15", "--shape", "16", "--delay", "2"],
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    head, rows = lines[0], lines[1:]
    assert head["mode"] == "link" and head["taps"] == MA and head["delay"] == 2
    tx = make_tx(k=7, nv=15, shape=16)
    raw = u64(tx.eye(n)[1])
    flt = run_link(make_tx(k=7, nv=15, shape=16), bbb.FIR.moving_average(), 2, 0, n)[0][0]
    want = [(p, int(raw[p, 0]), int(raw[p, 1]), int(flt[p, 0]), int(flt[p, 1])) for p in range(8)]
    assert [(d["phase"], d["bits"], d["raw_errors"], d["filtered_bits"], d["filtered_errors"]) for d in rows] == want
