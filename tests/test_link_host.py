"""The filtered link, host side (no GPU): FIR.delay(), the argument checks of bbb_link_sweep_open through the C ABI, the
numpy model of tests/link_model.py against plain restatements, and the finding that motivates the feature -- on the CPU
oracle's waveform a four-tap moving average in front of the decision takes the bathtub's minimum down by more than ten."""
import ctypes as C

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from basebandboard_amd.bitshaper import _cfg, rcf_coefficients

import fir_model
import link_model


# ---- FIR.delay -------------------------------------------------------------------------------------------------------

def test_fir_delay():
    assert bbb.FIR.moving_average().delay() == 1                              # centroid 1.5
    assert bbb.FIR.moving_average(pipeline=True).delay() == 4                 # centroid 4.5
    assert bbb.FIR([1]).delay() == 0 and bbb.FIR([0, 0, 5]).delay() == 2 and bbb.FIR([0, 0]).delay() == 0
    assert bbb.FIR([1, -1]).delay() == 0 and bbb.FIR([1, -3]).delay() == 0 and bbb.FIR([-1, 0, 0, 3]).delay() == 2
    c = rcf_coefficients(0.5)
    w = np.abs(np.array(c[::-1], dtype=np.int64))
    m = bbb.FIR.matched(c)
    assert m.delay() == int((np.arange(64) * w).sum() // w.sum())
    assert m.delay() in (30, 31)                                              # the pulse centre, tap 32, reversed: 31
    assert bbb.LinkSweep is not None


# ---- argument checks -------------------------------------------------------------------------------------------------

def _base():
    return _cfg([0] * 32 + [254] + [0] * 31, bbb.PRBS(7, device=-1))


def _setting(**kw):
    s = _lib.TxSetting()
    for i, v in enumerate(kw.pop("coeffs", rcf_coefficients(0.5))):
        s.coeffs[i] = v
    s.bit_en, s.noise_en, s.noise_var = kw.pop("bit_en", 1), kw.pop("noise_en", 1), kw.pop("noise_var", 8)
    s.threshold, s.strict, s.reserved = kw.pop("threshold", 0), kw.pop("strict", 0), kw.pop("reserved", 0)
    assert not kw
    return s


def _fir(taps=(1, 1, 1, 1), shift=0, decim=1, phase=0, ntaps=None):
    c = _lib.FirCfg()
    c.ntaps = len(taps) if ntaps is None else ntaps
    for i, v in enumerate(taps):
        c.taps[i] = v
    c.shift, c.decim, c.phase, c.out_bytes = shift, decim, phase, 0           # out_bytes is ignored
    return c


def _open(u, settings, nset=None, fir="default", delay=1, eye=None, chunk=0, base="default", out=True):
    lib = _lib.lib()
    arr = (_lib.TxSetting * max(1, len(settings)))(*settings) if settings is not None else None
    h = C.c_void_p()
    b = _base() if base == "default" else base
    f = _fir() if fir == "default" else fir
    rc = lib.bbb_link_sweep_open(u._h if u is not None else None, C.byref(b) if b is not None else None, arr,
                                 len(settings) if nset is None else nset, C.byref(f) if f is not None else None, delay,
                                 C.byref(eye) if eye is not None else None, chunk, C.byref(h) if out else None)
    assert not h.value
    return rc, lib.bbb_last_error_detail()


CASES = [
    ("null_handle", b"null handle"), ("null_out", b"null out"), ("null_base", b"null base"), ("null_settings", b"null settings"),
    ("null_fir", b"null fir"), ("nset0", b"nset"), ("nset513", b"nset"), ("decim2", b"decim"), ("phase1", b"phase"),
    ("delay256", b"delay"), ("sum_taps", b"sum of |taps|"), ("ntaps0", b"ntaps"), ("ntaps257", b"ntaps"), ("fir_shift", b"shift"),
    ("reserved", b"reserved"), ("noise_var16", b"noise_var"), ("coeff_high", b"coefficients"), ("bad_prbs_k", b"k=8 invalid for PRBS"),
    ("eye_ncols", b"ncols"), ("eye_shift", b"eye shift"), ("chunk", b"chunk_samples")]


@pytest.mark.parametrize("case, what", CASES, ids=[c[0] for c in CASES])
def test_bad_arguments_are_einval(case, what):
    """Every argument check comes before the device check: the host-only handle gives BBB_EINVAL, with a detail."""
    u = bbb.LUTOPT.shipped(256, device=-1)
    kw = dict(settings=[_setting(), _setting(noise_var=3)])
    if case == "null_handle":
        u = None
    elif case == "null_out":
        kw["out"] = False
    elif case == "null_base":
        kw["base"] = None
    elif case == "null_settings":
        kw.update(settings=None, nset=2)
    elif case == "null_fir":
        kw["fir"] = None
    elif case == "nset0":
        kw["nset"] = 0
    elif case == "nset513":
        kw["settings"] = [_setting()] * 513
    elif case == "decim2":
        kw["fir"] = _fir(decim=2)
    elif case == "phase1":
        kw["fir"] = _fir(phase=1)
    elif case == "delay256":
        kw["delay"] = 256
    elif case == "sum_taps":
        kw["fir"] = _fir(taps=[32767, 32767, 2])
    elif case == "ntaps0":
        kw["fir"] = _fir(ntaps=0)
    elif case == "ntaps257":
        kw["fir"] = _fir(ntaps=257)
    elif case == "fir_shift":
        kw["fir"] = _fir(shift=32)
    elif case == "reserved":
        kw["settings"] = [_setting(reserved=1)]
    elif case == "noise_var16":
        kw["settings"] = [_setting(), _setting(noise_var=16)]
    elif case == "coeff_high":
        kw["settings"] = [_setting(coeffs=[256] + [0] * 63)]
    elif case == "bad_prbs_k":
        kw["base"] = _base()
        kw["base"].prbs_k = 8
    elif case == "eye_ncols":
        kw["eye"] = _lib.EyeCfg(12, 4, 0, 0, 0)
    elif case == "eye_shift":
        kw["eye"] = _lib.EyeCfg(64, 16, 0, 0, 0)
    elif case == "chunk":
        kw["chunk"] = (1 << 30) + 1
    rc, detail = _open(u, **kw)
    assert rc == _lib.BBB_EINVAL, (case, rc, detail)
    assert what in detail, (case, detail)


def test_valid_open_without_device_is_enodev():
    u = bbb.LUTOPT.shipped(256, device=-1)
    rc, detail = _open(u, [_setting(), _setting(bit_en=0, noise_var=15, threshold=-(1 << 31), strict=1)])
    assert rc == _lib.BBB_ENODEV and b"host-only" in detail
    # the limits: 512 settings, 256 taps with sum |h| = 65535, delay 255, an eye, the largest chunk
    taps = [256, -256] * 127 + [256, -255]
    assert sum(abs(v) for v in taps) == 65535 and len(taps) == 256
    rc, _ = _open(u, [_setting(noise_var=v) for v in range(16)] * 32, fir=_fir(taps=taps, shift=31), delay=255,
                  eye=_lib.EyeCfg(8, 15, 45, 0, 0), chunk=1 << 30)
    assert rc == _lib.BBB_ENODEV
    lib = _lib.lib()
    assert lib.bbb_link_sweep_run(None, 0, 16, C.c_void_p(1 << 20), None) == _lib.BBB_EINVAL
    assert lib.bbb_link_sweep_close(None) == _lib.BBB_EINVAL


def test_python_checks():
    tx_like = type("T", (), {})()
    tx_like.src_sel, tx_like.prbs_shaper = 0, bbb.PRBSShaper(bbb.PRBS(7, device=-1), 0, [[0] * 64])
    with pytest.raises(ValueError):
        bbb.LinkSweep(tx_like, [], bbb.FIR([1]))
    with pytest.raises(ValueError):
        bbb.LinkSweep(tx_like, [bbb.TxSetting()], bbb.FIR([1]), delay=-1)


# ---- the model -------------------------------------------------------------------------------------------------------

def test_model_against_plain_restatements():
    rng = np.random.default_rng(5)
    x = rng.integers(-2048, 2048, 5000)
    xz = lambda j: int(x[j]) if j >= 0 else 0                                  # noqa: E731
    for taps, delay, first, n in (([1], 0, 0, 300), ([1, 1, 1, 1], 2, 0, 300), ([3, -2, 7], 0, 1, 100), ([0, 0, 0, 1, 1, 1, 1], 4, 44, 500),
                                  ([5] * 9, 200, 0, 77), ([1, 2], 1, 3000, 1000)):
        a = link_model.stream_acc(x, 0, first, n, taps, delay)
        want = [sum(h * xz(s + delay - i) for i, h in enumerate(taps)) for s in range(first, first + n)]
        assert a.tolist() == want, (taps, delay, first)
        # a window of the waveform that starts where wave_range says gives the same
        lo, count = link_model.wave_range(first, n, len(taps), delay)
        assert np.array_equal(link_model.stream_acc(x[lo:lo + count], lo, first, n, taps, delay), a)
        # ... and it is the FIR model's acc of the waveform, read `delay` further on
        full = fir_model.acc(x[:first + n + delay], taps)
        assert np.array_equal(full[first + delay:], a)
    # the identity filter: the raw sample's bathtub and histogram
    bits = rng.integers(0, 2, 1000)
    bit_of = lambda lo, cnt: bits[lo:lo + cnt]                                 # noqa: E731
    tub, h = link_model.link(x, 0, 3, 4000, [1], 0, 0, 5, True, bit_of, eye=(16, 4, 45))
    n = 3 + np.arange(4000)
    ok = n >= 45
    m, p = (n[ok] - 45) // 8, (n[ok] - 45) % 8
    err = (x[3:4003][ok] > 5) != bits[m].astype(bool)
    assert tub[:, 0].tolist() == np.bincount(p, minlength=8).tolist()
    assert tub[:, 1].tolist() == np.bincount(p, weights=err, minlength=8).astype(np.int64).tolist()
    want = np.zeros((256, 16), dtype=np.uint64)
    np.add.at(want, (127 - np.clip(x[3:4003] >> 4, -128, 127), (n - 45) % 16), 1)
    assert np.array_equal(h, want) and h.sum() == 4000
    # z saturates to int16 before the eye's shift
    assert link_model.stream_z(np.array([1 << 20, -(1 << 20), 40000, 5]), 1).tolist() == [32767, -32768, 20000, 2]


def test_moving_average_opens_the_bathtub(oracle):
    """PRBS-7, rcf_coefficients(0.5), noise_var 15, samples [0, 2^20): the raw decision's best phase against the decision
    behind taps {1, 1, 1, 1} re-timed by 2 -- both from the oracle's waveform.  The filtered minimum is below a tenth."""
    n, k = 1 << 20, 7
    lut = oracle.Lutopt(path=oracle.data_path(256))
    x = oracle.tx(lut, 1, rcf_coefficients(0.5), k, n + 2, noise_var=15, warmup=16)
    bits = oracle.prbs_bits(k, n // 8 + 2)[0]
    bit_of = lambda lo, cnt: bits[lo:lo + cnt]                                 # noqa: E731
    raw, _ = link_model.link(x, 0, 0, n, [1], 0, 0, 0, False, bit_of)
    flt, _ = link_model.link(x, 0, 0, n, [1, 1, 1, 1], 2, 0, 0, False, bit_of)
    assert np.array_equal(raw[:, 0], flt[:, 0])
    print("raw errors per phase", raw[:, 1].tolist(), "filtered", flt[:, 1].tolist())
    assert int(raw[:, 1].argmin()) == 4 and int(raw[:, 1].min()) == 2491
    assert flt[2:6, 1].tolist() == [177, 3, 6, 191]
    assert 10 * int(flt[:, 1].min()) < int(raw[:, 1].min())
