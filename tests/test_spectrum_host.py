"""Autocorrelation and spectrum, host side (no GPU): argument checks of the four entry points and the identities of psd()."""
import ctypes as C

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from basebandboard_amd.bitshaper import _cfg
from basebandboard_amd.spectrum import psd

FAKE = C.c_void_p(1 << 20)          # a non-NULL, aligned pointer that is never dereferenced: every call fails before


def _tx_cfg():
    return _cfg([0] * 32 + [254] + [0] * 31, bbb.PRBS(7, device=-1))


@pytest.mark.parametrize("nlags", [0, 4097, 1 << 31])
def test_bad_nlags_is_einval(nlags):
    lib = _lib.lib()
    assert lib.bbb_acf_accumulate_i16(FAKE, 64, 64, nlags, FAKE, 0, None) == _lib.BBB_EINVAL
    assert b"nlags" in lib.bbb_last_error_detail()
    u = bbb.LUTOPT.shipped(256, device=-1)
    a = C.c_void_p()
    cfg = _tx_cfg()
    assert lib.bbb_tx_acf_open(u._h, C.byref(cfg), nlags, 0, C.byref(a)) == _lib.BBB_EINVAL
    assert b"nlags" in lib.bbb_last_error_detail()
    assert not a.value


def test_capture_argument_checks():
    lib = _lib.lib()
    assert lib.bbb_acf_accumulate_i16(FAKE, 65, 64, 8, FAKE, 0, None) == _lib.BBB_EINVAL
    assert b"navail" in lib.bbb_last_error_detail()
    assert lib.bbb_acf_accumulate_i16(FAKE, 64, 64, 8, None, 0, None) == _lib.BBB_EINVAL
    assert b"acf_dev" in lib.bbb_last_error_detail()
    assert lib.bbb_acf_accumulate_i16(None, 64, 64, 8, FAKE, 0, None) == _lib.BBB_EINVAL
    assert b"samples_dev" in lib.bbb_last_error_detail()
    assert lib.bbb_acf_accumulate_i16(C.c_void_p((1 << 20) + 1), 64, 64, 8, FAKE, 0, None) == _lib.BBB_EINVAL
    assert b"misaligned" in lib.bbb_last_error_detail()
    # device -1 is never a device; nfirst = 0 is a no-op before that
    assert lib.bbb_acf_accumulate_i16(FAKE, 64, 64, 8, FAKE, -1, None) == _lib.BBB_ENODEV
    assert lib.bbb_acf_accumulate_i16(FAKE, 0, 64, 8, FAKE, -1, None) == _lib.BBB_OK
    assert lib.bbb_acf_accumulate_i16(None, 0, 0, 8, FAKE, -1, None) == _lib.BBB_OK


def test_transmitter_argument_checks():
    lib = _lib.lib()
    u = bbb.LUTOPT.shipped(256, device=-1)
    a = C.c_void_p()
    cfg = _tx_cfg()
    assert lib.bbb_tx_acf_open(u._h, C.byref(cfg), 256, (1 << 30) + 1, C.byref(a)) == _lib.BBB_EINVAL
    assert b"chunk_samples" in lib.bbb_last_error_detail()
    cfg.noise_var = 16
    assert lib.bbb_tx_acf_open(u._h, C.byref(cfg), 256, 0, C.byref(a)) == _lib.BBB_EINVAL
    assert b"noise_var" in lib.bbb_last_error_detail()
    cfg = _tx_cfg()
    cfg.prbs_k = 8
    assert lib.bbb_tx_acf_open(u._h, C.byref(cfg), 256, 0, C.byref(a)) == _lib.BBB_EINVAL
    assert b"k=8 invalid for PRBS" in lib.bbb_last_error_detail()
    assert lib.bbb_tx_acf_open(None, C.byref(_tx_cfg()), 256, 0, C.byref(a)) == _lib.BBB_EINVAL
    assert b"null handle" in lib.bbb_last_error_detail()
    assert lib.bbb_tx_acf_open(u._h, C.byref(_tx_cfg()), 256, 0, None) == _lib.BBB_EINVAL
    # valid arguments, a host-only handle: nothing to generate on
    assert lib.bbb_tx_acf_open(u._h, C.byref(_tx_cfg()), 256, 0, C.byref(a)) == _lib.BBB_ENODEV
    assert b"host-only" in lib.bbb_last_error_detail()
    assert not a.value
    assert lib.bbb_tx_acf_run(None, 0, 64, FAKE) == _lib.BBB_EINVAL
    assert b"null acf object" in lib.bbb_last_error_detail()
    assert lib.bbb_tx_acf_close(None) == _lib.BBB_EINVAL
    assert lib.bbb_tx_acf_run(FAKE, 0, 64, None) == _lib.BBB_EINVAL
    assert b"acf_dev" in lib.bbb_last_error_detail()


def np_acf(x, nlags):
    x = np.asarray(x, dtype=np.int64)
    out = np.zeros(nlags + 1, dtype=np.int64)
    for l in range(min(nlags, len(x))):
        out[l] = np.dot(x[:len(x) - l], x[l:])
    out[nlags] = x.sum()
    return out


@pytest.mark.parametrize("n, nfft", [(100, 128), (100, 100), (100, 256), (37, 37), (64, 1000)])
def test_rect_full_lag_is_periodogram(n, nfft):
    """rect window, L = N, navail = nfirst = N, no detrending, two-sided: |rfft(x, nfft)|^2 / N for any nfft >= N"""
    x = np.random.default_rng(n + nfft).integers(-2048, 2048, n)
    f, p = psd(np_acf(x, n), n, window="rect", nfft=nfft, detrend=False, onesided=False)
    ref = np.abs(np.fft.rfft(x.astype(np.float64), nfft)) ** 2 / n
    assert len(p) == nfft
    np.testing.assert_allclose(p[:len(ref)], ref, rtol=1e-9, atol=0)
    np.testing.assert_allclose(f, np.arange(nfft) / nfft, rtol=1e-15, atol=0)


@pytest.mark.parametrize("window", ["rect", "bartlett"])
@pytest.mark.parametrize("detrend", [False, True])
def test_power_is_c0(window, detrend):
    """the two-sided P summed over its nfft bins, divided by nfft, is w[0] c[0]"""
    n, L = 5000, 50
    x = np.random.default_rng(3).integers(-300, 500, n + L)
    acf = np.zeros(L + 1, dtype=np.int64)
    xx = x.astype(np.int64)
    for l in range(L):
        acf[l] = np.dot(xx[:n], xx[l:l + n])
    acf[L] = xx[:n].sum()
    for nfft in (None, 100, 333):
        _, p = psd(acf, n, window=window, nfft=nfft, detrend=detrend, onesided=False)
        mu = acf[L] / n
        c0 = acf[0] / n - (mu * mu if detrend else 0)
        assert abs(p.sum() / len(p) - c0) < 1e-9 * abs(c0)


def test_psd_shape_and_scaling():
    acf = np.array([100, 50, 20, 0], dtype=np.int64)
    f, p = psd(acf, 10, fs=2.0)
    assert len(p) == 5 and len(f) == 5                # L = 3: nfft = 8, one-sided bins 0 .. 4
    f1, p1 = psd(acf, 10, fs=1.0)
    np.testing.assert_allclose(p, p1 / 2.0)
    np.testing.assert_allclose(f, 2 * f1)
    _, pt = psd(acf, 10, onesided=False)
    np.testing.assert_allclose(p1[1:-1], 2 * pt[1:4])
    assert p1[0] == pt[0] and p1[-1] == pt[4]
    with pytest.raises(ValueError):
        psd(acf, 10, window="hann")
    with pytest.raises(ValueError):
        psd(acf, 0)
