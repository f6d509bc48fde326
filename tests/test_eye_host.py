"""Eye diagram and bathtub, host side (no GPU): argument checks of the three entry points, the DSO's persistence image and
the alignment constant of the bathtub against the shaper oracle."""
import ctypes as C
import re

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from basebandboard_amd.bitshaper import _cfg
from basebandboard_amd.eye import EyeConfig, persistence
from conftest import ROOT

FAKE = C.c_void_p(1 << 20)          # a non-NULL, aligned pointer that is never dereferenced: every call fails before


def _tx_cfg():
    return _cfg([0] * 32 + [254] + [0] * 31, bbb.PRBS(7, device=-1))


@pytest.mark.parametrize("bad, what", [(dict(ncols=12), b"ncols"), (dict(shift=16), b"shift")])
def test_bad_eye_cfg_is_einval(bad, what):
    lib = _lib.lib()
    ec = EyeConfig(**bad)._c()
    assert lib.bbb_eye_accumulate_i16(FAKE, 64, 0, C.byref(ec), FAKE, 0, None) == _lib.BBB_EINVAL
    assert what in lib.bbb_last_error_detail()
    u = bbb.LUTOPT.shipped(256, device=-1)
    e = C.c_void_p()
    cfg = _tx_cfg()
    assert lib.bbb_tx_eye_open(u._h, C.byref(cfg), C.byref(ec), 0, C.byref(e)) == _lib.BBB_EINVAL
    assert what in lib.bbb_last_error_detail()
    assert not e.value


def test_null_outputs_are_einval():
    lib = _lib.lib()
    ec = EyeConfig()._c()
    assert lib.bbb_eye_accumulate_i16(FAKE, 64, 0, C.byref(ec), None, 0, None) == _lib.BBB_EINVAL
    assert b"hist_dev" in lib.bbb_last_error_detail()
    assert lib.bbb_tx_eye_run(None, 0, 64, None, None) == _lib.BBB_EINVAL
    assert b"both NULL" in lib.bbb_last_error_detail()
    assert lib.bbb_tx_eye_run(None, 0, 64, FAKE, None) == _lib.BBB_EINVAL         # no object
    assert lib.bbb_tx_eye_close(None) == _lib.BBB_EINVAL
    assert lib.bbb_eye_accumulate_i16(FAKE, 64, 0, None, FAKE, 0, None) == _lib.BBB_EINVAL


def test_tx_cfg_checks_of_open():
    lib = _lib.lib()
    u = bbb.LUTOPT.shipped(256, device=-1)
    ec = EyeConfig()._c()
    e = C.c_void_p()
    cfg = _tx_cfg()
    cfg.noise_var = 16
    assert lib.bbb_tx_eye_open(u._h, C.byref(cfg), C.byref(ec), 0, C.byref(e)) == _lib.BBB_EINVAL
    assert b"noise_var" in lib.bbb_last_error_detail()
    cfg = _tx_cfg()
    cfg.prbs_k = 8
    assert lib.bbb_tx_eye_open(u._h, C.byref(cfg), C.byref(ec), 0, C.byref(e)) == _lib.BBB_EINVAL
    assert b"k=8 invalid for PRBS" in lib.bbb_last_error_detail()
    assert lib.bbb_tx_eye_open(None, C.byref(_tx_cfg()), C.byref(ec), 0, C.byref(e)) == _lib.BBB_EINVAL


def test_compute_without_device_is_enodev():
    """Valid arguments, nothing to compute on: a host-only handle (device -1), and device -1 for the capture side
    (ENODEV whether or not this host has a GPU: -1 is never a device)."""
    lib = _lib.lib()
    ec = EyeConfig()._c()
    assert lib.bbb_eye_accumulate_i16(FAKE, 64, 0, C.byref(ec), FAKE, -1, None) == _lib.BBB_ENODEV
    u = bbb.LUTOPT.shipped(256, device=-1)
    e = C.c_void_p()
    cfg = _tx_cfg()
    assert lib.bbb_tx_eye_open(u._h, C.byref(cfg), C.byref(ec), 0, C.byref(e)) == _lib.BBB_ENODEV
    assert b"host-only" in lib.bbb_last_error_detail()
    assert not e.value
    # nsamples = 0 is a no-op
    assert lib.bbb_eye_accumulate_i16(FAKE, 0, 0, C.byref(ec), FAKE, -1, None) == _lib.BBB_OK


def _np_hist(samples, first, ncols, shift, origin=0):
    x = np.asarray(samples, dtype=np.int64)
    rows = 127 - np.clip(x >> shift, -128, 127)
    cols = (first + np.arange(len(x)) - origin) % ncols
    h = np.zeros((256, ncols), dtype=np.uint64)
    np.add.at(h, (rows, cols), 1)
    return h


def test_persistence_reproduces_the_dso_lines():
    """The reference's DSO test (dso.py:92-111), restated: one line with sample i in column i, then one with -128 + 4 i;
    the memory image (address row << 6 | col) lights exactly those pixels."""
    target = np.zeros((256, 64), dtype=np.uint8)
    h = np.zeros((256, 64), dtype=np.uint64)
    for line in (np.arange(64), -128 + 4 * np.arange(64)):
        for i, v in enumerate(line):
            target[127 - v, i] = 1
        h += _np_hist(line, 0, 64, 0)
    img = persistence(h)
    assert img.dtype == np.uint8 and img.shape == (256, 64)
    assert np.array_equal(img, target)
    flat = img.reshape(-1)
    for i in range(64):
        assert flat[(127 - i) << 6 | i] == 1 and flat[(127 - (-128 + 4 * i)) << 6 | i] == 1
    assert int(flat.sum()) == 128             # no pixel of the two lines coincides
    with pytest.raises(ValueError):
        persistence(np.zeros((64, 256)))


def test_bit_sample0_constant():
    hdr = (ROOT / "include" / "bbb.h").read_text()
    assert re.search(r"#define\s+BBB_TX_BIT_SAMPLE0\s+45\b", hdr)
    assert bbb.BIT_SAMPLE0 == 45


@pytest.mark.parametrize("k", (7, 31))
def test_bit_sample0_derivation_on_the_oracle(oracle, k):
    """With only the centre tap c[32] = 254 and noise off, shaper sample 8m + 49 is +-254 exactly as PRBS bit m: the pulse
    of bit m peaks there, and phase p = 4 of the bathtub (sample 8m + 45 + p) is the pulse centre."""
    c = [0] * 64
    c[32] = 254
    nbits = 600
    x = oracle.shaper(c, k, 8 * nbits + 64)
    bits, _ = oracle.prbs_bits(k, nbits)
    m = np.arange(nbits)
    got = x[8 * m + bbb.BIT_SAMPLE0 + 4]
    assert np.array_equal(got, np.where(bits == 1, 254, -254))
    # and every other sample of the period is 0 (the single tap sits at one phase)
    others = np.delete(x[bbb.BIT_SAMPLE0 + 4:8 * nbits], np.arange(0, 8 * nbits - bbb.BIT_SAMPLE0 - 4, 8))
    assert not others.any()
