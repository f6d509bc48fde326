"""The 16x sinc interpolator on the host (no GPU): the coefficient table against numpy's formula and the golden BRAM words,
the numpy model against the outputs of the reference's own model (tests/golden/sinc_ref.json, written by
tools/make_golden_sinc.py), the no-wrap bound of the module's 16-bit adder tree, split invariance, the sub-sample timing the
interpolated phases recover, and the argument checks of the C ABI and of the Python classes."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from conftest import GOLDEN
import sinc_model as M


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN / "sinc_ref.json"))


def test_coefficients_match_model_and_golden(golden):
    h = bbb.SincInterpolator.coefficients()
    assert h.dtype == np.int8 and h.shape == (128,)
    assert np.array_equal(h, M.coefficients())
    assert np.array_equal(M.unpack(golden["packed"]), h)
    assert bbb.SincInterpolator.packed_coefficients() == golden["packed"]
    assert h.max() == 126 and h.min() == -20
    assert np.array_equal(h, h[::-1])
    # no value is near a truncation boundary, so a C double rebuild truncates as numpy does: the two end values are
    # -4e-16 (0 from either side), every other value is at least 0.0154 from a non-zero integer
    v = np.sinc(np.linspace(-4, 4, 128)) * np.hamming(128) * 127.0
    assert abs(v[0]) < 1e-12 and abs(v[127]) < 1e-12
    r = np.round(v[1:127])
    d = np.abs(v[1:127] - r)
    assert d[r != 0].min() > 0.0154 - 1e-4
    assert np.all(np.abs(v[1:127][r == 0]) < 1 - 0.0154)


def test_model_equals_reference_outputs(golden):
    x = np.array(golden["input"], dtype=np.int64)
    out = np.array(golden["output"], dtype=np.int64)
    assert len(x) == 72 and len(out) == 1106
    assert np.array_equal(x, (np.sin(2 * np.pi * 7 * np.linspace(0, 1, 72)) * 127).astype(np.int8))
    assert np.array_equal(M.batch(x), out[:1024])
    y = M.interpolate(np.concatenate([x, np.zeros(8, dtype=np.int64)]))
    assert np.array_equal(y[M.OFFSET:M.OFFSET + 1106], out)


def _worst_windows():
    """For each phase the window whose signs follow the taps (window[i] = x[m - i]), both polarities."""
    w = []
    for c in range(16):
        taps = M.H[c::16]
        w.append(np.where(taps >= 0, 127, -128))
        w.append(np.where(taps >= 0, -128, 127))
    return np.array(w)


def test_adders_never_wrap():
    sa = np.array([np.abs(M.H[c::16]).sum() for c in range(16)])
    assert sa.max() == 203 and sa.max() * 128 < 32768
    assert sorted({int(M.H[c::16].sum()) for c in range(16)}) == [125, 126]      # the DC gain per phase, of 256
    rng = np.random.default_rng(3)
    wins = np.concatenate([rng.integers(-128, 128, (20000, 8)), _worst_windows(),
                           np.full((1, 8), 127), np.full((1, 8), -128)])
    lo, hi = 0, 0
    for c in range(16):
        plain = (wins * M.H[c::16]).sum(axis=1)
        assert np.array_equal(M.adder_tree(wins, c), plain >> 8), c
        lo, hi = min(lo, int(plain.min())), max(hi, int(plain.max()))
    assert -32768 <= lo and hi <= 32767 and max(-lo, hi) >= 25000
    y = M.interpolate(rng.integers(-128, 128, 5000))
    assert y.min() >= -102 and y.max() <= 101


def test_split_invariance():
    rng = np.random.default_rng(1)
    x = rng.integers(-128, 128, 1000)
    whole = M.interpolate(x)
    for nb in range(8):
        for cut in (1, 7, 8, 333, 999):
            b = M.interpolate(x[cut:], before=x[max(0, cut - nb):cut])
            if nb >= min(cut, 7):
                assert np.array_equal(np.concatenate([M.interpolate(x[:cut]), b]), whole), (nb, cut)
            else:       # too little history: the samples beyond it count as 0
                xz = x.copy()
                xz[:cut - nb] = 0
                assert np.array_equal(b, M.interpolate(xz)[16 * cut:]), (nb, cut)
    x16 = rng.integers(-32768, 32768, 500)
    assert np.array_equal(M.interpolate(x16, shift=4), M.interpolate(np.clip(x16 >> 4, -128, 127)))


def test_interpolated_phase_recovers_subsample_timing():
    """A raised-cosine PRBS-7 capture at 4 samples per bit, taken 0.0 / 0.3 / 0.5 / 0.8 of a sample late: the widest-open of
    the 64 interpolated phases moves by round(16 * offset), within one step, and 50 or more phases decode without error."""
    nb, spb = 4000, 4
    widest = {}
    for frac in (0.0, 0.3, 0.5, 0.8):
        x, bits = M.rc_capture(nb, frac, spb)
        y = M.interpolate(x)
        opening = np.array([np.abs(y[64 * 8 + p::64]).min() for p in range(64)])
        widest[frac] = int(opening.argmax())
        clean = 0
        for p in range(16 * spb):
            d = (y[p::16 * spb] >= 0).astype(np.int64)
            clean += min(int((d[lag:lag + nb - 20] != bits[:len(d[lag:lag + nb - 20])]).sum()) for lag in range(4)) == 0
        assert clean >= 50, (frac, clean)
    print("widest-open phases", widest)
    for frac in (0.3, 0.5, 0.8):
        assert abs(widest[0.0] - widest[frac] - round(16 * frac)) <= 1, widest


def test_c_abi_argument_checks():
    lib = _lib.lib()
    assert lib.bbb_sinc_coefficients(None) == _lib.BBB_EINVAL
    ok = _lib.SincCfg(1, 1, 0)
    p = C.c_void_p(4096)             # never dereferenced: every call below fails its checks before a device is touched
    assert lib.bbb_sinc_interpolate(p, 8, 0, None, p, 0, None) == _lib.BBB_EINVAL
    assert lib.bbb_sinc_interpolate(None, 8, 0, C.byref(ok), p, 0, None) == _lib.BBB_EINVAL
    assert lib.bbb_sinc_interpolate(p, 8, 0, C.byref(ok), None, 0, None) == _lib.BBB_EINVAL
    for cfg in ((0, 1, 0), (3, 1, 0), (4, 1, 0), (1, 0, 0), (1, 3, 0), (2, 2, 16), (1, 1, 1), (1, 2, 15)):
        assert lib.bbb_sinc_interpolate(p, 8, 0, C.byref(_lib.SincCfg(*cfg)), p, 0, None) == _lib.BBB_EINVAL, cfg
    odd = C.c_void_p(4097)
    assert lib.bbb_sinc_interpolate(odd, 8, 0, C.byref(_lib.SincCfg(2, 1, 0)), p, 0, None) == _lib.BBB_EINVAL
    assert lib.bbb_sinc_interpolate(p, 8, 0, C.byref(_lib.SincCfg(1, 2, 0)), odd, 0, None) == _lib.BBB_EINVAL
    # nin = 0 is a no-op whatever the pointers
    assert lib.bbb_sinc_interpolate(None, 0, 0, C.byref(ok), None, 0, None) == _lib.BBB_OK
    eye = _lib.EyeCfg(64, 0, 0, 0, 0)
    o = C.c_void_p()
    assert lib.bbb_sinc_eye_open(None, C.byref(eye), 0, 0, None, C.byref(o)) == _lib.BBB_EINVAL
    assert lib.bbb_sinc_eye_open(C.byref(ok), None, 0, 0, None, C.byref(o)) == _lib.BBB_EINVAL
    assert lib.bbb_sinc_eye_open(C.byref(ok), C.byref(eye), 0, 0, None, None) == _lib.BBB_EINVAL
    assert lib.bbb_sinc_eye_open(C.byref(ok), C.byref(eye), (1 << 27) + 1, 0, None, C.byref(o)) == _lib.BBB_EINVAL
    for cfg in ((0, 2, 0), (3, 2, 0), (2, 2, 16), (1, 2, 1)):
        assert lib.bbb_sinc_eye_open(C.byref(_lib.SincCfg(*cfg)), C.byref(eye), 0, 0, None, C.byref(o)) == _lib.BBB_EINVAL
    for ec in ((12, 0, 0, 0, 0), (128, 0, 0, 0, 0), (64, 16, 0, 0, 0)):
        assert lib.bbb_sinc_eye_open(C.byref(ok), C.byref(_lib.EyeCfg(*ec)), 0, 0, None, C.byref(o)) == _lib.BBB_EINVAL
    assert lib.bbb_sinc_eye_run(None, p, 8, 0, 0, p) == _lib.BBB_EINVAL
    assert lib.bbb_sinc_eye_close(None) == _lib.BBB_EINVAL
    # out_bytes is ignored by the eye object: a value that bbb_sinc_interpolate refuses passes the checks here
    rc = lib.bbb_sinc_eye_open(C.byref(_lib.SincCfg(1, 7, 0)), C.byref(eye), 1024, 0, None, C.byref(o))
    assert rc != _lib.BBB_EINVAL
    if rc == _lib.BBB_OK:                                  # a GPU is present: give the object back
        assert lib.bbb_sinc_eye_run(o, p, 8, 0, 0, None) == _lib.BBB_EINVAL
        assert lib.bbb_sinc_eye_run(o, None, 8, 0, 0, p) == _lib.BBB_EINVAL
        assert lib.bbb_sinc_eye_run(o, p, 8, 0, 1 << 58, p) == _lib.BBB_EINVAL
        assert lib.bbb_sinc_eye_close(o) == _lib.BBB_OK


def test_python_argument_checks():
    s = bbb.SincInterpolator()
    with pytest.raises(ValueError):
        s.interpolate(torch.zeros(8, dtype=torch.int8))                     # not on the GPU
    with pytest.raises(ValueError):
        s.interpolate(np.zeros(8, dtype=np.int8))
    with pytest.raises(ValueError):
        s.eye(torch.zeros(8, dtype=torch.int16))
    for bad in (np.zeros(71, dtype=np.int8), np.zeros(72), np.full(72, 128), torch.zeros(72, dtype=torch.int16),
                torch.zeros(73, dtype=torch.int8)):
        with pytest.raises(ValueError):
            s.run(bad)
    rx = bbb.RX.__new__(bbb.RX)
    rx.samples_per_bit, rx.sample_delay, rx.prbs_k = 4, 0, 7
    for kw in ({}, {"interpolate": True}):
        with pytest.raises(ValueError):
            rx.phase_search(torch.zeros(64, dtype=torch.int16), **kw)       # not on the GPU, either way
        with pytest.raises(ValueError):
            rx.eye(torch.zeros(64, dtype=torch.int16), **kw)


def test_without_gpu_is_enodev():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = _lib.lib()
    p = C.c_void_p(4096)
    for cfg in ((1, 1, 0), (1, 2, 0), (2, 1, 15), (2, 2, 4)):
        assert lib.bbb_sinc_interpolate(p, 8, 7, C.byref(_lib.SincCfg(*cfg)), p, 0, None) == _lib.BBB_ENODEV
    o = C.c_void_p()
    assert lib.bbb_sinc_eye_open(C.byref(_lib.SincCfg(2, 2, 4)), C.byref(_lib.EyeCfg(64, 0, 0, 0, 0)), 0, 0, None,
                                 C.byref(o)) == _lib.BBB_ENODEV
    # the table needs no device
    h = np.zeros(128, dtype=np.int8)
    assert lib.bbb_sinc_coefficients(h.ctypes.data_as(C.c_void_p)) == _lib.BBB_OK and h[63] == 126
