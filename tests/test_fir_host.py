"""The FIR filter on the host (no GPU): the numpy model (tests/fir_model.py) against np.convolve, the clocked restatement
of the reference's MovingAverage against its tap form and against the expectation of the module's own test, the presets of
bbb_fir_moving_average, every rejected bbb_fir_cfg, FIR.matched, and the phase arithmetic of a record handed over in pieces."""
import ctypes as C

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib, fir
from basebandboard_amd.bitshaper import rcf_coefficients
import fir_model as M


def cfg(taps=(1,), shift=0, decim=1, phase=0, out_bytes=2, ntaps=None):
    c = _lib.FirCfg()
    c.ntaps = len(taps) if ntaps is None else ntaps
    for i, v in enumerate(taps):
        c.taps[i] = int(v)
    c.shift, c.decim, c.phase, c.out_bytes = shift, decim, phase, out_bytes
    return c


def test_model_against_convolve():
    rng = np.random.default_rng(1)
    for ntaps in (1, 2, 3, 7, 64, 255, 256):
        h = rng.integers(-200, 201, ntaps)
        x = rng.integers(-32768, 32768, 1000)
        full = np.convolve(x.astype(np.int64), h.astype(np.int64))
        assert np.array_equal(M.acc(x, h), full[:len(x)])
        # history: the tail of a longer record equals the record's own tail
        for nb in (0, 1, ntaps - 1, ntaps + 5):
            nb = max(nb, 0)
            want = full[300:len(x)] if nb >= ntaps - 1 else np.convolve(x[300 - nb:].astype(np.int64), h)[nb:len(x) - 300 + nb]
            assert np.array_equal(M.acc(x[300:], h, before=x[300 - nb:300]), want), (ntaps, nb)
        for decim, phase in ((1, 0), (2, 1), (3, 2), (7, 0), (256, 255)):
            for shift in (0, 3):
                y = M.filt(x, h, shift, decim, phase, out_bytes=4)
                assert np.array_equal(y, (full[:len(x)] >> shift)[phase::decim])
                assert len(y) == M.nout(len(x), decim, phase) == fir.nout(len(x), decim, phase)
    for ntaps in (1, 64, 256):
        h = rng.integers(-255, 256, ntaps)
        h[0] = 65535 - np.abs(h[1:]).sum() if ntaps > 1 else -32768             # at the sum limit
        x = rng.integers(-32768, 32768, 20_000)
        x[:300] = -32768
        assert np.array_equal(M.acc_fast(x, h), M.acc(x, h))
    assert M.nout(5, 8, 5) == 0 and M.nout(5, 8, 4) == 1 and M.nout(0, 1, 0) == 0


def test_model_saturations_and_slice():
    x = np.array([-32768] * 8 + [32767] * 8, dtype=np.int16)
    y = M.filt(x, [32767, 32767], out_bytes=2)
    assert y.dtype == np.int16 and y.min() == -32768 and y.max() == 32767
    y32 = M.filt(x, [32767, 32768 - 1, 1], out_bytes=4)
    assert y32.dtype == np.int32 and y32.min() == -65535 * 32768
    rng = np.random.default_rng(2)
    x = rng.integers(-100, 101, 1000)
    w, nbits = M.slice_packed(x, [1, 1, 1, 1], stride=4, phase=3, threshold=0, strict=True)
    assert nbits == 250 and len(w) == 4 and w.dtype == np.uint64
    bits = np.unpackbits(w.view(np.uint8), bitorder="little")
    run = np.convolve(x, [1, 1, 1, 1])[:1000]
    assert np.array_equal(bits[:250], (run[3::4] > 0)) and not bits[250:].any()
    # >= and > differ exactly where acc == threshold
    a, b = M.decisions(x, [1, 1], threshold=5), M.decisions(x, [1, 1], threshold=5, strict=True)
    assert np.array_equal(a != b, M.acc(x, [1, 1]) == 5) and (a != b).any()


def test_clocked_moving_average_is_the_seven_tap_filter():
    rng = np.random.default_rng(3)
    wave = rng.integers(-2048, 2047, 100)                             # the module's own stimulus (average.py:42)
    out = M.moving_average_clocked(wave)
    assert np.array_equal(out, M.acc(wave, [0, 0, 0, 1, 1, 1, 1]))     # x(t) = s(t-3) + s(t-4) + s(t-5) + s(t-6), no shift
    assert np.array_equal(out, M.filt(wave, [0, 0, 0, 1, 1, 1, 1], shift=0, out_bytes=4))
    # the test's expectation (average.py:50-54), index for index, is the same filter at shift 2
    assert np.array_equal((out >> 2)[6:], M.moving_average_expected(wave))
    assert np.array_equal(M.filt(wave, [0, 0, 0, 1, 1, 1, 1], shift=2, out_bytes=4)[6:], M.moving_average_expected(wave))
    assert not np.array_equal(out[6:], M.moving_average_expected(wave))        # the module itself does not shift
    # without the pipeline it is the running sum of adcplot.py:34
    assert np.array_equal(M.acc(wave, [1, 1, 1, 1])[:-3], out[3:])


def test_moving_average_presets():
    lib = _lib.lib()
    c = cfg(taps=[5] * 256, shift=9, decim=7, phase=3, out_bytes=4)
    assert lib.bbb_fir_moving_average(C.byref(c), 0) == _lib.BBB_OK
    assert (c.ntaps, list(c.taps[:8]), c.shift, c.decim, c.phase, c.out_bytes) == (4, [1, 1, 1, 1, 0, 0, 0, 0], 0, 1, 0, 2)
    assert lib.bbb_fir_moving_average(C.byref(c), 1) == _lib.BBB_OK
    assert (c.ntaps, list(c.taps[:8]), c.shift, c.decim, c.phase, c.out_bytes) == (7, [0, 0, 0, 1, 1, 1, 1, 0], 0, 1, 0, 2)
    assert not any(c.taps[8:])
    assert lib.bbb_fir_moving_average(None, 0) == _lib.BBB_EINVAL
    assert bbb.FIR.moving_average().taps == [1, 1, 1, 1] and bbb.FIR.moving_average().shift == 0
    f = bbb.FIR.moving_average(pipeline=True, shift=2)
    assert f.taps == [0, 0, 0, 1, 1, 1, 1] and f.shift == 2 and len(f) == 7


BAD = {
    "ntaps 0": dict(ntaps=0),
    "ntaps 257": dict(ntaps=257),
    "tap sum 65536": dict(taps=[32767, -32767, 2]),
    "tap sum 65536, one tap -32768": dict(taps=[-32768, 32767, 1]),
    "decim 0": dict(decim=0),
    "decim 257": dict(decim=257),
    "phase == decim": dict(decim=4, phase=4),
    "shift 32": dict(shift=32),
    "out_bytes 3": dict(out_bytes=3),
}


@pytest.mark.parametrize("name", list(BAD))
def test_rejected_cfg_is_einval_without_a_device(name):
    """The cfg is checked before anything else: the pointers are not valid device memory and device 99 does not exist."""
    lib = _lib.lib()
    c = cfg(**BAD[name])
    n = C.c_uint64(77)
    assert lib.bbb_fir_filter(C.c_void_p(4096), 100, 0, C.byref(c), C.c_void_p(1 << 20), C.byref(n), 99, None) == _lib.BBB_EINVAL, name
    assert lib.bbb_last_error_detail() and n.value == 77
    if name not in ("shift 32", "out_bytes 3"):                     # the slicer ignores these two
        assert lib.bbb_fir_slice(C.c_void_p(4096), 100, 0, C.byref(c), 0, 0, C.c_void_p(1 << 20), None, 99, None) == _lib.BBB_EINVAL, name


def test_argument_checks_come_before_the_device():
    lib = _lib.lib()
    ok = cfg(taps=[32767, -32767, 1])                                 # the sum limit itself is accepted
    n = C.c_uint64(77)
    assert lib.bbb_fir_filter(None, 0, 0, C.byref(ok), None, C.byref(n), 99, None) == _lib.BBB_OK and n.value == 0     # nin = 0: a no-op
    assert lib.bbb_fir_filter(C.c_void_p(4096), 3, 0, C.byref(cfg(decim=8, phase=5)), None, C.byref(n), 99, None) == _lib.BBB_OK and n.value == 0
    assert lib.bbb_fir_filter(None, 10, 0, None, None, None, 99, None) == _lib.BBB_EINVAL
    assert lib.bbb_fir_filter(None, 10, 0, C.byref(ok), C.c_void_p(1 << 20), None, 99, None) == _lib.BBB_EINVAL
    assert lib.bbb_fir_filter(C.c_void_p(4096), 10, 0, C.byref(ok), None, None, 99, None) == _lib.BBB_EINVAL
    assert lib.bbb_fir_filter(C.c_void_p(4097), 10, 0, C.byref(ok), C.c_void_p(1 << 20), None, 99, None) == _lib.BBB_EINVAL
    assert lib.bbb_fir_filter(C.c_void_p(4096), 10, 0, C.byref(cfg(out_bytes=4)), C.c_void_p((1 << 20) + 2), None, 99, None) == _lib.BBB_EINVAL
    assert lib.bbb_fir_slice(C.c_void_p(4096), 10, 0, C.byref(ok), 0, 0, C.c_void_p((1 << 20) + 4), None, 99, None) == _lib.BBB_EINVAL
    # an output that overlaps the samples read, history included
    assert lib.bbb_fir_filter(C.c_void_p(4096), 100, 0, C.byref(ok), C.c_void_p(4096 + 198), None, 99, None) == _lib.BBB_EINVAL
    assert b"overlaps" in lib.bbb_last_error_detail()
    assert lib.bbb_fir_filter(C.c_void_p(4096), 100, 2, C.byref(ok), C.c_void_p(4096 - 4 - 200 + 2), None, 99, None) == _lib.BBB_EINVAL
    assert lib.bbb_fir_slice(C.c_void_p(4096), 100, 0, C.byref(ok), 0, 0, C.c_void_p(4096 + 192), None, 99, None) == _lib.BBB_EINVAL
    # everything in order: only now the device is asked for, and there is no device 99
    for rc in (lib.bbb_fir_filter(C.c_void_p(4096), 100, 2, C.byref(ok), C.c_void_p(4096 - 4 - 200), C.byref(n), 99, None),
               lib.bbb_fir_slice(C.c_void_p(4096), 100, 0, C.byref(ok), 0, 1, C.c_void_p(4096 + 200), None, 99, None)):
        assert rc in (_lib.BBB_ENODEV, _lib.BBB_EINVAL) and rc != _lib.BBB_OK
    assert b"overlaps" not in lib.bbb_last_error_detail()
    assert n.value == 100


def test_python_class_checks():
    with pytest.raises(ValueError):
        bbb.FIR([])
    with pytest.raises(ValueError):
        bbb.FIR([1] * 257)
    with pytest.raises(ValueError):
        bbb.FIR([32767, 32767, 2])
    with pytest.raises(ValueError):
        bbb.FIR([40000])
    with pytest.raises(ValueError):
        bbb.FIR([1], shift=32)
    f = bbb.FIR([32767, -32768])
    for kw in (dict(decim=0), dict(decim=257), dict(decim=4, phase=4), dict(decim=4, phase=-1)):
        with pytest.raises(ValueError):
            f._cfg(**{"decim": 1, "phase": 0, **kw})
    with pytest.raises(ValueError):
        f.stream(decim=3, phase=3)
    import torch
    with pytest.raises(ValueError):
        f.filter(torch.zeros(8, dtype=torch.int16))                 # not on the GPU


def test_matched_reverses_a_shaper_set():
    for beta in (0.0, 0.35, 1.0):
        c = rcf_coefficients(beta)
        m = bbb.FIR.matched(c)
        assert m.taps == c[::-1] and len(m) == 64
        assert 1834 <= sum(abs(v) for v in c) <= 3474
    rect = [0] * 30 + [254] * 4 + [0] * 30
    assert bbb.FIR.matched(rect, shift=3).taps == rect[::-1] and bbb.FIR.matched(rect, shift=3).shift == 3
    # the response of a set to itself peaks at its energy, at lag 63
    c = np.array(rcf_coefficients(0.5), dtype=np.int64)
    r = M.acc(np.concatenate([c, np.zeros(64, dtype=np.int64)]), bbb.FIR.matched(c).taps)
    assert r.argmax() == 63 and r[63] == (c * c).sum()


@pytest.mark.parametrize("decim", [1, 2, 3, 4, 16, 256])
def test_stream_phase_arithmetic(decim):
    """Pieces of any length, each filtered at the carried phase with ntaps - 1 samples of history, give the outputs of one call."""
    rng = np.random.default_rng(decim)
    x = rng.integers(-32768, 32768, 3000)
    h = rng.integers(-100, 101, 9)
    for phase in {0, 1 % decim, decim - 1}:
        whole = M.filt(x, h, 2, decim, phase)
        for _ in range(4):
            cuts = sorted(set(rng.integers(0, len(x) + 1, 7).tolist()))
            assert np.array_equal(M.stream(x, h, cuts, 2, decim, phase), whole), (phase, cuts)
        assert np.array_equal(M.stream(x, h, list(range(1, 40)), 2, decim, phase), whole)    # pieces shorter than the filter
    for p in range(decim if decim <= 16 else 3):
        for n in (0, 1, decim - 1, decim, decim + 1, 1000):
            q = fir.next_phase(p, decim, n)
            assert q == M.next_phase(p, decim, n) and 0 <= q < decim
            # the next output after the chunk's own sits at chunk index p + nout * decim = n + q
            assert p + fir.nout(n, decim, p) * decim == n + q
