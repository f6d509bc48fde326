"""The numerically controlled oscillator on the host (no GPU): the ROM against numpy's formula and the golden file, the
clock-by-clock register model of gateware/bbb/nco.py against the closed form the kernels compute, the reference's own
test_nco assertion, and the argument checks of the C ABI and of basebandboard_amd.NCO."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from conftest import GOLDEN
import nco_model as M


def test_rom_matches_numpy_and_golden():
    rom = bbb.NCO.rom_table()
    assert rom.dtype == np.int16 and rom.shape == (1024,)
    assert np.array_equal(rom, M.rom())
    golden = json.load(open(GOLDEN / "nco_rom.json"))
    assert golden["rom"] == rom.tolist()
    # the quirks the restatement keeps: period 1023 steps, odd about the middle, full int16 range less one
    assert rom[0] == rom[1023] == 0
    assert np.array_equal(rom[::-1], -rom)
    assert rom.max() == 32767 and rom.min() == -32767
    # no entry is near a half-integer, so a C double sin + nearbyint rebuild rounds as numpy does
    v = np.sin(np.linspace(0, 2 * np.pi, 1024)) * 32767
    assert np.min(np.abs(np.abs(v - np.floor(v)) - 0.5)) > 0.001
    assert all(int(rom[i]) == round(32767 * math.sin(2 * math.pi * i / 1023)) for i in range(1023))


def test_reference_known_answer_on_the_model():
    """nco.py:47-66: fcw = 2^14, am = 2^16 - 1, 1024 clocks; values[3:] == expected[:-3]."""
    x, _ = M.clock(1024, 2 ** 14, am=2 ** 16 - 1)
    expected = (np.round(np.sin(np.linspace(0, 2 * np.pi, 1024)) * (2 ** 15 - 1)).astype(np.int64) * (2 ** 16 - 1)) >> 16
    assert x[3:].tolist() == expected.tolist()[:-3]
    assert x[:3].tolist() == [0, 0, 0]


def _inputs(rng, n, use):
    fm = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32) if "fm" in use else int(rng.integers(-2 ** 23, 2 ** 23))
    am = rng.integers(0, 2 ** 16, n).astype(np.uint16) if "am" in use else int(rng.integers(0, 2 ** 16))
    pm = rng.integers(-512, 512, n).astype(np.int16) if "pm" in use else int(rng.integers(-512, 512))
    if "am" in use and n > 2:
        am[:2] = (0, 65535)
    return fm, am, pm


COMBOS = [tuple(u for u, b in zip(("fm", "am", "pm"), bits) if b) for bits in np.ndindex(2, 2, 2)]


@pytest.mark.parametrize("use", COMBOS, ids=lambda u: "+".join(u) or "const")
def test_clock_model_equals_closed_form(use):
    rng = np.random.default_rng(sum((i + 1) * ord(c) for i, c in enumerate("".join(use))))
    for n in (0, 1, 2, 3, 4, 5, 17, 300):
        fcw = int(rng.integers(0, 2 ** 24))
        fm, am, pm = _inputs(rng, n, use)
        for st in ((0, 0, 0, 0), (int(rng.integers(0, 2 ** 24)), int(rng.integers(-32768, 32768)),
                                  int(rng.integers(-32768, 32768)), int(rng.integers(-2 ** 31, 2 ** 31)))):
            xa, sa = M.clock(n, fcw, fm, am, pm, st)
            xb, sb = M.closed(n, fcw, fm, am, pm, st)
            assert np.array_equal(xa, xb), (use, n, st)
            assert tuple(sa) == tuple(sb), (use, n, st)


def test_closed_form_split_invariance():
    rng = np.random.default_rng(5)
    n, fcw = 500, 0x5A5A5A
    fm, am, pm = _inputs(rng, n, ("fm", "am", "pm"))
    whole, s_end = M.closed(n, fcw, fm, am, pm)
    for _ in range(20):
        cuts = sorted(set(rng.integers(0, n, 6).tolist()) | {0, n})
        st, parts = (0, 0, 0, 0), []
        for a, b in zip(cuts[:-1], cuts[1:]):
            x, st = M.closed(b - a, fcw, fm[a:b], am[a:b], pm[a:b], st)
            parts.append(x)
        assert np.array_equal(np.concatenate(parts), whole) and st == s_end
    # constant inputs far out, from reset: closed_at equals the closed form over the same range
    x, _ = M.closed(4000, 2 ** 20 + 3, 5, 999, -7)
    assert np.array_equal(M.closed_at(0, 4000, 2 ** 20 + 3, 5, 999, -7), x)
    assert np.array_equal(M.closed_at(2 ** 24 + 1000, 3000, 2 ** 20 + 3, 5, 999, -7), x[1000:])


def test_state_after_equals_model():
    """NCO.state_after (the host arithmetic behind seek) against the clock model; no device needed."""
    o = bbb.NCO.__new__(bbb.NCO)                          # the host half of the object only
    o._cfg = _lib.NcoCfg(0x12345, 40000, -77, 100)
    for t in (0, 1, 2, 3, 4, 1000):
        _, st = M.clock(t, 0x12345, -77, 40000, 100)
        assert tuple(o.state_after(t)) == st
    start = (123456, -300, 20000, -5_000_000)
    for t in (0, 1, 2, 3, 77):
        _, st = M.clock(t, 0x12345, -77, 40000, 100, start)
        assert tuple(o.state_after(t, start)) == st
    # far out: pa wraps mod 2^24, the rest depends on t mod 2^24 only
    T = 2 ** 40 + 5
    s = o.state_after(T)
    assert s.pa == (T * (0x12345 - 77)) % (1 << 24)
    inc = 0x12345 - 77
    r = lambda j: int(M.ROM[((((j * inc) % (1 << 24)) >> 14) + 100) & 1023])    # noqa: E731
    assert (s.q, s.w, s.y) == (r(T - 1), r(T - 2), 40000 * r(T - 3))


def test_cfg_and_width_checks():
    for kw in ({"fcw": 1 << 24}, {"fcw": -1}, {"fcw": 1, "am": 1 << 16}, {"fcw": 1, "am": -1}, {"fcw": 1, "fm": 1 << 23},
               {"fcw": 1, "fm": -(1 << 23) - 1}, {"fcw": 1, "pm": 512}, {"fcw": 1, "pm": -513}, {"fcw": 1.5},
               {"fcw": 1, "n": 32}, {"fcw": 1, "m": 12}, {"fcw": 1, "p": 14}):
        with pytest.raises(ValueError):
            bbb.NCO(**kw)
    lib = _lib.lib()
    o = C.c_void_p()
    for cfg in ((1 << 24, 0, 0, 0), (0, 1 << 16, 0, 0), (0, 0, 1 << 23, 0), (0, 0, -(1 << 23) - 1, 0), (0, 0, 0, 512),
                (0, 0, 0, -513)):
        assert lib.bbb_nco_open(C.byref(_lib.NcoCfg(*cfg)), 0, None, C.byref(o)) == _lib.BBB_EINVAL
    assert lib.bbb_nco_open(None, 0, None, C.byref(o)) == _lib.BBB_EINVAL
    assert lib.bbb_nco_rom(None) == _lib.BBB_EINVAL
    assert lib.bbb_nco_run(None, None, None, None, 1, None) == _lib.BBB_EINVAL
    assert lib.bbb_nco_set_cfg(None, C.byref(_lib.NcoCfg(0, 0, 0, 0))) == _lib.BBB_EINVAL
    assert lib.bbb_nco_get_state(None, C.byref(_lib.NcoState())) == _lib.BBB_EINVAL
    assert lib.bbb_nco_set_state(None, C.byref(_lib.NcoState())) == _lib.BBB_EINVAL
    assert lib.bbb_nco_set_stream(None, None) == _lib.BBB_EINVAL
    assert lib.bbb_nco_close(None) == _lib.BBB_EINVAL
    # the extremes of every range are accepted by the checks (and then need a device)
    for cfg in ((0, 0, -(1 << 23), -512), ((1 << 24) - 1, (1 << 16) - 1, (1 << 23) - 1, 511)):
        rc = lib.bbb_nco_open(C.byref(_lib.NcoCfg(*cfg)), 0, None, C.byref(o))
        assert rc != _lib.BBB_EINVAL
        if rc == _lib.BBB_OK:                              # a GPU is present: give the object back
            assert lib.bbb_nco_close(o) == _lib.BBB_OK


def test_open_without_gpu_is_enodev():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = _lib.lib()
    o = C.c_void_p()
    assert lib.bbb_nco_open(C.byref(_lib.NcoCfg(1 << 20, 1 << 14, 0, 0)), 0, None, C.byref(o)) == _lib.BBB_ENODEV
    with pytest.raises(_lib.BbbError) as e:
        bbb.NCO(1 << 20, 1 << 14)
    assert e.value.code == _lib.BBB_ENODEV
