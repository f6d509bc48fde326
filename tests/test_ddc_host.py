"""The digital down-converter without a GPU: the numpy model (tests/ddc_model.py) against a brute per-output loop and against
the accumulate rule of tests/fir_model.py, its split invariance, every rejected argument of bbb_ddc_run through the C ABI,
bbb_ddc_polar_host against the model's CORDIC, the closed loop NCO model -> DDC model -> bits, and the per-sample arithmetic
(basebandboard_amd/csrc/ddc_common.hpp) as a stand-alone program under ASan/UBSan."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib, ddc
from conftest import ROOT

import ddc_model as M
import fir_model
import nco_model

CORNERS = (-32768, -32767, -1, 0, 1, 32767)


# ---- the model ---------------------------------------------------------------------------------------------------------

def _brute(x, fcw, taps, shift, decim, phase, first, pa0, before, mode):
    """One output at a time, one tap at a time, python integers."""
    rom = [int(v) for v in nco_model.ROM]
    x, before = [int(v) for v in x], [int(v) for v in before]

    def sample(n):
        if n >= 0:
            return x[n]
        return before[len(before) + n] if -n <= len(before) else 0

    def mixed(n):
        j = (first + n) % (1 << 24)
        adr = ((pa0 + j * fcw) % (1 << 24)) >> 14
        return (sample(n) * rom[(adr + 256) % 1024]) >> 15, (sample(n) * -rom[adr]) >> 15

    out = []
    for n in range(phase, len(x), decim):
        ai = sum(int(h) * mixed(n - i)[0] for i, h in enumerate(taps))
        aq = sum(int(h) * mixed(n - i)[1] for i, h in enumerate(taps))
        ai, aq = ai >> shift, aq >> shift
        if mode != M.IQ32:
            ai, aq = max(-32768, min(32767, ai)), max(-32768, min(32767, aq))
        out.append((ai, aq))
    return out


def test_model_equals_the_definition_output_by_output():
    rng = np.random.default_rng(1)
    cases = [(40, 1, 0, 1, 0, 0, 0, 0, 0), (90, 7, 3, 1, 0, 5, 0xABCDEF, 1 << 20, 6), (300, 9, 0, 3, 2, (1 << 24) - 3, 0, 0x5A5A5A, 3),
             (257, 64, 6, 16, 15, (1 << 40) + 1, 0xABCDEF, (1 << 24) - 1, 70), (50, 2, 15, 2, 1, 7, 1, 1, 1), (33, 8, 0, 1, 0, 0, 0, 1 << 14, 7)]
    for n, ntaps, shift, decim, phase, first, pa0, fcw, nb in cases:
        h = rng.integers(-200, 201, ntaps)
        rec = rng.integers(-32768, 32768, n + nb)
        x, before = rec[nb:], rec[:nb]
        for mode in (M.IQ16, M.IQ32):
            got = M.ddc(x, fcw, h, shift, decim, phase, first, pa0, before, mode)
            want = _brute(x, fcw, h, shift, decim, phase, first, pa0, before, mode)
            assert got.tolist() == [list(p) for p in want], (n, ntaps, decim, mode)
        # the history rule: samples beyond the nearest ntaps - 1 do not count, missing ones are 0
        assert np.array_equal(M.ddc(x, fcw, h, shift, decim, phase, first, pa0, before),
                              M.ddc(x, fcw, h, shift, decim, phase, first, pa0, before[max(0, nb - (ntaps - 1)):]))
    # mi and mq stay inside [-32767, 32767] at the corners of x and the ROM
    x = np.array([-32768, -32768, 32767, 32767])
    for fcw in (0, 1 << 22, 3 << 22):                                         # adr 0 / 256 / 768: c, s = 32767, 0 / 0, 32767 / 0, -32767
        mi, mq = M.mix(x, 1, fcw, 0)
        assert max(np.abs(mi).max(), np.abs(mq).max()) <= 32767


def test_model_accumulates_as_the_fir_model_does():
    rng = np.random.default_rng(2)
    for ntaps in (1, 2, 7, 64, 256):
        h = rng.integers(-255, 256, ntaps)
        h[0] = 65535 - np.abs(h[1:]).sum() if ntaps > 1 else -32768             # at the sum limit
        m = rng.integers(-32767, 32768, 3000)
        for nb in (0, 1, ntaps - 1, ntaps + 5):
            assert np.array_equal(M.acc(m[nb:], h, m[:nb]), fir_model.acc(m[nb:], h, m[:nb])), (ntaps, nb)
    assert M.nout(5, 8, 5) == fir_model.nout(5, 8, 5) == 0 and M.nout(100, 3, 2) == fir_model.nout(100, 3, 2)


def test_model_split_invariance():
    rng = np.random.default_rng(3)
    x = rng.integers(-32768, 32768, 5000)
    h = rng.integers(-100, 101, 33)
    for decim, phase, first in ((1, 0, 0), (3, 2, (1 << 24) - 1000), (16, 5, (1 << 40) + 1), (256, 255, 12345)):
        for mode in (M.IQ16, M.IQ32, M.POLAR):
            whole = M.ddc(x, 0x5A5A5A, h, 4, decim, phase, first, 0xABCDEF, mode=mode)
            for cuts in ([1], [2047, 2048], [1, 2, 3, 40, 4999], sorted(set(rng.integers(0, 5001, 6).tolist()))):
                assert np.array_equal(M.stream(x, 0x5A5A5A, h, cuts, 4, decim, phase, first, 0xABCDEF, mode), whole), (decim, mode, cuts)


# ---- the C ABI's checks ------------------------------------------------------------------------------------------------

def _fir(taps=(1,), shift=0, decim=1, phase=0, out_bytes=0, ntaps=None):
    c = _lib.FirCfg()
    c.ntaps = len(taps) if ntaps is None else ntaps
    for i, v in enumerate(taps):
        c.taps[i] = int(v)
    c.shift, c.decim, c.phase, c.out_bytes = shift, decim, phase, out_bytes
    return c


def _run(in_dev=4096, nin=100, nbefore=0, first=0, fcw=1 << 20, pa0=0, mode=_lib.DDC_IQ16, fir="default", out=1 << 20, ddc_cfg="default",
         nout=None, device=99):
    lib = _lib.lib()
    f = _fir() if fir == "default" else fir
    d = _lib.DdcCfg(fcw, pa0, mode) if ddc_cfg == "default" else ddc_cfg
    rc = lib.bbb_ddc_run(C.c_void_p(in_dev), nin, nbefore, first, C.byref(d) if d is not None else None,
                         C.byref(f) if f is not None else None, C.c_void_p(out), C.byref(nout) if nout is not None else None, device, None)
    return rc, lib.bbb_last_error_detail().decode()


BAD = {
    "null ddc cfg": (dict(ddc_cfg=None), "null ddc cfg"),
    "null fir cfg": (dict(fir=None), "null fir cfg"),
    "null in_dev": (dict(in_dev=None), "null in_dev"),
    "null out_dev": (dict(out=None), "null out_dev"),
    "fcw 2^24": (dict(fcw=1 << 24), "fcw"),
    "pa0 2^24": (dict(pa0=1 << 24), "pa0"),
    "mode 3": (dict(mode=3), "mode"),
    "ntaps 0": (dict(fir=_fir(ntaps=0)), "ntaps"),
    "ntaps 257": (dict(fir=_fir(ntaps=257)), "ntaps"),
    "tap sum 65536": (dict(fir=_fir(taps=[32767, -32767, 2])), "sum"),
    "decim 0": (dict(fir=_fir(decim=0)), "decim"),
    "decim 257": (dict(fir=_fir(decim=257)), "decim"),
    "phase == decim": (dict(fir=_fir(decim=4, phase=4)), "phase"),
    "shift 32": (dict(fir=_fir(shift=32)), "shift"),
    "first_sample + nin over 2^58": (dict(first=(1 << 58) - 99), "2^58"),
    "first_sample over 2^58": (dict(first=(1 << 58) + 1, nin=0), "2^58"),
    "misaligned in_dev": (dict(in_dev=4097), "misaligned"),
    "misaligned out_dev, IQ16": (dict(out=(1 << 20) + 2), "misaligned"),
    "misaligned out_dev, POLAR": (dict(out=(1 << 20) + 2, mode=_lib.DDC_POLAR), "misaligned"),
    "misaligned out_dev, IQ32": (dict(out=(1 << 20) + 4, mode=_lib.DDC_IQ32), "misaligned"),
    "out_dev overlaps the last sample": (dict(out=4096 + 196), "overlaps"),
    "out_dev overlaps the history": (dict(out=4096 - 4 - 400 + 4, nbefore=2, fir=_fir(taps=[1, 1, 1])), "overlaps"),
    "out_dev overlaps, IQ32": (dict(out=4096 - 800 + 8, mode=_lib.DDC_IQ32), "overlaps"),
}


@pytest.mark.parametrize("name", list(BAD))
def test_rejected_arguments_are_einval_without_a_device(name):
    """Checked before the device is touched: the pointers are not device memory and device 99 does not exist."""
    kw, what = BAD[name]
    n = C.c_uint64(77)
    rc, detail = _run(nout=n, **kw)
    assert rc == _lib.BBB_EINVAL and what in detail, (name, rc, detail)
    assert n.value == 77


def test_valid_calls_reach_the_device_and_nothing_to_do_is_ok():
    n = C.c_uint64(77)
    # nin = 0, and a phase beyond the record: no-ops with nout = 0, whatever the pointers and the device
    assert _run(in_dev=None, nin=0, out=None, nout=n)[0] == _lib.BBB_OK and n.value == 0
    n.value = 77
    assert _run(nin=3, fir=_fir(decim=8, phase=5), out=None, nout=n)[0] == _lib.BBB_OK and n.value == 0
    # everything in order, at the limits of every check: only now the device is asked for, and there is no device 99
    ok = [dict(), dict(fcw=(1 << 24) - 1, pa0=(1 << 24) - 1, mode=_lib.DDC_POLAR), dict(first=(1 << 58) - 100),
          dict(fir=_fir(taps=[32767, -32767, 1], shift=31, decim=16, phase=15, out_bytes=3)),          # out_bytes is ignored
          dict(out=4096 + 200), dict(out=4096 - 400), dict(out=4096 - 4 - 400, nbefore=7, fir=_fir(taps=[1, 1, 1])),
          dict(out=4096 - 800, mode=_lib.DDC_IQ32), dict(out=(1 << 20) + 4), dict(in_dev=4098)]
    for kw in ok:
        n.value = 77
        rc, detail = _run(nout=n, **kw)
        assert rc == _lib.BBB_ENODEV, (kw, rc, detail)
        assert n.value == M.nout(100, kw["fir"].decim, kw["fir"].phase) if "fir" in kw else n.value == 100
    import torch
    if not torch.cuda.is_available():
        assert _run(device=0)[0] == _lib.BBB_ENODEV


def test_python_class_checks():
    f = bbb.FIR([1, 2, 3], shift=2)
    d = bbb.DDC(1 << 20, f, decim=4, phase=3, pa0=5)
    assert (d.fir is f, d.decim, d.phase, d.fcw, d.pa0, d.device) == (True, 4, 3, 1 << 20, 5, 0)
    assert bbb.DDC(0, [1] * 64, shift=6).fir.shift == 6
    for kw in (dict(fcw=1 << 24), dict(fcw=-1), dict(pa0=1 << 24), dict(decim=0), dict(decim=257), dict(decim=4, phase=4), dict(taps=[]),
               dict(taps=[32767, 32767, 2]), dict(shift=32)):
        with pytest.raises(ValueError):
            bbb.DDC(**{"fcw": 1, "taps": [1], **kw})
    import torch
    with pytest.raises(ValueError):
        d.iq(torch.zeros(8, dtype=torch.int16))                     # not on the GPU
    with pytest.raises(ValueError):
        d.stream(out_dtype=torch.int8)
    s = d.stream(first_sample=9)
    assert (s.phase, s.first_sample, s.keep, s.lead, s.have) == (3, 9, 2, 8, 0)
    assert bbb.DDCStream is ddc.DDCStream and callable(bbb.RX.downconvert) and callable(bbb.NCO.ddc)


# ---- the CORDIC --------------------------------------------------------------------------------------------------------

def test_polar_host_equals_the_model_and_is_accurate():
    rng = np.random.default_rng(4)
    pairs = [(i, q) for i in CORNERS for q in CORNERS]
    pairs += [(0, 5), (5, 0), (0, -5), (-5, 0), (3, 4), (-3, 4), (-3, -4), (3, -4), (1, 1), (-1, -1)]
    pairs += rng.integers(-32768, 32768, (3000, 2)).tolist() + rng.integers(-20, 21, (500, 2)).tolist()
    i, q = np.array(pairs).T
    mag, ph = M.cordic(i, q)
    got = np.array([ddc.polar_host(a, b) for a, b in pairs])
    assert np.array_equal(got[:, 0], mag) and np.array_equal(got[:, 1], ph)
    # what bbb.h says of it: mag within 0.59 of hypot, phase within 1 unit of atan2 (modulo a turn), (0, 0) -> (0, 0)
    nz = (i != 0) | (q != 0)
    assert np.abs(mag[nz] - np.hypot(i[nz], q[nz])).max() <= 0.59 and mag.max() == 46341
    turn = np.arctan2(q[nz], i[nz]) / (2 * math.pi) * 65536
    err = (ph[nz] - turn + 32768) % 65536 - 32768
    assert np.abs(err).max() <= 1.0
    assert ddc.polar_host(0, 0) == (0, 0) and ddc.polar_host(1, 0) == (1, 0) and ddc.polar_host(0, 1) == (1, 16384)
    assert ddc.polar_host(-1, 0) == (1, -32768) and ddc.polar_host(0, -1) == (1, -16384)
    lib = _lib.lib()
    assert lib.bbb_ddc_polar_host(1, 1, None, None) == _lib.BBB_EINVAL


# ---- the closed loop: NCO model -> DDC model -> bits -----------------------------------------------------------------------

def test_closed_loop_against_the_clocked_nco_model():
    """A BPSK-like carrier made by the NCO model with pm = -512 (half a turn of the 1024-entry address) for bit 1, taken down
    by the model with the pa0 of NCO.ddc: the sign of Q is the bit, for every bit whose 64 samples lie inside the record.
    A condition, not a tolerance."""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, 512)
    fcw, spb = 1 << 20, 64
    pm = np.repeat(np.where(bits == 1, -512, 0), spb).astype(np.int64)
    x, _ = nco_model.closed(len(pm), fcw, am=0xFFFF, pm=pm)
    xc, _ = nco_model.clock(4096, fcw, am=0xFFFF, pm=pm)
    assert np.array_equal(x[:4096], xc)                              # the closed form is the clocked module
    out = M.ddc(x, fcw, [1] * 64, shift=6, decim=64, phase=66, first=0, pa0=(-3 * fcw) % (1 << 24))
    assert len(out) == 511
    q = out[:, 1].astype(np.int64)
    print("errors", int(((q > 0) != (bits[:511] == 1)).sum()), "min |Q|", int(np.abs(q).min()))
    assert np.array_equal(q > 0, bits[:511] == 1)


# ---- the kernel's arithmetic on the CPU, under the sanitizers --------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("ddc_host")
    exe = d / "ddc_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", str(ROOT / "tests" / "ddc_host.cpp"), "-o", str(exe)])
    return exe


WALK_STRIDE = 1021


def test_cordic_stays_inside_int32_on_a_walk_of_the_pairs(host_exe):
    """Every I with every 1021st Q (the start moving with I: 4.2 million pairs, and the 36 corner pairs), the int32 CORDIC
    beside one on int64 accumulators: equal results, max(|X|, |Y|) < 2^31, mag <= 65535.  All 2^32 pairs take a quarter of an
    hour on one core without the sanitizers (`ddc_host walk 1`); DESIGN.md §21 records that run."""
    r = subprocess.run([str(host_exe), "walk", str(WALK_STRIDE)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    words = r.stdout.split()
    got = dict(zip(words[::2], map(int, words[1::2])))
    print(got)
    assert got["pairs"] >= (1 << 32) // WALK_STRIDE and got["max_xy"] < 1 << 31 and got["max_mag"] <= 65535


def test_mixer_and_cordic_on_the_cpu_equal_the_model(host_exe, tmp_path):
    rng = np.random.default_rng(6)
    i = np.concatenate([np.repeat(CORNERS, 6), rng.integers(-32768, 32768, 20000), rng.integers(-9, 10, 2000)])
    q = np.concatenate([np.tile(CORNERS, 6), rng.integers(-32768, 32768, 20000), rng.integers(-9, 10, 2000)])
    mag, ph = M.cordic(i, q)
    blob = [np.array([len(i)]), np.stack([i, q, mag.astype(np.int64), ph.astype(np.int64)], axis=1).ravel()]
    pa0, fcw, first, n = 0xABCDEF, 0x5A5A5A, (1 << 40) + (1 << 24) - 5000, 20000        # the 2^24 wrap lies inside
    x = rng.integers(-32768, 32768, n)
    x[:8] = [-32768, 32767, -32768, 32767, 0, -1, 1, -32768]
    mi, mq = M.mix(x, first, fcw, pa0)
    blob += [np.array([pa0, fcw, first & 0xFFFFFFFF, n]), nco_model.ROM, np.stack([x, mi, mq], axis=1).ravel()]
    src = tmp_path / "vectors.bin"
    src.write_bytes(np.concatenate(blob).astype(np.uint32).astype("<u4").tobytes())
    r = subprocess.run([str(host_exe), "vectors", str(src)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert r.stdout.split() == ["pairs", str(len(i)), "samples", str(n)]
    # the ROM the library ships is the model's
    assert np.array_equal(bbb.NCO.rom_table(), nco_model.ROM)
