"""The digital down-converter on the GPU, bit for bit against the numpy model (tests/ddc_model.py): a seeded sample of shapes in
which every listed size, tap count, decimation, history, shift, oscillator setting, sample number and misalignment meets every
kernel variant (three output modes, block and point form), both saturations at the int32 bound, one call against the same
record in pieces (bbb_ddc_run with nbefore / first_sample, and DDCStream), more than one pass of the grid, the polar outputs on
zeros, axes and quadrants, and the closed loop NCO -> DDC on the device."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import basebandboard_amd as bbb
from basebandboard_amd import _lib
import ddc_model as M
import nco_model

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
T = 2048                                           # input samples per workgroup step (kFirTile)
MODES = (M.IQ16, M.IQ32, M.POLAR)
GUARD = 0x5A5A                                     # what the output buffer holds where nothing may be written

NIN = (1, 7, 2047, 2048, 2049, 3 * 2048 + 5)
NTAPS = (1, 2, 7, 8, 9, 64, 255, 256)
DECIM_PHASE = [(d, p) for d in (2, 3, 8, 16, 256) for p in (0, d - 1)]
NBEFORE = ("0", "ntaps-2", "ntaps-1", "ntaps+5")
SHIFT = (0, 15, 31)
FCW = (0, 1, 1 << 14, 1 << 20, 0x5A5A5A, (1 << 24) - 1)
PA0 = (0, 0xABCDEF)
FIRST = (0, (1 << 24) - 3, (1 << 40) + 1)          # the second puts the 2^24 wrap inside the first tile
IN_OFF = (0, 1, 7)                                 # samples between a 16-byte boundary and in_dev
OUT_OFF = (0, 1)                                   # output elements between a 16-byte boundary and out_dev
CASES_PER_VARIANT = 48


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_raw(x, nbefore, in_off, out_off, fcw, pa0, mode, taps, shift, decim, phase, first):
    """bbb_ddc_run on x[nbefore:] with x[:nbefore] in front, in_dev in_off samples and out_dev out_off elements behind a 16-byte
    boundary.  Returns the outputs as the model lays them out; checks that nothing around them was written."""
    nbefore, nin = int(nbefore), len(x) - int(nbefore)
    lead = (-(nbefore) % 8 + in_off) % 8                               # (lead + nbefore) mod 8 = in_off
    buf = torch.zeros(lead + len(x) + 8, dtype=torch.int16, device=DEV)
    buf[lead:lead + len(x)] = dev(np.asarray(x, dtype=np.int16))
    assert (buf.data_ptr() + 2 * (lead + nbefore)) % 16 == 2 * in_off
    n = M.nout(nin, decim, phase)
    dt = torch.int32 if mode == M.IQ32 else torch.int16
    pair = 8 if mode == M.IQ32 else 4
    per16 = 16 // pair
    obuf = torch.full((per16 + out_off + n + 3, 2), GUARD, dtype=dt, device=DEV)
    o0 = per16 + out_off
    assert (obuf.data_ptr() + pair * o0) % 16 == pair * out_off
    f = bbb.FIR(taps, shift=shift)._cfg(decim, phase)
    cfg = _lib.DdcCfg(fcw, pa0, mode)
    got = C.c_uint64()
    _lib.check(_lib.lib().bbb_ddc_run(C.c_void_p(buf.data_ptr() + 2 * (lead + nbefore)), nin, nbefore, first, C.byref(cfg), C.byref(f),
                                      C.c_void_p(obuf.data_ptr() + pair * o0), C.byref(got), 0,
                                      C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "bbb_ddc_run")
    assert got.value == n
    res = obuf.cpu().numpy()
    assert (res[:o0] == GUARD).all() and (res[o0 + n:] == GUARD).all(), "written outside the outputs"
    return res[o0:o0 + n]


def variant_cases(mode, point, seed):
    """CASES_PER_VARIANT shapes of one kernel variant: every list is shuffled on its own and dealt round, so each of its
    values turns up (the lists are shorter than the sample) in combinations that differ from variant to variant."""
    rng = np.random.default_rng(seed)

    def deal(values):
        values = list(values)
        order = [values[i] for i in rng.permutation(len(values))]
        return list(itertools.islice(itertools.cycle(order), CASES_PER_VARIANT))

    cols = dict(nin=deal(NIN), ntaps=deal(NTAPS), dp=deal(DECIM_PHASE if point else [(1, 0)]), nb=deal(NBEFORE), shift=deal(SHIFT),
                fcw=deal(FCW), pa0=deal(PA0), first=deal(FIRST), in_off=deal(IN_OFF), out_off=deal(OUT_OFF))
    cases = [dict(zip(cols, vals)) for vals in zip(*cols.values())]
    for name, values in (("nin", NIN), ("ntaps", NTAPS), ("nb", NBEFORE), ("shift", SHIFT), ("fcw", FCW), ("pa0", PA0), ("first", FIRST),
                         ("in_off", IN_OFF), ("out_off", OUT_OFF), ("dp", DECIM_PHASE if point else [(1, 0)])):
        assert {c[name] for c in cases} == set(values), name
    return cases, rng


@pytest.mark.parametrize("point", (False, True), ids=("block", "point"))
@pytest.mark.parametrize("mode", MODES, ids=("iq16", "iq32", "polar"))
def test_sampled_shapes_equal_the_model(mode, point):
    cases, rng = variant_cases(mode, point, seed=100 * mode + int(point))
    for c in cases:
        ntaps, (decim, phase) = c["ntaps"], c["dp"]
        nb = max(0, {"0": 0, "ntaps-2": ntaps - 2, "ntaps-1": ntaps - 1, "ntaps+5": ntaps + 5}[c["nb"]])
        # taps small enough that a shift of 0 does not saturate everything, large enough that 15 leaves something
        bound = min(32767, 40000 // ntaps)
        h = rng.integers(-bound, bound + 1, ntaps)
        x = rng.integers(-32768, 32768, nb + c["nin"])
        got = run_raw(x, nb, c["in_off"], c["out_off"], c["fcw"], c["pa0"], mode, h.tolist(), c["shift"], decim, phase, c["first"])
        want = M.ddc(x[nb:], c["fcw"], h, c["shift"], decim, phase, c["first"], c["pa0"], before=x[:nb], mode=mode)
        assert got.dtype == want.dtype and np.array_equal(got, want), c


@pytest.mark.parametrize("decim,phase", ((1, 0), (3, 2)))
def test_saturation_and_the_int32_bound(decim, phase):
    """Constant full-scale inputs against the oscillator's peak (fcw = 0: c = rom[256] = 32767 at pa0 = 0, -s = 32767 at
    pa0 = 768 << 14) through taps of one sign with sum |h| = 65535: |ai| or |aq| = 65535 * 32767, 98303 below 2^31."""
    assert nco_model.ROM[256] == 32767 and nco_model.ROM[768] == -32767 and nco_model.ROM[0] == 0
    reached = set()
    for ntaps, x0, pa0, sign in itertools.product((3, 256), (-32768, 32767), (0, 768 << 14), (1, -1)):
        h = np.full(ntaps, 65535 // ntaps)
        h[0] += 65535 - h.sum()
        h = sign * np.minimum(h, 32767)
        h[1] += sign * (65535 - np.abs(h).sum())
        assert np.abs(h).sum() == 65535 and np.abs(h).max() <= 32767
        x = np.full(ntaps + 300, x0)
        for mode, shift in ((M.IQ32, 0), (M.IQ16, 0), (M.IQ16, 15), (M.IQ16, 16), (M.POLAR, 0), (M.IQ32, 31)):
            got = run_raw(x, 0, 0, 0, 0, pa0, mode, h.tolist(), shift, decim, phase, 5)
            want = M.ddc(x, 0, h, shift, decim, phase, 5, pa0, mode=mode)
            assert np.array_equal(got, want), (ntaps, x0, pa0, sign, mode, shift)
            if mode == M.IQ32 and shift == 0:
                reached.add(int(np.abs(got.astype(np.int64)).max()))
            if mode == M.IQ16 and shift == 0:
                reached.update(int(v) for v in (got.min(), got.max()))
    assert 65535 * 32767 in reached and {-32768, 32767} <= reached


@pytest.mark.parametrize("mode", MODES, ids=("iq16", "iq32", "polar"))
@pytest.mark.parametrize("decim,phase,ntaps", ((1, 0, 9), (3, 1, 64), (16, 15, 256)))
def test_one_call_equals_the_record_in_pieces(mode, decim, phase, ntaps):
    rng = np.random.default_rng(7 + ntaps)
    n = 3 * T + 5
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    h = rng.integers(-100, 101, ntaps)
    first, fcw, pa0, shift = (1 << 24) - 2049, 0x5A5A5A, 0xABCDEF, 5
    whole = run_raw(x, 0, 0, 0, fcw, pa0, mode, h.tolist(), shift, decim, phase, first)
    assert np.array_equal(whole, M.ddc(x, fcw, h, shift, decim, phase, first, pa0, mode=mode))
    d = bbb.DDC(fcw, h.tolist(), decim, phase, shift, pa0)
    for cut in (1, 2047, 2048, 4097 + 14):
        # through bbb_ddc_run: the second piece with the first one's last ntaps - 1 samples in front of it
        nb = min(cut, ntaps - 1)
        a = run_raw(x[:cut], 0, 0, 0, fcw, pa0, mode, h.tolist(), shift, decim, phase, first)
        b = run_raw(x[cut - nb:], nb, 1, 1, fcw, pa0, mode, h.tolist(), shift, decim, (phase - cut) % decim, first + cut)
        assert np.array_equal(np.concatenate([a, b]), whole), cut
        # through DDCStream, and in three pieces
        s = d.stream(first_sample=first, out_dtype=torch.int32 if mode == M.IQ32 else torch.int16, polar=mode == M.POLAR)
        parts = [s.push(dev(p)) for p in (x[:cut], x[cut:cut + 3], x[cut + 3:])]
        if mode == M.POLAR:
            parts = [torch.stack([m.view(torch.int16), p], dim=1) for m, p in parts]
        assert np.array_equal(torch.cat(parts).cpu().numpy(), whole), cut
        assert s.first_sample == first + n and s.phase == (phase - n) % decim


@pytest.mark.parametrize("decim,phase", ((1, 0), (8, 3)))
def test_more_than_one_pass_of_the_grid(decim, phase):
    """Three workgroups per compute unit take one step each; a record of more steps than that sends some round again, with
    the images' other pair and the loads made a pass ahead."""
    steps = 3 * torch.cuda.get_device_properties(0).multi_processor_count
    n = (steps + 2) * T + 5
    rng = np.random.default_rng(8)
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    h = rng.integers(-3000, 3001, 9)
    d = bbb.DDC(0x5A5A5A, h.tolist(), decim, phase, shift=3, pa0=1)
    got = d.iq(dev(x), first_sample=(1 << 24) - 5).cpu().numpy()
    assert np.array_equal(got, M.ddc(x, 0x5A5A5A, h, 3, decim, phase, (1 << 24) - 5, 1))


def test_polar_on_zeros_axes_and_quadrants():
    """One batch: the I axis (fcw = 0, pa0 = 0: s = rom[0] = 0), the Q axis (pa0 = 768 << 14: c = rom[1024 mod 1024] = 0), and
    a turning oscillator over samples of both signs with stretches of zeros.  The polar outputs are the CORDIC of the IQ16
    outputs of the same calls, and as close to hypot and atan2 as bbb.h says."""
    rng = np.random.default_rng(9)
    x = rng.integers(-32768, 32768, T + 77)
    x[100:140] = 0
    x[T - 3:T + 3] = 0
    iq, pol = [], []
    for fcw, pa0 in ((0, 0), (0, 768 << 14), (0x5A5A5A, 0xABCDEF)):
        for decim, phase in ((1, 0), (2, 1)):
            iq.append(run_raw(x, 0, 0, 0, fcw, pa0, M.IQ16, [1], 0, decim, phase, 0))
            pol.append(run_raw(x, 0, 0, 1, fcw, pa0, M.POLAR, [1], 0, decim, phase, 0))
    iq, pol = np.concatenate(iq).astype(np.int64), np.concatenate(pol)
    i, q = iq[:, 0], iq[:, 1]
    assert ((i == 0) & (q == 0)).any() and ((i > 0) & (q == 0)).any() and ((i < 0) & (q == 0)).any()
    assert ((i == 0) & (q > 0)).any() and ((i == 0) & (q < 0)).any()
    for si, sq in itertools.product((1, -1), (1, -1)):
        assert ((si * i > 0) & (sq * q > 0)).any()
    mag, ph = M.cordic(i, q)
    assert np.array_equal(pol[:, 0].view(np.uint16), mag) and np.array_equal(pol[:, 1], ph)
    nz = (i != 0) | (q != 0)
    assert np.abs(mag[nz] - np.hypot(i[nz], q[nz])).max() <= 0.59
    err = (ph[nz] - np.arctan2(q[nz], i[nz]) / (2 * np.pi) * 65536 + 32768) % 65536 - 32768
    assert np.abs(err).max() <= 1.0
    assert not mag[~nz].any() and not ph[~nz].any()


def test_closed_loop_nco_to_ddc_on_the_device():
    """NCO.generate with pm = -512 for bit 1, taken down by NCO.ddc: the sign of Q is the bit (tests/test_ddc_host.py has
    the same loop between the models).  Output q of the model's phase 66 is sample 64 + 2 + 64 q: the first 64 samples are
    handed over as history."""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, 512)
    pm = dev(np.repeat(np.where(bits == 1, -512, 0), 64).astype(np.int16))
    with bbb.NCO(1 << 20, am=0xFFFF) as nco:
        x = nco.generate(pm.numel(), pm=pm)
        d = nco.ddc([1] * 64, decim=64, phase=2, shift=6)
    assert d.pa0 == (-3 << 20) % (1 << 24)
    out = bbb.RX(7, 8, 0).downconvert(x, d, first_sample=64, nbefore=64)
    want = M.ddc(x.cpu().numpy(), 1 << 20, [1] * 64, 6, 64, 66, 0, d.pa0)
    got = out.cpu().numpy()
    assert got.shape == (511, 2) and np.array_equal(got, want)
    assert np.array_equal(got[:, 1] > 0, bits[:511] == 1) and np.abs(got[:, 1].astype(np.int64)).min() >= 16000
    # the polar views and what is derived from them
    mag, ph = d.polar(x, first_sample=64, nbefore=64)
    m, p = M.cordic(got[:, 0], got[:, 1])
    assert mag.dtype == torch.uint16 and ph.dtype == torch.int16
    assert np.array_equal(mag.cpu().numpy(), m) and np.array_equal(ph.cpu().numpy(), p)
    assert torch.equal(d.am(x, 64, 64), mag) and torch.equal(d.pm(x, 64, 64), ph)
    assert np.array_equal(d.fm(x, 64, 64).cpu().numpy(), (p[1:].astype(np.int64) - p[:-1]).astype(np.int16))
    # out=: written in place, int32 selected by the tensor
    o32 = torch.empty((511, 2), dtype=torch.int32, device=DEV)
    assert d.iq(x, 64, 64, out=o32) is o32
    assert np.array_equal(o32.cpu().numpy(), M.ddc(x.cpu().numpy(), 1 << 20, [1] * 64, 6, 64, 66, 0, d.pa0, mode=M.IQ32))


def test_example_returns_the_tone_s_amplitude_and_phase():
    """examples/bbb_mc --ddc: the NCO's tone of amplitude am / 2 (x = am * rom >> 16) and phase offset pm / 1024 turn comes back
    as magnitude am / 4 (half the amplitude, the boxcar's gain of 64 undone by the shift of 6) and phase 64 pm - 16384 (a sine
    against the cosine).  The truncations of the three shifts cost the magnitude less than 1 %; the table's period of 1023
    entries (its first and last entry are both 0) costs the phase at most one entry, 64 units."""
    import json
    import subprocess
    from conftest import ROOT
    r = subprocess.run([str(ROOT / "examples" / "bbb_mc"), "--ddc", "1", "--am", "16384", "--pm", "100", "--nco-samples", "100000"],
                       cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout.strip().splitlines()[-1])
    print(j)
    assert j["mode"] == "ddc" and j["outputs"] == 100000 // 64
    assert abs(j["mag_min"] - 4096) <= 41 and abs(j["mag_max"] - 4096) <= 41
    assert abs(j["phase_min"] + 9984) <= 64 and abs(j["phase_max"] + 9984) <= 64
