"""The numerically controlled oscillator on the GPU, compared exactly with the numpy model of gateware/bbb/nco.py
(tests/nco_model.py): the reference's known answer, NCOTest's defaults, every mix of buffer and constant inputs, sizes around
every boundary of the kernels, split invariance, the registers, seek, streams, spectra through RX.spectrum, NCO.acf and the
C++ example.

Out of reach: more than one pass of the grid in the fm tile kernels.  bbb_nco_run hands them chunks of 2^24 samples, which
never hold more tiles than their grid has workgroups (tests/grid.py has the kernels that do loop)."""
import json
import subprocess

import numpy as np
import pytest
import torch

import basebandboard_amd as bbb
from basebandboard_amd.spectrum import capture_acf
from conftest import ROOT
import nco_model as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
STEP, TILE, CHUNK = 4096, 16384, 1 << 24           # workgroup step, fm scan tile, fm chunk of bbb_nco_run


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:                                   # moved as int16 bits: uint16 tensors have few kernels
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def inputs(rng, n, use):
    fm = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32) if "fm" in use else int(rng.integers(-2 ** 23, 2 ** 23))
    am = rng.integers(0, 2 ** 16, n).astype(np.uint16) if "am" in use else int(rng.integers(0, 2 ** 16))
    pm = rng.integers(-512, 512, n).astype(np.int16) if "pm" in use else int(rng.integers(-512, 512))
    if "am" in use and n >= 4:
        am[1:3] = (0, 65535)
    return fm, am, pm


def run(o, n, fm, am, pm, out=None):
    t = lambda v: dev(v) if isinstance(v, np.ndarray) else None     # noqa: E731
    return o.generate(n, fm=t(fm), am=t(am), pm=t(pm), out=out).cpu().numpy()


def make(fcw, fm, am, pm, **kw):
    c = lambda v, d: d if isinstance(v, np.ndarray) else v          # noqa: E731
    return bbb.NCO(fcw, am=c(am, 0xFFFF), fm=c(fm, 0), pm=c(pm, 0), **kw)


COMBOS = [tuple(u for u, b in zip(("fm", "am", "pm"), bits) if b) for bits in np.ndindex(2, 2, 2)]


def test_reference_known_answer(gpu):
    """nco.py:47-66 on the device: fcw = 2^14, am = 2^16 - 1, 1024 samples."""
    x = bbb.NCO(2 ** 14, 2 ** 16 - 1).generate(1024).cpu().numpy()
    expected = (np.round(np.sin(np.linspace(0, 2 * np.pi, 1024)) * (2 ** 15 - 1)).astype(np.int64) * (2 ** 16 - 1)) >> 16
    assert x[3:].tolist() == expected.tolist()[:-3] and x[:3].tolist() == [0, 0, 0]
    assert np.array_equal(x, M.clock(1024, 2 ** 14, am=2 ** 16 - 1)[0])


def test_ncotest_defaults(gpu):
    n = 1 << 22
    o = bbb.NCO(2 ** 20, 2 ** 14)
    x = o.generate(n).cpu().numpy()
    ex, st = M.closed(n, 2 ** 20, 0, 2 ** 14, 0)
    assert np.array_equal(x, ex)
    assert tuple(o.state) == st


@pytest.mark.parametrize("use", COMBOS, ids=lambda u: "+".join(u) or "const")
def test_every_mix_of_buffers(gpu, use):
    rng = np.random.default_rng(17 + len(use) + 3 * ("fm" in use) + 5 * ("pm" in use))
    n = 3 * TILE + 777
    fcw = int(rng.integers(0, 2 ** 24))
    fm, am, pm = inputs(rng, n, use)
    o = make(fcw, fm, am, pm)
    x = run(o, n, fm, am, pm)
    ex, st = M.closed(n, fcw, fm, am, pm)
    assert np.array_equal(x, ex)
    assert tuple(o.state) == st
    # a second call continues the waveform from the registers, with fresh buffers
    fm2, am2, pm2 = inputs(rng, 1000, use)
    fm2, am2, pm2 = (v2 if isinstance(v2, np.ndarray) else v1 for v1, v2 in ((fm, fm2), (am, am2), (pm, pm2)))
    x2 = run(o, 1000, fm2, am2, pm2)
    ex2, st2 = M.closed(1000, fcw, fm2, am2, pm2, st)
    assert np.array_equal(x2, ex2) and tuple(o.state) == st2


@pytest.mark.parametrize("n", [1, 2, 3, 4, 63, 65, STEP - 1, STEP + 1, TILE - 1, TILE + 1, CHUNK - 1, CHUNK + 1])
def test_sizes(gpu, n):
    rng = np.random.default_rng(n)
    fcw = int(rng.integers(0, 2 ** 24))
    for use in ((), ("fm", "am", "pm")):
        fm, am, pm = inputs(rng, n, use)
        o = make(fcw, fm, am, pm)
        st0 = (int(rng.integers(0, 2 ** 24)), int(rng.integers(-32768, 32768)), int(rng.integers(-32768, 32768)),
               int(rng.integers(-2 ** 31, 2 ** 31)))
        o.state = st0
        x = run(o, n, fm, am, pm)
        ex, st = M.closed(n, fcw, fm, am, pm, st0)
        assert np.array_equal(x, ex), (n, use)
        assert tuple(o.state) == st, (n, use)


def test_size_2_28_constant(gpu):
    """2^28 samples of constant inputs (one launch of 2^16 workgroup steps, pa wrapped 2^8 times): windows against the
    closed form from reset, and the registers against the host arithmetic.  The constant path's 2^30-sample launch boundary
    is not crossed here; the hand-off between launches is the one the fm chunk +- 1 sizes and the consecutive calls cover."""
    n, fcw, am, fm, pm = 1 << 28, 0x5A5A5A, 40000, -12345, 77
    o = bbb.NCO(fcw, am, fm, pm)
    x = o.generate(n)
    for a in (0, 1 << 20, (1 << 27) - 5000, n - 100_000):
        w = x[a:a + 100_000].cpu().numpy()
        assert np.array_equal(w, M.closed_at(a, len(w), fcw, fm, am, pm)), a
    assert o.state == o.state_after(n)
    del x


def test_split_invariance(gpu):
    rng = np.random.default_rng(11)
    n, fcw = 200_003, 0x3F0F0F
    fm, am, pm = inputs(rng, n, ("fm", "am", "pm"))
    ex, st_end = M.closed(n, fcw, fm, am, pm)
    fmd, amd, pmd = dev(fm), dev(am), dev(pm)
    for trial in range(4):
        cuts = set(rng.integers(0, n, 8).tolist()) | {0, n}
        c0 = int(rng.integers(1000, n - 1000))
        cuts |= {c0, c0 + 1, c0 + 3, c0 + 5}                 # runs of 1-3 samples that cut the pipeline
        cuts = sorted(cuts)
        o = bbb.NCO(fcw)
        out = torch.empty(n, dtype=torch.int16, device=DEV)
        for a, b in zip(cuts[:-1], cuts[1:]):                # slices: misaligned buffers take the element-wise path
            o.generate(b - a, fm=fmd[a:b], am=amd[a:b], pm=pmd[a:b], out=out[a:b])
        assert np.array_equal(out.cpu().numpy(), ex), trial
        assert tuple(o.state) == st_end


def test_mixed_calls_and_retune(gpu):
    """Constant inputs, then buffers, then a retune, then constants again: each piece continues from the registers."""
    rng = np.random.default_rng(3)
    o = bbb.NCO(2 ** 20, 2 ** 14)
    st, got, exp = (0, 0, 0, 0), [], []
    plan = [(5000, (), {}), (3, ("fm",), {}), (7001, ("fm", "am", "pm"), {}), (1, (), {"fcw": 12345, "pm": -3}),
            (2, ("am",), {}), (40_000, (), {"am": 65535, "fm": -(1 << 23)}), (9999, ("pm",), {"fcw": 2 ** 23 + 1})]
    for n, use, retune in plan:
        if retune:
            o.set_cfg(**retune)
        fm, am, pm = inputs(rng, n, use)
        fm = fm if "fm" in use else o.fm
        am = am if "am" in use else o.am
        pm = pm if "pm" in use else o.pm
        got.append(run(o, n, fm if "fm" in use else None, am if "am" in use else None, pm if "pm" in use else None))
        x, st = M.closed(n, o.fcw, fm, am, pm, st)
        exp.append(x)
    assert np.array_equal(np.concatenate(got), np.concatenate(exp))
    assert tuple(o.state) == st


def test_state_get_set(gpu):
    rng = np.random.default_rng(8)
    o = bbb.NCO(0x10001, 30000, 5, -9)
    o.generate(12345)
    assert tuple(o.state) == M.closed(12345, 0x10001, 5, 30000, -9)[1]
    for st0 in ((0xABCDEF, -32768, 32767, -2 ** 31), (1, 2, 3, 2 ** 31 - 1)):
        o.state = st0
        fm, am, pm = inputs(rng, 7777, ("fm", "am", "pm"))
        x = run(o, 7777, fm, am, pm)
        ex, st = M.closed(7777, 0x10001, fm, am, pm, st0)
        assert np.array_equal(x, ex) and tuple(o.state) == st
    o.reset()
    assert tuple(o.state) == (0, 0, 0, 0)
    assert np.array_equal(o.generate(100).cpu().numpy(), M.closed(100, 0x10001, 5, 30000, -9)[0])
    for bad in ((1 << 24, 0, 0, 0), (0, 32768, 0, 0), (0, 0, -32769, 0), (0, 0, 0, 2 ** 31)):
        with pytest.raises(ValueError):
            o.state = bad


def test_seek_far(gpu):
    T = 2 ** 40 + 5
    o = bbb.NCO(0x5A5A5A, 50000, 1000, 300)
    o.seek(T)
    x = o.generate(100_000).cpu().numpy()
    assert np.array_equal(x, M.closed_at(T, 100_000, 0x5A5A5A, 1000, 50000, 300))
    o.seek(1)
    assert np.array_equal(o.generate(10).cpu().numpy(), M.closed(11, 0x5A5A5A, 1000, 50000, 300)[0][1:])


def test_argument_checks(gpu):
    o = bbb.NCO(1 << 20)
    for kw in ({"fm": torch.zeros(10, dtype=torch.int16, device=DEV)}, {"am": torch.zeros(10, dtype=torch.int16, device=DEV)},
               {"pm": torch.zeros(10, dtype=torch.int32, device=DEV)}, {"out": torch.zeros(10, dtype=torch.int32, device=DEV)},
               {"fm": torch.zeros(10, dtype=torch.int32)}, {"fm": torch.zeros(5, dtype=torch.int32, device=DEV)},
               {"pm": torch.zeros(20, dtype=torch.int16, device=DEV)[::2]}):
        with pytest.raises(ValueError):
            o.generate(10, **kw)
    with pytest.raises(ValueError):
        o.generate(-1)
    with pytest.raises(ValueError):
        o.set_cfg(fcw=1 << 24)
    assert o.generate(0).numel() == 0 and tuple(o.state) == (0, 0, 0, 0)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            o.generate(10, fm=torch.zeros(10, dtype=torch.int32, device="cuda:1"))


def test_streams_and_independent_objects(gpu):
    rng = np.random.default_rng(21)
    n = 100_000
    fm, am, pm = inputs(rng, n, ("fm", "am", "pm"))
    fmd, amd, pmd = dev(fm), dev(am), dev(pm)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    a, b = bbb.NCO(0x111111), bbb.NCO(2 ** 20, 2 ** 14)
    xa, xb = [], []
    with torch.cuda.stream(s):
        for k in range(0, n, 25_000):
            xa.append(a.generate(25_000, fm=fmd[k:k + 25_000], am=amd[k:k + 25_000], pm=pmd[k:k + 25_000]))
            xb.append(b.generate(25_000))
    torch.cuda.current_stream(DEV).wait_stream(s)
    xa2 = a.generate(1000)                                   # back on the default stream, ordered behind the side stream
    assert np.array_equal(torch.cat(xa).cpu().numpy(), M.closed(n, 0x111111, fm, am, pm)[0])
    assert np.array_equal(torch.cat(xb).cpu().numpy(), M.closed(n, 2 ** 20, 0, 2 ** 14, 0)[0])
    st = M.closed(n, 0x111111, fm, am, pm)[1]
    assert np.array_equal(xa2.cpu().numpy(), M.closed(1000, 0x111111, 0, 0xFFFF, 0, st)[0])


def peak_bin(f, p):
    return int(np.argmax(p[1:])) + 1


def test_spectrum_tone_and_am_sidebands(gpu):
    rx = bbb.RX(7, 8, 0)
    n, nlags = 1 << 22, 1024
    fcw = 3 * 2 ** 18                                          # 3/64 of the sample rate
    f, p = rx.spectrum(bbb.NCO(fcw).generate(n), nlags=nlags, nfft=4096)
    assert abs(f[peak_bin(f, p)] - fcw / 2 ** 24) <= 1 / 4096
    # AM by a second NCO's tone: sidebands at fc +- fmod
    fmod = 2 ** 18                                             # 1/64
    mod = bbb.NCO(fmod, 2 ** 15).generate(n)                   # +- 16383
    am = (mod.int() + 32768).to(torch.int16).view(torch.uint16)
    x = bbb.NCO(2 ** 22).generate(n, am=am)                    # carrier at 1/4
    f, p = rx.spectrum(x, nlags=nlags, nfft=4096, window="rect")
    k = lambda fr: int(round(fr * 4096))                       # noqa: E731
    carrier, lo, hi = p[k(0.25)], p[k(0.25 - 1 / 64)], p[k(0.25 + 1 / 64)]
    floor = np.median(p)
    assert lo > 100 * floor and hi > 100 * floor and carrier > lo
    assert abs(10 * np.log10(lo / hi)) < 1.0


def test_ncotest_wiring_on_tx_waveform(gpu):
    """NCOTest: fm = adc_b.data << 8 (gateware/top.py:60), here the transmitter's waveform as the ADC capture."""
    n = 1 << 20
    tx = bbb.TX(9, 1, 0, 16, 1, 6, device=0)
    cap = tx.generate(n)
    fm = cap.int() << 8
    o = bbb.NCO(2 ** 20, 2 ** 14)
    x = o.generate(n, fm=fm)
    ex, st = M.closed(n, 2 ** 20, fm.cpu().numpy(), 2 ** 14, 0)
    assert np.array_equal(x.cpu().numpy(), ex) and tuple(o.state) == st
    f, p = bbb.RX(7, 8, 0).spectrum(x, nlags=256)
    assert np.all(np.isfinite(p)) and p.max() > 0


@pytest.mark.parametrize("nlags,n,chunk", [(256, 1_000_003, 1 << 18), (1, 5000, 8), (4096, 300_001, 5000), (100, 50, 16)])
def test_acf_in_chunks_equals_one_capture(gpu, nlags, n, chunk):
    o = bbb.NCO(0x1234567 & 0xFFFFFF, 60000, -5, 3)
    got = o.acf(n, nlags=nlags, chunk_samples=chunk)
    st = o.state
    o.reset()
    whole = o.generate(n)
    assert torch.equal(got, capture_acf(whole, nlags))
    assert o.state == st
    f, p = o.spectrum(0 + 10_000, nlags=min(nlags, 64) + 1)
    assert len(f) == len(p)


def test_example_writes_the_waveform(gpu, tmp_path):
    exe = ROOT / "examples" / "bbb_mc"
    out = tmp_path / "nco.bin"
    n = 1_000_003
    r = subprocess.run([str(exe), "--nco", str(out), "--fcw", "1048576", "--am", "16384", "--nco-samples", str(n)],
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    (head,) = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    x = np.frombuffer(out.read_bytes(), dtype="<i2")
    o = bbb.NCO(2 ** 20, 2 ** 14)
    assert np.array_equal(x, o.generate(n).cpu().numpy())
    assert head["samples"] == n and (head["pa"], head["q"], head["w"], head["y"]) == tuple(o.state)
