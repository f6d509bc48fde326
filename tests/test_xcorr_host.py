"""The pulse-response counters and the filter design without a GPU: xcorr_counts against the model, the argument checks of
bbb_xcorr_accumulate_i16 / bbb_tx_xcorr_* through the C ABI, mmse_taps against an independent least-squares fit, the closed
loop measure -> design -> apply -> verify on the CPU oracle's waveform, and the kernel's per-lane core
(basebandboard_amd/csrc/xcorr_common.hpp) run lane by lane on the CPU under ASan/UBSan against the model."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib, equalizer
from basebandboard_amd.bitshaper import _cfg, rcf_coefficients
from conftest import ROOT

import fir_model
import link_model
import xcorr_model as M
from xcorr_model import LOOP, LOOP_DELAY, LOOP_DESIGNED, LOOP_MA_BEST, LOOP_RAW_BEST, LOOP_TAPS

SPBS = (1, 2, 4, 8, 16, 32)

# ---- the model and the counts ----------------------------------------------------------------------------------------

def test_model_equals_the_definition_term_by_term():
    rng = np.random.default_rng(1)
    for spb, nlags, origin, first, n, bit0 in ((1, 5, 0, 0, 40, 0), (4, 9, 17, 3, 90, 0), (8, 64, 17, 0, 300, 0), (8, 20, 50, 31, 77, 0),
                                               (2, 128, 7, 200, 64, 30), (32, 70, 5, 1000, 130, 28), (16, 1, 3, 1, 1, 0)):
        lo, hi = M.needed_bits(first, n, spb, origin, nlags)
        assert lo >= bit0
        bits = rng.integers(0, 2, max(0, hi - bit0 + 1))
        x = rng.integers(-32768, 32768, n)
        got, want = M.xcorr(x, first, bits, bit0, spb, origin, nlags), M.brute(x, first, bits, bit0, spb, origin, nlags)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (spb, nlags, origin, first)


@pytest.mark.parametrize("spb", SPBS)
def test_counts_equal_the_model(spb):
    rng = np.random.default_rng(spb)
    origin = 17
    cases = [(0, 1), (origin, 1), (origin - 1, 2), (origin + 1, spb), (3, 5 * spb + 3), (origin + 5 * spb + 1, 7 * spb - 1), (0, origin),
             (origin + 1000, 0), (1 << 40, 999)]
    cases += [(int(rng.integers(0, 200)), int(rng.integers(0, 700))) for _ in range(12)]
    for first, n in cases:
        for nlags in (1, spb, spb + 1, min(64 * spb, 1024)):
            got = equalizer.xcorr_counts(first, n, spb, origin, nlags)
            assert got.dtype == np.int64 and len(got) == nlags
            if n <= 1000 and first < 1 << 20:
                lo, hi = M.needed_bits(first, n, spb, origin, nlags)
                want = M.xcorr(np.ones(n, dtype=np.int64), first, np.ones(max(0, hi + 1), dtype=np.int64), 0, spb, origin, nlags)[1]
            else:                                      # far out every lag has bit 0 behind it: the residues share the samples
                want = np.array([len(range((origin + l - first) % spb, n, spb)) for l in range(nlags)])
            assert np.array_equal(got, want), (first, n, nlags)
    h = equalizer.pulse_response(np.array([10, -6, 0, 5]), np.array([4, 3, 0, 0]))
    assert h.dtype == np.float64 and h.tolist() == [2.5, -2.0, 0.0, 0.0]


# ---- argument checks -------------------------------------------------------------------------------------------------

def _acc(spb=8, nlags=64, origin=17, first=100, n=1000, bit0=None, nbits=None, samples=1 << 20, bits=1 << 21, xc=1 << 22,
         cfg="default"):
    lo, hi = M.needed_bits(first, n, spb, origin, nlags) if spb in SPBS else (0, 200)
    bit0 = lo if bit0 is None else bit0
    nbits = hi - bit0 + 1 if nbits is None else nbits
    c = _lib.XcorrCfg(spb, nlags, origin)
    lib = _lib.lib()
    rc = lib.bbb_xcorr_accumulate_i16(C.c_void_p(samples), n, first, C.c_void_p(bits), bit0, nbits,
                                      C.byref(c) if cfg == "default" else None, C.c_void_p(xc), 0, None)
    return rc, lib.bbb_last_error_detail().decode()


def test_capture_argument_checks_come_before_the_device():
    import torch
    no_gpu = not torch.cuda.is_available()
    bad = [(dict(spb=3), "spb"), (dict(spb=0), "spb"), (dict(spb=64), "spb"), (dict(nlags=0), "nlags"),
           (dict(spb=1, nlags=65), "nlags"), (dict(spb=8, nlags=513), "nlags"), (dict(spb=32, nlags=1025), "nlags"),
           (dict(spb=16, nlags=1025), "nlags"), (dict(cfg=None), "null xcorr cfg"), (dict(xc=0), "null xc_dev"),
           (dict(samples=0), "null samples_dev"), (dict(bits=0), "null bits_packed_dev"), (dict(samples=(1 << 20) + 1), "misaligned"),
           (dict(xc=(1 << 22) + 4), "misaligned"), (dict(bits=(1 << 21) + 4), "misaligned"), (dict(first=(1 << 62) + 1), "2^62"),
           (dict(first=1 << 61, n=(1 << 62)), "2^62"), (dict(origin=(1 << 62) + 1), "origin"), (dict(bit0=0, nbits=(1 << 62) + 1), "2^62")]
    for kw, what in bad:
        rc, detail = _acc(**kw)
        assert rc == _lib.BBB_EINVAL and what in detail, (kw, rc, detail)
    # a bit range one short at either end, at several placements
    for kw in (dict(), dict(first=0, n=17), dict(first=17, n=1), dict(first=5000, n=3, nlags=1), dict(spb=32, nlags=1024, first=40000, n=70),
               dict(spb=1, nlags=64, origin=0, first=64, n=10)):
        lo, hi = M.needed_bits(kw.get("first", 100), kw.get("n", 1000), kw.get("spb", 8), kw.get("origin", 17), kw.get("nlags", 64))
        if hi < lo:
            continue
        rc, detail = _acc(bit0=lo + 1, nbits=hi - lo, **kw)
        assert rc == _lib.BBB_EINVAL and "needs data bits" in detail, (kw, detail)
        rc, detail = _acc(bit0=lo, nbits=hi - lo, **kw)
        assert rc == _lib.BBB_EINVAL and "needs data bits" in detail, (kw, detail)
        if no_gpu:                                     # the exact range and a wider one pass every check: the device is next
            assert _acc(bit0=lo, nbits=hi - lo + 1, **kw)[0] == _lib.BBB_ENODEV
            assert _acc(bit0=max(0, lo - 3), nbits=hi - max(0, lo - 3) + 70, **kw)[0] == _lib.BBB_ENODEV
    # nothing to do: no samples, or every sample below bit 0 (no bits needed, not even a pointer)
    assert _acc(n=0, samples=0, bits=0)[0] == _lib.BBB_OK
    assert _acc(first=0, n=17, bits=0, bit0=0, nbits=0)[0] == _lib.BBB_OK
    assert _acc(first=0, n=18, bits=0, bit0=0, nbits=0)[0] == _lib.BBB_EINVAL
    # the limits
    if no_gpu:
        for spb in SPBS:
            assert _acc(spb=spb, nlags=min(64 * spb, 1024))[0] == _lib.BBB_ENODEV


def test_transmitter_argument_checks():
    lib = _lib.lib()
    u = bbb.LUTOPT.shipped(256, device=-1)
    base = _cfg(rcf_coefficients(0.5), bbb.PRBS(7, device=-1))
    o = C.c_void_p()

    def einval(rc, text):
        assert rc == _lib.BBB_EINVAL and text in lib.bbb_last_error_detail().decode(), lib.bbb_last_error_detail()

    einval(lib.bbb_tx_xcorr_open(None, C.byref(base), 64, 0, C.byref(o)), "null handle")
    einval(lib.bbb_tx_xcorr_open(u._h, C.byref(base), 64, 0, None), "null out")
    einval(lib.bbb_tx_xcorr_open(u._h, C.byref(base), 0, 0, C.byref(o)), "nlags")
    einval(lib.bbb_tx_xcorr_open(u._h, C.byref(base), 513, 0, C.byref(o)), "nlags")
    einval(lib.bbb_tx_xcorr_open(u._h, C.byref(base), 64, (1 << 30) + 1, C.byref(o)), "chunk_samples")
    bad = _cfg(rcf_coefficients(0.5), bbb.PRBS(7, device=-1))
    bad.prbs_k = 8
    einval(lib.bbb_tx_xcorr_open(u._h, C.byref(bad), 64, 0, C.byref(o)), "k=8 invalid for PRBS")
    assert lib.bbb_tx_xcorr_open(u._h, C.byref(base), 512, 1 << 30, C.byref(o)) == _lib.BBB_ENODEV
    assert not o.value
    einval(lib.bbb_tx_xcorr_run(None, 0, 16, C.c_void_p(1 << 20)), "null xcorr object")
    einval(lib.bbb_tx_xcorr_close(None), "null xcorr object")
    assert "#define BBB_TX_BIT_ORIGIN 17" in (ROOT / "include" / "bbb.h").read_text()
    assert equalizer.TX_BIT_ORIGIN == bbb.TX_BIT_ORIGIN == 17 and equalizer.MAX_LAGS == 1024


# ---- mmse_taps -------------------------------------------------------------------------------------------------------

def _simulate(h, spb, nbits, sigma, seed):
    """(x, s): white +-1 data through h (bit m adds s[m] h[n - spb m] to sample n) plus white noise."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, nbits) * 2 - 1
    up = np.zeros(nbits * spb)
    up[::spb] = s
    x = np.convolve(up, h)[:nbits * spb]
    return x + sigma * rng.standard_normal(len(x)), s


def test_mmse_single_lag_puts_one_tap_at_the_delay():
    for spb, cursor, ntaps, sigma2 in ((8, 5, 7, 0.0), (8, 9, 7, 3.0), (4, 12, 9, 0.5), (1, 3, 4, 0.0)):
        peak = cursor - 2 if sigma2 else cursor
        h = np.zeros(16)
        h[peak] = -3.5
        taps, delay = equalizer.mmse_taps(h, spb, cursor, ntaps, sigma2)
        assert taps.dtype == np.int16 and len(taps) == ntaps and delay == cursor - peak
        assert taps[delay] == -256 and np.abs(np.delete(taps, delay)).max() == 0, taps
    with pytest.raises(ValueError, match="cursor"):
        equalizer.mmse_taps([0, 0, 1, 0], 8, 1, 4, 0.0)                   # a cursor in front of the peak: not causal
    with pytest.raises(ValueError):
        equalizer.mmse_taps([0, 0, 0], 8, 1, 4, 0.0)
    with pytest.raises(ValueError):
        equalizer.mmse_taps([1.0], 8, 0, 0, 0.0)


def test_mmse_two_path_pulse_matches_least_squares():
    """The model-based solution against a data-based one: numpy.linalg.lstsq of the simulated received samples onto the
    sent symbols, for a main path and an echo three samples later (spb 2, so neighbouring bits interfere at every tap).
    Compared on the tap vector normalised to max |w| = 1.  Tolerance: one quantisation step of scale_bits = 8, 1 / 256 =
    0.0039.  Its source, measured on the CPU at this seed and length (2^19 bits): the unquantised model solution and the
    least-squares fit differ by 0.00165 at most (the fit's sampling error; 0.0006 .. 0.0019 over seeds 11 .. 14), rounding to
    8 bits adds at most half a step, 0.00195; the quantised taps / 256 differ from the fit by 0.00281."""
    spb, cursor, ntaps, sigma = 2, 10, 6, 0.3
    h = np.zeros(16)
    h[6:13] = [0.15, 0.5, 1.0, 0.6, -0.3, 0.45, -0.2]
    nbits = 1 << 19
    x, s = _simulate(h, spb, nbits, sigma, seed=11)
    m = np.arange(8, nbits - 8)
    t = spb * m + cursor
    A = np.stack([x[t - i] for i in range(ntaps)], axis=1)
    w_ls = np.linalg.lstsq(A, s[m].astype(np.float64), rcond=None)[0]
    taps, delay = equalizer.mmse_taps(h, spb, cursor, ntaps, sigma * sigma)
    assert delay == cursor - 8 and int(np.abs(taps).argmax()) == delay
    got, want = taps / 256.0, w_ls / np.abs(w_ls).max()
    print("taps", taps.tolist(), "max difference", np.abs(got - want).max())
    assert np.abs(taps).max() == 256
    assert np.abs(got - want).max() <= 1 / 256


def test_mmse_filter_obeys_its_delay():
    """Noiseless: the designed filter applied with tests/fir_model.py and sliced at origin + spb m + cursor returns the
    bits; FIR.mmse carries the same taps and the delay."""
    spb, cursor, ntaps, origin = 4, 13, 10, 6
    h = np.zeros(24)
    h[8], h[11], h[14] = 1.0, 0.55, -0.2
    x, s = _simulate(h, spb, 4000, 0.0, seed=3)
    xi = np.concatenate([np.zeros(origin), np.rint(x * 1000)]).astype(np.int64)      # bit 0 has lag 0 at sample `origin`
    taps, delay = equalizer.mmse_taps(h, spb, cursor, ntaps, 0.01)
    acc = fir_model.acc(xi, taps.tolist())
    m = np.arange(0, 4000 - 8)
    assert np.array_equal(acc[origin + spb * m + cursor] > 0, s[m] > 0)
    # ... which is the unfiltered decision's sample origin + spb m + peak of the stream re-timed by `delay`
    assert origin + spb * 5 + cursor == origin + spb * 5 + 8 + delay
    f = bbb.FIR.mmse(h, spb, cursor, ntaps, 0.01, shift=3)
    assert f.taps == taps.tolist() and f.design_delay == delay and f.shift == 3
    assert bbb.FIR.moving_average().design_delay is None and bbb.FIR([1, 2]).design_delay is None
    # LinkSweep takes a design's delay when none is given: an impossible one is refused before any device is looked for,
    # where the same taps' centroid (1) would have gone on to open the object
    tx_like = type("T", (), {})()
    tx_like.src_sel, tx_like.prbs_shaper = 0, bbb.PRBSShaper(bbb.PRBS(7, device=-1), 0, [[0] * 64])
    g = bbb.FIR([1, 1, 1, 1])
    g.design_delay = -1
    with pytest.raises(ValueError, match="delay"):
        bbb.LinkSweep(tx_like, [bbb.TxSetting()], g)


def test_noise_power():
    assert equalizer.noise_power(1000, 100, [1.0, 2.0, 1.0, 0.0], 2) == 10 - 3
    assert equalizer.noise_power(100, 100, [4.0], 1) == 0.0
    with pytest.raises(ValueError):
        equalizer.noise_power(1, 0, [1.0], 1)


# ---- the closed loop on the CPU --------------------------------------------------------------------------------------

def test_closed_loop_on_the_oracle_waveform(oracle):
    """Measure the pulse response of the oracle's waveform with the model, design 12 taps from it and the measured noise
    power, and count errors at the best phase: unfiltered, behind the moving average, behind the designed filter."""
    n, k = LOOP["n"], LOOP["k"]
    coeffs = rcf_coefficients(LOOP["beta"])
    lut = oracle.Lutopt(path=oracle.data_path(256))
    x = oracle.tx(lut, 1, coeffs, k, n + 64, noise_var=LOOP["noise_var"], warmup=16)
    bits = oracle.prbs_bits(k, n // 8 + 16)[0]
    bit_of = lambda lo, cnt: bits[lo:lo + cnt]                                 # noqa: E731
    xc, counts = M.xcorr(x[:n], 0, bits, 0, 8, 17, LOOP["nlags"])
    assert np.array_equal(counts, equalizer.xcorr_counts(0, n, 8, 17, LOOP["nlags"]))
    h = equalizer.pulse_response(xc, counts)
    # the m-sequence's off-peak correlation keeps the estimate within 2 max |c| / 127 = 4 of the coefficients; the noise (120 rms
    # over 2^17 terms per lag: 0.33 rms) adds less than 5 sigma = 1.7
    assert np.abs(h - np.array(coeffs)).max() < 4.0 + 1.7 and int(np.abs(h).argmax()) == 32
    sigma2 = equalizer.noise_power(int((x[:n].astype(np.int64) ** 2).sum()), n, h, 8)
    taps, delay = equalizer.mmse_taps(h, 8, LOOP["cursor"], LOOP["ntaps"], sigma2)
    raw, _ = link_model.link(x, 0, 0, n, [1], 0, 0, 0, False, bit_of)
    ma, _ = link_model.link(x, 0, 0, n, [1, 1, 1, 1], 2, 0, 0, False, bit_of)
    des, _ = link_model.link(x, 0, 0, n, taps.tolist(), delay, 0, 0, False, bit_of)
    print("noise power", sigma2, "taps", taps.tolist(), "delay", delay)
    print("errors per phase: raw", raw[:, 1].tolist(), "moving average", ma[:, 1].tolist(), "designed", des[:, 1].tolist())
    assert int(raw[:, 1].min()) == LOOP_RAW_BEST and int(ma[:, 1].min()) == LOOP_MA_BEST
    assert 2 * int(des[:, 1].min()) < int(raw[:, 1].min())
    assert int(des[:, 1].min()) <= 10 * LOOP_MA_BEST                            # within an order of magnitude of the moving average
    assert int(des[:, 1].argmin()) in (3, 4) and delay == LOOP_DELAY
    assert taps.tolist() == LOOP_TAPS and des[:, 1].tolist() == LOOP_DESIGNED


# ---- the kernel's core on the CPU, under the sanitizers ----------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("xcorr_host")
    exe = d / "xcorr_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", str(ROOT / "tests" / "xcorr_host.cpp"), "-o", str(exe)])
    return exe


def _case(rng, spb, nlags, origin, first, n, a, gx, bit0_back=0, extra_bits=0, x=None, bits=None):
    lo, hi = M.needed_bits(first, n, spb, origin, nlags)
    bit0 = max(0, lo - bit0_back)
    nbits = max(0, hi - bit0 + 1 + extra_bits)
    b = rng.integers(0, 2, nbits) if bits is None else np.full(nbits, bits)
    x = rng.integers(-32768, 32768, n).astype(np.int16) if x is None else np.full(n, x, dtype=np.int16)
    return dict(spb=spb, nlags=nlags, origin=origin, first=first, bit0=bit0, nbits=nbits, n=n, a=a, gx=gx, x=x, bits=b)


def _blob(c):
    head = np.array([c["spb"], c["nlags"], c["origin"], c["first"], c["bit0"], c["nbits"], c["n"], c["a"], c["gx"], 0], dtype=np.int64)
    xs = np.zeros((c["n"] + 3) // 4 * 4, dtype=np.int16)
    xs[:c["n"]] = c["x"]
    return head.tobytes() + xs.tobytes() + M.pack(c["bits"]).tobytes()


def _long_cases(rng, widths=(8, 65, 129)):
    """More than 2^16 steps of ONE lane at full scale (2051 tiles through one workgroup: 65632 steps of 32768 each pass 2^31),
    at every lane width (8, 16 and 32 lag groups): int32 partials that are not flushed on the way overflow, which UBSan reports.
    -32768 against bits all 1 drives the masked sums and the running total, 32767 against bits all 0 the total alone."""
    cases = [_case(rng, 8, nlags, 17, 0, (2048 + 3) * 8192, 0, 1, x=-32768, bits=1) for nlags in widths]
    if 8 in widths:
        cases.append(_case(rng, 8, 8, 17, 0, (2048 + 3) * 8192, 0, 1, x=32767, bits=0))
    return cases


def test_without_the_flush_the_long_cases_overflow(tmp_path):
    """The negative of the long cases: the same program against a copy of the header whose flush interval is 2^30 (never
    reached) must end in UBSan's signed-overflow report.  So the long cases pass because of the flush."""
    hdr = (ROOT / "basebandboard_amd" / "csrc" / "xcorr_common.hpp").read_text()
    rule = "constexpr int kXcorrFlushSteps = 32768;"
    assert hdr.count(rule) == 1
    (tmp_path / "xcorr_common.hpp").write_text(hdr.replace(rule, "constexpr int kXcorrFlushSteps = 1 << 30;"))
    src = (ROOT / "tests" / "xcorr_host.cpp").read_text()
    inc = '#include "../basebandboard_amd/csrc/xcorr_common.hpp"'
    assert src.count(inc) == 1
    (tmp_path / "xcorr_host.cpp").write_text(src.replace(inc, '#include "xcorr_common.hpp"'))
    exe = tmp_path / "no_flush"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", str(tmp_path / "xcorr_host.cpp"), "-o", str(exe)])
    rng = np.random.default_rng(7)
    short = _case(rng, 8, 8, 17, 0, 3 * 8192 + 5, 0, 1)
    for c, fails in ((short, False), (_long_cases(rng, widths=(8,))[0], True)):
        (tmp_path / "c.bin").write_bytes(_blob(c))
        r = subprocess.run([str(exe), str(tmp_path / "c.bin"), str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=600)
        if fails:
            assert r.returncode != 0 and "signed integer overflow" in r.stderr, (r.returncode, r.stderr[-2000:])
        else:
            assert r.returncode == 0, r.stderr[-2000:]


def test_lane_core_on_the_cpu_equals_the_model(host_exe, tmp_path):
    rng = np.random.default_rng(7)
    cases = []
    for spb in SPBS:
        top = min(64 * spb, 1024)
        for nlags in sorted({1, spb, spb + 1, min(65, top), min(8 * spb + 1, top), min(16 * spb + 1, top), top}):
            # bit 0 inside the range (m < 0 terms, and m = 0 at a lane's step), the range beginning at, before and after it
            cases.append(_case(rng, spb, nlags, 17, 0, 300 + 33 * spb, int(rng.integers(0, 8)), 1))
            cases.append(_case(rng, spb, nlags, 17, 17, 1, 0, 1))
            cases.append(_case(rng, spb, nlags, 17, 18 + 65 * spb, 7, 5, 2, bit0_back=2, extra_bits=3))
        # several tiles, two workgroups, an unaligned pointer, bits that begin above 0, a range far out
        cases.append(_case(rng, spb, min(9 * spb + 3, top), 123, 100, 3 * 8192 + 77, 3, 2))
        cases.append(_case(rng, spb, top, 5, (1 << 40) + 3, 8192 + 9, 7, 3, bit0_back=1))
        # the origin far above the range's start: whole tiles below bit 0
        cases.append(_case(rng, spb, min(40, top), 20000, 1, 30000, 1, 2))
    cases += _long_cases(rng)
    src, out = tmp_path / "cases.bin", tmp_path / "out.txt"
    src.write_bytes(b"".join(_blob(c) for c in cases))
    r = subprocess.run([str(host_exe), str(src), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    lines = out.read_text().splitlines()
    assert len(lines) == len(cases)
    for c, line in zip(cases, lines):
        want = M.xcorr(c["x"], c["first"], c["bits"], c["bit0"], c["spb"], c["origin"], c["nlags"])[0]
        got = np.array(line.split(), dtype=np.int64)
        assert np.array_equal(got, want), {k: v for k, v in c.items() if k not in ("x", "bits")}
