"""The FIR filter on the GPU, compared exactly with the numpy model (tests/fir_model.py): every tap count with sizes around
every boundary of the kernels, extreme patterns and both saturations, history and cuts, every misalignment, decimation with
every phase, the packed slicer against bbb_rx_slice, indices past 2^31, the receiver with rx_filter, and the C++ example."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest
import torch

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from basebandboard_amd.bitshaper import PRBSShaper
from basebandboard_amd.eye import capture_eye
from conftest import ROOT
import fir_model as M
import grid

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
T = 2048                                           # input samples per workgroup step (kFirTile)
WAVE_BITS = 64 * 8                                 # decisions one wave of the decim = 1 kernel writes
NPDT = {torch.int16: np.int16, torch.int32: np.int32}
OB = {torch.int16: 2, torch.int32: 4}
FIELDS = ("bits", "errors", "errors_raw", "reload_clocks", "resyncs")
NTAPS = (1, 2, 3, 4, 7, 63, 64, 65, 255, 256)


def i64(t):
    return t.view(torch.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def grid_stride():
    """Input samples one pass of the grid covers (tests/grid.py has the workgroups per compute unit)."""
    return T * grid.FIR * grid.cus()


def taps_at_limit(rng, ntaps):
    """Random taps of both signs with sum |h| = 65535 (65534 where two taps cannot reach it, 32768 with one)."""
    if ntaps == 1:
        return np.array([-32768])
    w = rng.random(ntaps) + 0.05
    mag = np.minimum(np.floor(w / w.sum() * 65535).astype(np.int64), 32767)
    i = 0
    while mag.sum() < 65535 and (mag < 32767).any():
        if mag[i % ntaps] < 32767:
            mag[i % ntaps] += 1
        i += 1
    assert 65534 <= mag.sum() <= 65535
    return mag * rng.choice([-1, 1], ntaps)


def run(x, taps, shift=0, decim=1, phase=0, nbefore=0, out_dtype=torch.int16, acc=None):
    """FIR.filter(x[nbefore:]) with x[:nbefore] as history against the model (`acc`: the model's acc of x[nbefore:], when the
    caller has it already)."""
    y = bbb.FIR(taps, shift=shift).filter(dev(x), decim=decim, phase=phase, nbefore=nbefore, out_dtype=out_dtype)
    assert y.dtype == out_dtype and y.numel() == M.nout(len(x) - nbefore, decim, phase)
    if acc is None:
        acc = M.acc(x[nbefore:], taps, before=x[:nbefore])
    ex = acc[phase::decim] >> shift
    ex = np.clip(ex, -32768, 32767).astype(np.int16) if out_dtype == torch.int16 else ex.astype(np.int32)
    got = y.cpu().numpy()
    assert np.array_equal(got, ex), (len(x), len(taps), shift, decim, phase, nbefore, out_dtype, int(np.flatnonzero(got != ex)[0]))
    return y


@pytest.mark.parametrize("ntaps", NTAPS)
def test_tap_counts_and_sizes(gpu, ntaps):
    """Sizes around a step, two steps and one pass of the grid, both output types.  The filter is causal, so the model's acc
    of the longest record serves every shorter one."""
    rng = np.random.default_rng(100 + ntaps)
    h = taps_at_limit(rng, ntaps)
    g = grid_stride()
    x = rng.integers(-32768, 32768, g + 1).astype(np.int16)
    acc = M.acc_fast(x, h)
    assert np.array_equal(acc[:3 * T], M.acc(x[:3 * T], h))
    for n in (1, T - 1, T, T + 1, 2 * T + 1, g - 1, g, g + 1):
        run(x[:n], h, shift=16, out_dtype=torch.int16, acc=acc[:n])
        run(x[:n], h, shift=0, out_dtype=torch.int32, acc=acc[:n])
    f = bbb.FIR(h)
    assert f.filter(torch.empty(0, dtype=torch.int16, device=DEV)).numel() == 0


def test_extremes(gpu):
    n = 2 * T + 9
    lo = np.full(n, -32768, dtype=np.int16)
    alt = np.where(np.arange(n) & 1, 32767, -32767).astype(np.int16)
    for h in ([21845] * 3, [256] * 255 + [255], [32767, 32767, 1]):
        for sign in (1, -1):
            hs = [sign * v for v in h]
            assert sum(abs(v) for v in hs) == 65535
            y = run(lo, hs, out_dtype=torch.int32).cpu().numpy()
            assert int(y[len(h):].astype(np.int64)[0]) == -sign * 65535 * 32768          # the largest |acc| there is
            for shift in (0, 1, 15, 31):
                run(lo, hs, shift=shift, out_dtype=torch.int32)
                y16 = run(lo, hs, shift=shift, out_dtype=torch.int16).cpu().numpy()
                if shift <= 15:
                    assert y16[-1] == (32767 if sign < 0 else -32768)               # saturated at either end
            # taps whose signs follow the alternating samples: every product has one sign
            ha = [v if i % 2 == 0 else -v for i, v in enumerate(hs)]
            for shift in (0, 1, 15, 31):
                run(alt, ha, shift=shift, out_dtype=torch.int32)
                run(alt, ha, shift=shift, out_dtype=torch.int16)
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    for shift in (0, 1, 15, 31):
        run(x, taps_at_limit(rng, 64), shift=shift, out_dtype=torch.int16)
        run(x, taps_at_limit(rng, 64), shift=shift, out_dtype=torch.int32)


@pytest.mark.parametrize("ntaps", [2, 7, 65, 256])
def test_history(gpu, ntaps):
    rng = np.random.default_rng(13 + ntaps)
    h = taps_at_limit(rng, ntaps)
    x = rng.integers(-32768, 32768, 3 * T + 300).astype(np.int16)
    for nb in sorted({0, 1, max(ntaps - 2, 0), ntaps - 1, ntaps + 5}):
        for decim, phase in ((1, 0), (3, 2)):
            run(x[:T + 77 + nb], h, shift=16, nbefore=nb, decim=decim, phase=phase)
            run(x[:nb + 1], h, shift=16, nbefore=nb, decim=decim, phase=phase, out_dtype=torch.int32)


@pytest.mark.parametrize("decim", [1, 3, 8])
def test_cuts_equal_the_uncut_record(gpu, decim):
    """A record cut at 1, T - 1, T and T + 1: through bbb_fir_filter with nbefore and the carried phase, and through FIR.stream."""
    rng = np.random.default_rng(17 + decim)
    x = rng.integers(-32768, 32768, 2 * T + 500).astype(np.int16)
    xd = dev(x)
    for ntaps in (1, 7, 64, 256):
        f = bbb.FIR(taps_at_limit(rng, ntaps), shift=15)
        for phase in {0, decim - 1}:
            for dt in (torch.int16, torch.int32):
                whole = f.filter(xd, decim=decim, phase=phase, out_dtype=dt)
                assert np.array_equal(whole.cpu().numpy(), M.filt(x, f.taps, 15, decim, phase, out_bytes=OB[dt]))
                for cut in (1, T - 1, T, T + 1):
                    nb = min(cut, ntaps - 1)
                    a = f.filter(xd[:cut], decim=decim, phase=phase, out_dtype=dt)
                    b = f.filter(xd[cut - nb:], decim=decim, phase=M.next_phase(phase, decim, cut), nbefore=nb, out_dtype=dt)
                    assert torch.equal(torch.cat([a, b]), whole), (ntaps, phase, cut)
                    s = f.stream(decim=decim, phase=phase, out_dtype=dt)
                    parts = [s.push(xd[:cut]), s.push(xd[cut:cut]), s.push(xd[cut:cut + 3]), s.push(xd[cut + 3:])]
                    assert parts[1].numel() == 0 and torch.equal(torch.cat(parts), whole), (ntaps, phase, cut)
    # many short pieces, shorter than the filter
    f = bbb.FIR(taps_at_limit(rng, 65), shift=14)
    whole = f.filter(xd[:700], decim=decim, phase=decim - 1)
    s = f.stream(decim=decim, phase=decim - 1)
    assert torch.equal(torch.cat([s.push(xd[a:a + 7]) for a in range(0, 700, 7)]), whole)


@pytest.mark.parametrize("out_dt", [torch.int16, torch.int32], ids=["int16", "int32"])
def test_every_misalignment(gpu, out_dt):
    """Input element offsets 0..7 and output element offsets 0..7: offset 0 of either takes the wide path, the others the
    narrow one.  The guard elements around the output stay untouched."""
    rng = np.random.default_rng(19)
    n, guard = T + 333, 64
    src = rng.integers(-32768, 32768, n + 16).astype(np.int16)
    base_in = dev(src)
    f = bbb.FIR(taps_at_limit(rng, 9), shift=16 if out_dt == torch.int16 else 0)
    for decim, phase in ((1, 0), (2, 1)):
        no = M.nout(n, decim, phase)
        for oi in range(8):
            for oo in range(8):
                base_out = torch.full((no + 2 * guard + 8,), 77, dtype=out_dt, device=DEV)
                assert base_in.data_ptr() % 16 == 0 and base_out.data_ptr() % 16 == 0
                lo = guard + oo
                nb = min(oi, 8)
                f.filter(base_in[oi - nb:oi + n], decim=decim, phase=phase, nbefore=nb, out=base_out[lo:lo + no])
                got = base_out.cpu().numpy()
                ex = M.filt(src[oi:oi + n], f.taps, f.shift, decim, phase, before=src[oi - nb:oi], out_bytes=OB[out_dt])
                assert np.array_equal(got[lo:lo + no], ex), (decim, oi, oo)
                assert np.all(got[:lo] == 77) and np.all(got[lo + no:] == 77), (decim, oi, oo)


@pytest.mark.parametrize("decim", [1, 2, 3, 4, 16, 64, 256])
def test_decimation(gpu, decim):
    """Every phase for decim <= 4 and phases 0, 1, decim - 1 beyond; sizes down to those where phase >= nin and nothing is
    written.  A guard word follows the output."""
    rng = np.random.default_rng(23 + decim)
    x = rng.integers(-32768, 32768, 3 * T + 41).astype(np.int16)
    xd = dev(x)
    phases = range(decim) if decim <= 4 else (0, 1, decim - 1)
    for ntaps in (4, 65):
        f = bbb.FIR(taps_at_limit(rng, ntaps), shift=16)
        acc = M.acc(x, f.taps)
        for phase in phases:
            for n in (1, 2, decim - 1, decim, decim + 1, T, T + 1, len(x)):
                if n < 1:
                    continue
                for dt in (torch.int16, torch.int32):
                    no = M.nout(n, decim, phase)
                    buf = torch.full((no + 4,), -21555, dtype=dt, device=DEV)
                    f.filter(xd[:n], decim=decim, phase=phase, out=buf[:no])
                    ex = acc[:n][phase::decim] >> 16
                    got = buf.cpu().numpy()
                    assert no == len(ex) and np.array_equal(got[:no], ex.astype(NPDT[dt])), (ntaps, phase, n, dt)
                    assert np.all(got[no:] == -21555), (ntaps, phase, n, dt)
                    # ... and the slicer's words
                    w, nbits = f.slice(xd[:n], stride=decim, phase=phase, threshold=-3)
                    ew, enb = M.pack((acc[:n][phase::decim] >= -3).astype(np.uint8)), no
                    assert nbits == enb and np.array_equal(w.cpu().numpy().view(np.uint64), ew), (ntaps, phase, n)
    assert M.nout(1, decim, decim - 1) == (1 if decim == 1 else 0)


@pytest.mark.parametrize("stride", [1, 4, 8])
def test_unit_filter_slices_as_rx_slice(gpu, stride):
    rng = np.random.default_rng(29 + stride)
    x = rng.integers(-3, 4, 5 * T + 123).astype(np.int16)                    # many zeros: >= and > differ
    xd = dev(x)
    f = bbb.FIR([1])
    for strict in (False, True):
        for phase in range(min(stride, 3)):
            for n in (1, 63 * stride, 64 * stride, 65 * stride, len(x)):
                a, na = f.slice(xd[:n], stride=stride, phase=phase, strict=strict)
                b, nb = bbb.RX(7, stride, phase).slice(xd[:n], strict=strict)
                assert na == nb and torch.equal(a, b), (strict, phase, n)


def test_slice_thresholds_and_word_boundaries(gpu):
    rng = np.random.default_rng(31)
    x = rng.integers(-2048, 2048, 4 * T).astype(np.int16)
    xd = dev(x)
    h = [1, 1, 1, 1]
    f = bbb.FIR(h)
    for stride in (1, 2, 8):
        nbs = [63, 64, 65, WAVE_BITS - 1, WAVE_BITS, WAVE_BITS + 1, T // stride - 1, T // stride, T // stride + 1]
        for nbits in nbs:
            n = (nbits - 1) * stride + 1
            for thr, strict in ((0, False), (0, True), (1000, False), (-1000, True), (8188, False), (-8192, True), (2 ** 31 - 1, True),
                                (-2 ** 31, False)):
                w, got = f.slice(xd[:n], stride=stride, threshold=thr, strict=strict)
                ew, enb = M.slice_packed(x[:n], h, stride, 0, thr, strict)
                assert got == enb == nbits and w.numel() == (nbits + 63) // 64
                assert np.array_equal(w.cpu().numpy().view(np.uint64), ew), (stride, nbits, thr, strict)      # tail bits are 0
    # equal to the threshold: acc = 4 * 250 on a constant record
    c = dev(np.full(200, 250, dtype=np.int16))
    assert int(f.slice(c, threshold=1000)[0][0]) & 0xFF == 0xF8 and int(f.slice(c, threshold=1000, strict=True)[0][0]) & 0xFF == 0
    # shift and out_bytes play no part
    a = bbb.FIR(h, shift=7).slice(xd[:1000], threshold=500)[0]
    assert torch.equal(a, f.slice(xd[:1000], threshold=500)[0])
    # with history
    w, nb = f.slice(xd[:1000], stride=4, phase=1, nbefore=3)
    ew, enb = M.slice_packed(x[3:1000], h, 4, 1, before=x[:3])
    assert nb == enb and np.array_equal(w.cpu().numpy().view(np.uint64), ew)


def test_indices_past_2_31(gpu):
    """2^31 + 300 inputs filled on the device with x[i] = (7919 i mod 65521) - 32760: the outputs around index 2^31 - 1 and
    the last ones against the model, on those slices only.  The fill's period matters: 65521 is prime, so x[i] differs from
    x[i - 2^31] and from x[i - 2^32] at every i, and an input index that wrapped to a smaller one reads other data (with a
    period of 65536, which divides both, it would read the same; tests/test_periodic_host.py holds both statements)."""
    n = (1 << 31) + 300
    x = torch.empty(n, dtype=torch.int16, device=DEV)
    step = 1 << 27
    for a in range(0, n, step):
        b = min(n, a + step)
        x[a:b] = (((torch.arange(a, b, dtype=torch.int64, device=DEV) * 7919) % 65521) - 32760).to(torch.int16)

    def pattern(a, b):
        return (((np.arange(a, b, dtype=np.int64) * 7919) % 65521) - 32760).astype(np.int16)
    h = [3000, -5000, 7000, -9000, 11000, -13000, 9000, -8535]
    assert sum(abs(v) for v in h) == 65535 and 65535 * 32760 < 2 ** 31                 # |x| <= 32760: acc stays within int32
    f = bbb.FIR(h, shift=3)
    y = f.filter(x, out_dtype=torch.int32)
    assert y.numel() == n
    for a, b in (((1 << 31) - 500, (1 << 31) + 300), (n - 1000, n), (0, 1000)):
        ex = M.filt(pattern(a, b), h, 3, before=pattern(max(a - 7, 0), a), out_bytes=4)
        assert np.array_equal(y[a:b].cpu().numpy(), ex), a
    del y
    # decimated, and sliced: output indices stay small, input indices pass 2^31
    y = f.filter(x, decim=256, phase=255)
    nq = M.nout(n, 256, 255)
    a0 = 255 + 256 * (nq - 8)                                               # the input index of the eighth output from the end
    # the last two outputs sit at input indices 2^31 - 1 and 2^31 + 255
    assert y.numel() == nq and a0 + 256 * 6 == (1 << 31) - 1 and a0 + 256 * 7 < n
    ex = M.filt(pattern(a0, n), h, 3, before=pattern(a0 - 7, a0))[::256]
    assert len(ex) == 8 and np.array_equal(y[nq - 8:].cpu().numpy(), ex)
    w, nbits = f.slice(x, stride=8, phase=5, threshold=100)
    assert nbits == M.nout(n, 8, 5)
    a = (nbits - 512) // 64 * 64                                            # whole words at the end
    ex = M.pack((M.acc(pattern(8 * a, n), h, before=pattern(8 * a - 7, 8 * a))[5::8] >= 100).astype(np.uint8))
    assert np.array_equal(w[a // 64:].cpu().numpy().view(np.uint64), ex)
    del x, y, w
    torch.cuda.empty_cache()


def test_through_the_c_abi_on_a_stream(gpu):
    """bbb_fir_filter and bbb_fir_slice called directly, on a stream of their own: nout_out, history behind the pointer, NULL
    counts, and an output inside the samples refused."""
    rng = np.random.default_rng(41)
    x = rng.integers(-32768, 32768, 3 * T + 5).astype(np.int16)
    xd = dev(x)
    lib = _lib.lib()
    c = _lib.FirCfg()
    h = taps_at_limit(rng, 33)
    c.ntaps = 33
    for i, v in enumerate(h):
        c.taps[i] = int(v)
    c.shift, c.decim, c.phase, c.out_bytes = 16, 5, 3, 2
    nin, nb = len(x) - 40, 40
    no = M.nout(nin, 5, 3)
    y = torch.zeros(no, dtype=torch.int16, device=DEV)
    w = torch.zeros((no + 63) // 64, dtype=torch.int64, device=DEV)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    n = C.c_uint64()
    sp = C.c_void_p(st.cuda_stream)
    assert lib.bbb_fir_filter(C.c_void_p(xd.data_ptr() + 80), nin, nb, C.byref(c), C.c_void_p(y.data_ptr()), C.byref(n), 0, sp) == _lib.BBB_OK
    assert n.value == no
    assert lib.bbb_fir_slice(C.c_void_p(xd.data_ptr() + 80), nin, nb, C.byref(c), -7, 1, C.c_void_p(w.data_ptr()), None, 0, sp) == _lib.BBB_OK
    st.synchronize()
    acc = M.acc(x[40:], h, before=x[:40])[3::5]
    assert np.array_equal(y.cpu().numpy(), (acc >> 16).astype(np.int16))
    assert np.array_equal(w.cpu().numpy().view(np.uint64), M.pack((acc > -7).astype(np.uint8)))
    assert lib.bbb_fir_filter(C.c_void_p(xd.data_ptr() + 80), nin, nb, C.byref(c), C.c_void_p(xd.data_ptr() + 16), None, 0, sp) == _lib.BBB_EINVAL
    assert b"overlaps" in lib.bbb_last_error_detail()
    assert lib.bbb_fir_filter(C.c_void_p(xd.data_ptr() + 80), nin, nb, C.byref(c), C.c_void_p(y.data_ptr()), None, 0, sp) == _lib.BBB_OK
    st.synchronize()


@pytest.fixture(scope="module")
def link():
    """A noisy transmission of the rectangular pulse (the last set of PRBSShaper.from_rcf): 2^18 samples, on both sides."""
    tx = bbb.TX(9, 1, 0, 0, 1, 12, device=0)
    tx.prbs_shaper = PRBSShaper.from_rcf(tx.prbs, 1, [0.5])
    assert tx.prbs_shaper.coefficients[1] == [0] * 30 + [254] * 4 + [0] * 30
    x = tx.generate(1 << 18)
    torch.cuda.synchronize()
    return x, x.cpu().numpy()


def test_receiver_with_the_moving_average(gpu, link):
    xd, x = link
    for f in (bbb.FIR.moving_average(), bbb.FIR.moving_average(pipeline=True)):
        for delay, first in ((2, 0), (5, 0), (2, 16), (7, 13)):
            rx = bbb.RX(9, 8, delay)
            d = M.decisions(x, f.taps)[first + delay::8]
            ew, enb = M.pack(d), len(d)
            w, nb = rx.slice(xd, first, rx_filter=f)
            assert nb == enb and np.array_equal(w.cpu().numpy().view(np.uint64), ew), (delay, first)
            model_bits = dev(ew.view(np.int64))
            assert rx.count_errors(xd, first, first_bit=3, rx_filter=f) == (rx.prbsdet.count_errors(model_bits, enb, first_bit=3), enb)
            got, want = rx.detect(xd, first, rx_filter=f), rx.prbsdet.run_stream(model_bits, enb)
            assert {k: got[k] for k in FIELDS} == {k: want[k] for k in FIELDS}, (delay, first)
    # strict decisions, and a first sample beyond the record
    rx = bbb.RX(9, 8, 2)
    f = bbb.FIR.moving_average()
    w, nb = rx.slice(xd, strict=True, rx_filter=f)
    assert np.array_equal(w.cpu().numpy().view(np.uint64), M.pack(M.decisions(x, f.taps, strict=True)[2::8]))
    assert rx.slice(xd[:100], 200, rx_filter=f)[1] == 0
    # recorded, not asserted: the errors of the exact detector with and without the filter
    plain, filt = bbb.RX(9, 8, 0).detect(xd), rx.detect(xd, rx_filter=f)
    print("noise_var 12, rectangular pulse: plain slicer", {k: plain[k] for k in FIELDS}, "moving average", {k: filt[k] for k in FIELDS})


def test_eye_and_phase_search_with_rx_filter(gpu, link):
    xd, _ = link
    rx = bbb.RX(9, 8, 0)
    f = bbb.FIR.moving_average(shift=2)
    y = f.filter(xd)
    assert y.dtype == torch.int16 and y.numel() == xd.numel()
    assert torch.equal(i64(rx.eye(xd, 5, rx_filter=f)), i64(capture_eye(y, 5)))
    assert torch.equal(i64(rx.eye(xd, 5, rx_filter=f)), i64(rx.eye(y, 5)))
    assert rx.phase_search(xd, rx_filter=f) == rx.phase_search(y)
    stats, best = rx.phase_search(xd, rx_filter=f)
    print("best phase with the moving average", best, {k: stats[best][k] for k in FIELDS})
    # the defaults are what they were
    assert torch.equal(i64(rx.eye(xd, 5)), i64(capture_eye(xd, 5))) and rx.phase_search(xd) == rx.phase_search(xd, rx_filter=None)
    a, na = rx.slice(xd)
    b, nb = rx.slice(xd, rx_filter=None)
    assert na == nb and torch.equal(a, b)


def test_decode_capture_average(gpu):
    """software/memdump/adcplot.py:34-36 in numpy: lfilter([1, 1, 1, 1], [1], dat); dat[3::4]; dat > 0."""
    rng = np.random.default_rng(37)
    dat = rng.integers(-2048, 2048, 8192).astype("<i2")
    filt = np.convolve(dat.astype(np.int64), [1, 1, 1, 1])[:len(dat)]            # lfilter with a = [1]
    ex = (filt[3::4] > 0).astype(np.uint8)
    got = bbb.RX.decode_capture(dat.tobytes(), average=True)
    assert got.dtype == np.uint8 and np.array_equal(got, ex)
    assert np.array_equal(bbb.RX.decode_capture(dat.tobytes()), (dat[::4] > 0).astype(np.uint8))       # unchanged
    assert np.array_equal(bbb.RX.decode_capture(dat.tobytes(), 8, 0, True), (filt[3::8] > 0).astype(np.uint8))


def test_example_prints_the_counts(gpu):
    exe = ROOT / "examples" / "bbb_mc"
    n = 200_000
    r = subprocess.run([str(exe), "--fir", "1", "--eye-samples", str(n), "--prbs", "9", "--nv", "12"], capture_output=True, text=True,
                       timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    out, = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert out["mode"] == "fir" and out["samples"] == n
    tx = bbb.TX(9, 1, 0, 0, 1, 12, device=0)
    tx.prbs_shaper = PRBSShaper.from_rcf(tx.prbs, 1, [0.5])
    x = tx.generate(n)
    plain = bbb.RX(9, 8, 0).detect(x)
    filt = bbb.RX(9, 8, 2).detect(x, rx_filter=bbb.FIR.moving_average())
    for name, st in (("plain", plain), ("moving_average", filt)):
        assert {k: out[name][k] for k in ("bits", "errors", "reload_clocks")} == {k: st[k] for k in ("bits", "errors", "reload_clocks")}, name
    assert out["plain"]["bits"] == out["moving_average"]["bits"] == n // 8
    print("bbb_mc --fir", out)
