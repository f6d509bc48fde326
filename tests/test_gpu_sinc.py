"""The 16x sinc interpolator on the GPU, compared exactly with the numpy model of gateware/bbb/sinc.py (tests/sinc_model.py):
the reference's batch, the four type combinations, saturating int16 input, extreme patterns, sizes around every boundary of
the kernel, more than 2^32 output bytes, history and cuts, every misalignment, streams, the interpolated eye, and the
interpolated phase search of RX."""
import ctypes as C
import json
import subprocess

import numpy as np
import pytest
import torch

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from basebandboard_amd.eye import EyeConfig, capture_eye
from conftest import GOLDEN, ROOT
import sinc_model as M
import grid

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BLOCK = 256                                        # input samples per workgroup step
NPDT = {torch.int8: np.int8, torch.int16: np.int16}
FIELDS = ("bits", "errors", "errors_raw", "reload_clocks", "resyncs")


def i64(t):
    return t.view(torch.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def grid_stride():
    """Input samples one pass of the grid covers (tests/grid.py has the workgroups per compute unit)."""
    return BLOCK * grid.SINC * grid.cus()


def check(x, shift=0, out_dtype=None, nbefore=0, **kw):
    """interpolate(x[nbefore:]) with x[:nbefore] as history against the model."""
    s = bbb.SincInterpolator()
    y = s.interpolate(dev(x), nbefore=nbefore, shift=shift, out_dtype=out_dtype, **kw)
    want = out_dtype or {np.dtype(np.int8): torch.int8, np.dtype(np.int16): torch.int16}[x.dtype]
    assert y.dtype == want and y.numel() == 16 * (len(x) - nbefore)
    ex = M.interpolate(x[nbefore:], before=x[:nbefore], shift=shift)
    got = y.cpu().numpy()
    assert np.array_equal(got, ex), (len(x), shift, out_dtype, nbefore, int(np.flatnonzero(got != ex)[0]))
    return y


def test_reference_batch(gpu):
    g = json.load(open(GOLDEN / "sinc_ref.json"))
    x = np.array(g["input"], dtype=np.int8)
    s = bbb.SincInterpolator()
    y = s.run(x)
    assert isinstance(y, np.ndarray) and y.dtype == np.int8 and y.tolist() == g["output"][:1024]
    yt = s.run(dev(x))
    assert yt.is_cuda and yt.dtype == torch.int8 and yt.cpu().tolist() == g["output"][:1024]
    assert s.run(torch.from_numpy(x)).tolist() == g["output"][:1024]
    assert s.run(g["input"]).tolist() == g["output"][:1024]
    # with 8 zero samples appended the stream form gives all 1106 values of the reference's model
    y = s.interpolate(dev(np.concatenate([x, np.zeros(8, dtype=np.int8)]))).cpu().numpy()
    assert y[109:1215].tolist() == g["output"]


def test_example_prints_the_batch(gpu, tmp_path):
    g = json.load(open(GOLDEN / "sinc_ref.json"))
    exe = ROOT / "examples" / "bbb_mc"
    pgm = tmp_path / "sinc_eye.pgm"
    n = 200_000
    r = subprocess.run([str(exe), "--sinc", str(pgm), "--eye-samples", str(n), "--prbs", "9", "--nv", "2", "--shape", "16",
                        "--shift", "1"],
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    batch, eye = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert batch["mode"] == "sinc" and batch["batch"] == g["output"][:1024]
    assert eye["captured"] == n // 2 and eye["interpolated"] == 16 * (n // 2)
    # the same eye through Python: every second sample of the transmitter's waveform, interpolated
    cap = bbb.TX(9, 1, 0, 16, 1, 2, device=0).generate(n)[::2].contiguous()
    hist = bbb.RX(9, 4, 0).eye(cap, eye=EyeConfig(ncols=64, shift=0, col_origin=392 - 32), interpolate=True, shift=1)
    img = np.frombuffer(pgm.read_bytes()[-256 * 64:], dtype=np.uint8).reshape(256, 64)
    h = i64(hist).cpu().numpy()
    assert np.array_equal(img > 0, h > 0)
    # an open eye: the bit centre lands in column 32, where next to nothing (the start of the record) is near the threshold
    assert h[:, 32].sum() == 16 * (n // 2) // 64 and h[120:135, 32].sum() < 0.001 * h[:, 32].sum()


@pytest.mark.parametrize("in_dt,out_dt", [(i, o) for i in (torch.int8, torch.int16) for o in (torch.int8, torch.int16)],
                         ids=lambda d: str(d).split(".")[-1])
def test_type_combinations(gpu, in_dt, out_dt):
    rng = np.random.default_rng(11)
    n = 3 * BLOCK + 77
    if in_dt == torch.int8:
        check(rng.integers(-128, 128, n).astype(np.int8), out_dtype=out_dt)
        return
    for shift in (0, 4, 15):
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        x[:8] = (32767, -32768, 127, 128, -128, -129, 0, -1)           # saturate both ways, and the edges of the range
        x[100:110] = (127 << shift) if shift < 8 else 32767
        x[200:210] = max(-128 << shift, -32768)
        check(x, shift=shift, out_dtype=out_dt)
    # small values pass shift 0 unclamped
    check(rng.integers(-128, 128, n).astype(np.int16), shift=0, out_dtype=out_dt)


def test_extreme_patterns(gpu):
    n = 2 * BLOCK + 9
    for v in (127, -128):
        y = check(np.full(n, v, dtype=np.int8)).cpu().numpy()
        assert abs(int(y[16 * 8:].astype(np.int64).max()) - v * 126 // 256) <= 1
    # the worst-sign pattern of every phase: the largest sums the adders ever see
    for c in range(16):
        w = np.where(M.H[c::16] >= 0, 127, -128)[::-1]               # x[m - i] follows the sign of tap i
        x = np.tile(np.concatenate([w, -1 - w]), 40).astype(np.int8)
        y = check(x, out_dtype=torch.int16).cpu().numpy()
        assert y.max() <= 101 and y.min() >= -102
    assert max(np.abs(M.acc(np.where(M.H[c::16] >= 0, 127, -128)[::-1])).max() for c in range(16)) > 25000
    rng = np.random.default_rng(5)
    check(rng.integers(-128, 128, 100_000).astype(np.int8))
    check(rng.integers(-2048, 2048, 100_000).astype(np.int16), shift=4)


def test_sizes_around_every_boundary(gpu):
    rng = np.random.default_rng(7)
    g = grid_stride()
    sizes = [1, 2, 7, 8, 9, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, g - 1, g, g + 1,
             2 * g + 1, 10 ** 6 + 3]
    for n in sizes:
        check(rng.integers(-128, 128, n).astype(np.int8))
    for n in (1, 8, BLOCK + 1, g + 1):
        check(rng.integers(-32768, 32768, n).astype(np.int16), shift=7, out_dtype=torch.int16)
    s = bbb.SincInterpolator()
    assert s.interpolate(torch.empty(0, dtype=torch.int8, device=DEV)).numel() == 0


def torch_model(x, before):
    """The model in torch on the GPU (int32), for records too long for numpy: x int8 [n], before int8 [<= 7]."""
    h = dev(M.H.astype(np.int32)).reshape(8, 16)
    xe = torch.cat([torch.zeros(7 - before.numel(), dtype=torch.int32, device=DEV), before.int(), x.int()])
    acc = torch.zeros(x.numel(), 16, dtype=torch.int32, device=DEV)
    for i in range(8):
        acc += xe[7 - i:7 - i + x.numel(), None] * h[i][None, :]
    return (acc >> 8).reshape(-1)


def test_more_than_4g_output_bytes(gpu):
    """nin > 2^28: the output indices pass 2^32.  Compared in full, against the model in torch, itself checked against numpy."""
    rng = np.random.default_rng(9)
    small = rng.integers(-128, 128, 100_003).astype(np.int8)
    assert np.array_equal(torch_model(dev(small[5:]), dev(small[:5])).cpu().numpy(), M.interpolate(small[5:], before=small[:5]))
    n = (1 << 28) + 12_345
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    x = torch.randint(-128, 128, (n,), dtype=torch.int8, device=DEV, generator=g)
    y = bbb.SincInterpolator().interpolate(x)
    assert y.numel() == 16 * n > 1 << 32
    step = 1 << 24
    for a in range(0, n, step):
        b = min(n, a + step)
        ex = torch_model(x[a:b], x[max(0, a - 7):a])
        assert torch.equal(y[16 * a:16 * b].int(), ex), a
    del y
    torch.cuda.empty_cache()


def test_history_and_cuts(gpu):
    rng = np.random.default_rng(13)
    for dt, shift in ((np.int8, 0), (np.int16, 3)):
        lo, hi = (-128, 128) if dt == np.int8 else (-2048, 2048)
        x = rng.integers(lo, hi, 5000).astype(dt)
        for nb in range(8):
            check(x[:1000 + nb], nbefore=nb, shift=shift)
            check(x[:nb + 1], nbefore=nb, shift=shift)
        check(x[:40], nbefore=30, shift=shift)                             # more history than the filter uses
        # a record cut at arbitrary points, each piece given its 7 earlier samples, equals one call
        s = bbb.SincInterpolator()
        xd = dev(x)
        whole = s.interpolate(xd, shift=shift)
        for _ in range(5):
            cuts = sorted(set(rng.integers(1, len(x), 6).tolist()) | {0, len(x)})
            parts = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                nb = min(a, 7)
                parts.append(s.interpolate(xd[a - nb:b], nbefore=nb, shift=shift))
            assert torch.equal(torch.cat(parts), whole), cuts


@pytest.mark.parametrize("in_dt,out_dt", [(i, o) for i in (torch.int8, torch.int16) for o in (torch.int8, torch.int16)],
                         ids=lambda d: str(d).split(".")[-1])
def test_every_misalignment(gpu, in_dt, out_dt):
    """Input and output slices at every offset within 16 bytes; the guard elements around the output stay untouched."""
    rng = np.random.default_rng(17)
    n, guard = 1000, 64
    s = bbb.SincInterpolator()
    src = rng.integers(-128, 128, n + 64).astype(NPDT[in_dt])
    base_in = dev(src)
    nin_off, nout_off = 16 // base_in.element_size(), 16 // torch.empty(0, dtype=out_dt).element_size()
    pairs = {(oi, (5 * oi + 1) % nout_off) for oi in range(nin_off)} | {(3 % nin_off, oo) for oo in range(nout_off)}
    for oi, oo in sorted(pairs):
        base_out = torch.full((16 * n + 2 * guard + 16,), 77, dtype=out_dt, device=DEV)
        assert base_in.data_ptr() % 16 == 0 and base_out.data_ptr() % 16 == 0
        lo = guard + oo
        for nb in (0, min(oi, 7)):
            base_out.fill_(77)
            x = base_in[oi - nb:oi + n]
            s.interpolate(x, nbefore=nb, out=base_out[lo:lo + 16 * n])
            got = base_out.cpu().numpy()
            assert np.array_equal(got[lo:lo + 16 * n], M.interpolate(src[oi:oi + n], before=src[oi - nb:oi])), (oi, oo, nb)
            assert np.all(got[:lo] == 77) and np.all(got[lo + 16 * n:] == 77), (oi, oo, nb)


def test_streams(gpu):
    rng = np.random.default_rng(19)
    n = 300_001
    a, b = rng.integers(-128, 128, n).astype(np.int8), rng.integers(-2048, 2048, n).astype(np.int16)
    ad, bd = dev(a), dev(b)
    s = bbb.SincInterpolator()
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        ya = s.interpolate(ad)
        yb = s.interpolate(bd, shift=4, out_dtype=torch.int8)             # queued right behind the first
        yc = s.interpolate(ya.clone()[:1000].contiguous())               # and one that reads the first call's output
    st.synchronize()
    assert np.array_equal(ya.cpu().numpy(), M.interpolate(a))
    assert np.array_equal(yb.cpu().numpy(), M.interpolate(b, shift=4))
    assert np.array_equal(yc.cpu().numpy(), M.interpolate(M.interpolate(a)[:1000]))


@pytest.mark.parametrize("ncols", [8, 16, 32, 64])
def test_eye_of_the_interpolated_record(gpu, ncols):
    rng = np.random.default_rng(23 + ncols)
    n, first = 20_011, 12_345
    s = bbb.SincInterpolator()
    for dt, shift, chunks in ((np.int16, 4, (0, 1000, 4097)), (np.int8, 0, (1000,))):
        x = rng.integers(-2048, 2048, n).astype(dt) if dt == np.int16 else rng.integers(-128, 128, n).astype(np.int8)
        xd = dev(x)
        eye = EyeConfig(ncols=ncols, shift=1, col_origin=37)
        y = M.interpolate(x, shift=shift)
        ex = M.eye_hist(y, 16 * first, ncols, 1, 37)
        direct = capture_eye(s.interpolate(xd, shift=shift, out_dtype=torch.int16), 16 * first, eye)
        assert np.array_equal(direct.cpu().numpy().astype(np.int64), ex)
        for chunk in chunks:
            h = s.eye(xd, first, eye, shift=shift, chunk_in=chunk)
            assert torch.equal(i64(h), i64(direct)), (dt, chunk)
        # a record cut into several runs, each with its history, adding into one histogram
        h = None
        for a, b in ((0, 1), (1, 5000), (5000, 5003), (5003, n)):
            nb = min(a, 7)
            h = s.eye(xd[a - nb:b], first + a, eye, hist=h, shift=shift, nbefore=nb, chunk_in=1000)
        assert torch.equal(i64(h), i64(direct)), dt
    # the defaults: 64 columns, shift 0, first_sample 0
    assert np.array_equal(s.eye(xd).cpu().numpy().astype(np.int64), M.eye_hist(y, 0, 64, 0, 0))


def test_eye_object_through_the_c_abi(gpu):
    """One object, several runs on a stream of its own; cfg.out_bytes is ignored."""
    rng = np.random.default_rng(29)
    x = rng.integers(-2048, 2048, 9001).astype(np.int16)
    xd = dev(x)
    lib = _lib.lib()
    st = torch.cuda.Stream(device=DEV)
    hist = torch.zeros(256, 32, dtype=torch.uint64, device=DEV)
    torch.cuda.synchronize()
    e = C.c_void_p()
    cfg, eye = _lib.SincCfg(2, 9, 4), _lib.EyeCfg(32, 0, 5, 0, 0)
    assert lib.bbb_sinc_eye_open(C.byref(cfg), C.byref(eye), 777, 0, C.c_void_p(st.cuda_stream), C.byref(e)) == _lib.BBB_OK
    assert lib.bbb_sinc_eye_run(e, C.c_void_p(xd.data_ptr()), 4000, 0, 100, C.c_void_p(hist.data_ptr())) == _lib.BBB_OK
    assert lib.bbb_sinc_eye_run(e, C.c_void_p(xd.data_ptr() + 2 * 4000), 5001, 7, 4100, C.c_void_p(hist.data_ptr())) == _lib.BBB_OK
    assert lib.bbb_sinc_eye_run(e, None, 0, 0, 0, C.c_void_p(hist.data_ptr())) == _lib.BBB_OK
    assert lib.bbb_sinc_eye_close(e) == _lib.BBB_OK
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), M.eye_hist(M.interpolate(x, shift=4), 1600, 32, 0, 5))


def test_rx_phase_search_interpolated(gpu):
    """RX.phase_search(interpolate=True) = interpolate, then slice and detect at each of the 64 phases; on a capture at 4
    samples per bit taken 0.3 of a sample late its best phase decodes with no error after the detector's preamble."""
    nbits, spb = 6000, 4
    x, bits = M.rc_capture(nbits, 0.3, spb)
    x = x[:spb * (nbits - 8)]                                # the last pulses lack their successors
    rx = bbb.RX(7, spb, 0)
    for cap, shift in ((dev(x), 0), (dev(x.astype(np.int16) * 16 + 5), 4)):
        stats, best = rx.phase_search(cap, interpolate=True, shift=shift)
        assert len(stats) == 16 * spb
        y = rx.interpolate(cap, shift=shift)
        assert y.dtype == torch.int16 and np.array_equal(y.cpu().numpy(), M.interpolate(x))
        for p in range(16 * spb):
            d = bbb.RX(7, 16 * spb, p).detect(y)
            assert {k: stats[p][k] for k in FIELDS} == {k: d[k] for k in FIELDS}, p
        print("best phase", best, {k: stats[best][k] for k in FIELDS})
        assert stats[best]["errors"] == 0 and stats[best]["bits"] == nbits - 8
    # the uninterpolated search of the same capture answers in whole samples
    coarse, cbest = rx.phase_search(dev(x.astype(np.int16)))
    assert len(coarse) == spb and 0 <= cbest < spb


def test_rx_defaults_are_unchanged(gpu):
    """interpolate=False (the default) takes the paths RX had before: bbb_eye_accumulate_i16 and bbb_rx_phase_search with
    the caller's stride and samples_per_bit phases, the same numbers."""
    n = 8 * 40_000
    x = bbb.TX(31, 1, 0, 16, 1, 6, device=0).generate(n)
    rx = bbb.RX(31, 8, 1)
    h = rx.eye(x, 5)
    assert torch.equal(i64(h), i64(capture_eye(x, 5))) and torch.equal(i64(h), i64(rx.eye(x, 5, interpolate=False)))
    assert np.array_equal(h.cpu().numpy().astype(np.int64), M.eye_hist(x.cpu().numpy(), 5, 64, 4, 0))
    stats, best = rx.phase_search(x)
    assert (stats, best) == rx.phase_search(x, interpolate=False) and len(stats) == 8
    st = (_lib.DetectorStats * 8)()
    _lib.check(_lib.lib().bbb_rx_phase_search(C.c_void_p(x.data_ptr()), n, 8, 8, 0, 31, st, 0,
                                              C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "bbb_rx_phase_search")
    assert stats == [{f: int(getattr(s, f)) for f, _ in _lib.DetectorStats._fields_} for s in st]
    assert best == min(range(8), key=lambda p: (stats[p]["errors"] + stats[p]["reload_clocks"], p))
    for p in range(8):
        d = bbb.RX(31, 8, p).detect(x)
        assert {k: stats[p][k] for k in FIELDS} == {k: d[k] for k in FIELDS}
