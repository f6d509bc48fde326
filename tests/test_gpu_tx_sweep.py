"""BER sweep over transmitter settings on the GPU, exact: every setting's counters against TX.eye's bathtub for a TX with
that setting (and some against numpy on the oracle's waveform, or far out on TX.generate's), the full shape x noise_var
grid, split invariance, the handle left as it was, the bathtub-only eye at scale, and the C++ example."""
import json
import subprocess

import numpy as np
import pytest
import torch

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from basebandboard_amd.eye import BIT_SAMPLE0, EyeConfig
from basebandboard_amd.txsweep import TxSetting
from conftest import ROOT
from test_gpu_eye import CONFIGS, make_tx, np_tub, tx_taps, u64

pytestmark = pytest.mark.gpu


def setting_kw(kw, s):
    """make_tx keyword arguments of the TX that setting s stands for"""
    out = dict(kw)
    if s.shape_sel is not None:
        out["shape"] = s.shape_sel
    out.update(nv=s.noise_var, bit_en=int(s.bit_en), noise_en=int(s.noise_en))
    return out


def variants(kw, ekw):
    """several settings around one case: its own, other noise_vars, noise / bits off, other decisions"""
    nv = kw.get("nv", 8)
    thr, strict = ekw.get("threshold", 0), ekw.get("strict", False)
    own = dict(noise_var=nv, bit_en=bool(kw.get("bit_en", 1)), noise_en=bool(kw.get("noise_en", 1)))
    return [TxSetting(threshold=thr, strict=strict, **own),
            TxSetting(threshold=thr, strict=strict, **{**own, "noise_var": 0}),
            TxSetting(threshold=thr, strict=strict, **{**own, "noise_var": 15}),
            TxSetting(threshold=-3, strict=not strict, **{**own, "noise_var": 8}),
            TxSetting(threshold=thr, strict=strict, **{**own, "noise_en": False}),
            TxSetting(threshold=100, strict=True, **{**own, "noise_var": 5}),
            TxSetting(threshold=thr, strict=strict, **{**own, "bit_en": False})]


@pytest.mark.parametrize("name, kw, first, n, ekw, chunk", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_sweep_vs_eye(gpu, oracle, name, kw, first, n, ekw, chunk):
    tx = make_tx(**kw)
    settings = variants(kw, ekw)
    with bbb.TxBerSweep(tx, settings, warmup=16, chunk_samples=chunk) as s:
        got = u64(s.run(n, first_sample=first))
    assert got.shape == (len(settings), 8, 2)
    for i, st in enumerate(settings):
        eye = EyeConfig(col_origin=BIT_SAMPLE0, threshold=st.threshold, strict=st.strict)
        _, tub = make_tx(**setting_kw(kw, st)).eye(n, first_sample=first, warmup=16, eye=eye, chunk_samples=chunk)
        assert np.array_equal(got[i], u64(tub)), (name, i, got[i], u64(tub))
    # the case's own setting against numpy on the oracle's waveform
    lut = oracle.Lutopt(path=oracle.data_path(kw.get("lut", 256)))
    x = oracle.tx(lut, 1, tx_taps(tx), tx.prbs.k, n, first_sample=first, source=tx.src_sel, bit_en=int(tx.bit_en),
                  noise_en=int(tx.noise_en), noise_var=tx.noise_var, warmup=16)
    eye = EyeConfig(col_origin=BIT_SAMPLE0, threshold=settings[0].threshold, strict=settings[0].strict)
    assert np.array_equal(got[0], np_tub(x, first, eye, tx.prbs.k, tx.src_sel == 1))


def test_explicit_coefficients_and_mixed_sets(gpu, oracle):
    """settings with their own coefficient sets (several tables in one object) and more than one launch per table"""
    tx = make_tx(k=7, nv=8)
    taps = [[255] * 64, tx_taps(tx), [0] * 32 + [254] + [0] * 31]
    settings = [TxSetting(coeffs=t, noise_var=v, threshold=th) for t in taps for v in (0, 4, 9, 15) for th in (0, 30)]
    settings += [TxSetting(shape_sel=s, noise_var=v) for s in (0, 31) for v in range(16)]
    n, first = 150_001, 3
    got = u64(bbb.TxBerSweep(tx, settings, chunk_samples=(1 << 16) + 8).run(n, first))
    lut = oracle.Lutopt(path=oracle.data_path(256))
    for i, st in enumerate(settings):
        coeffs = st.coeffs if st.coeffs is not None else tx.prbs_shaper.coefficients[st.shape_sel]
        x = oracle.tx(lut, 1, coeffs, 7, n, first_sample=first, noise_var=st.noise_var, warmup=16)
        assert np.array_equal(got[i], np_tub(x, first, EyeConfig(threshold=st.threshold), 7, False)), i


def test_far_out(gpu):
    """first_sample beyond 2^33: against numpy on TX.generate's output"""
    first, n = (1 << 33) + 12_345, 3 * (1 << 16) + 77
    settings = [TxSetting(noise_var=8), TxSetting(noise_var=3, threshold=-20, strict=True), TxSetting(noise_var=14, threshold=9)]
    got = u64(bbb.TxBerSweep(make_tx(k=31, nv=8), settings, chunk_samples=(1 << 16) + 8).run(n, first))
    for i, st in enumerate(settings):
        x = make_tx(k=31, nv=st.noise_var).generate(n, first_sample=first).cpu().numpy()
        assert np.array_equal(got[i], np_tub(x, first, EyeConfig(threshold=st.threshold, strict=st.strict), 31, False)), i


def test_full_grid(gpu):
    n = 1 << 20
    grid = u64(make_tx(k=7, nv=8).ber_sweep(n, noise_vars=range(16), shape_sels=range(32)))
    assert grid.shape == (32, 16, 8, 2)
    rng = np.random.default_rng(5)
    for j in rng.choice(32 * 16, 32, replace=False):
        s, v = divmod(int(j), 16)
        _, tub = make_tx(k=7, nv=v, shape=s).eye(n)
        assert np.array_equal(grid[s, v], u64(tub)), (s, v)
    for s in range(32):
        _, tub = make_tx(k=7, noise_en=0, shape=s).eye(n)
        assert np.array_equal(grid[s, 0], u64(tub)), s
    assert (grid[:, :, :, 0] == grid[0, 0, :, 0]).all()              # bits per phase: the same for every setting
    assert grid[16, 15, :, 1].sum() > grid[16, 0, :, 1].sum()          # more noise, more errors


def test_split_invariance(gpu):
    a, b, c = 7, 7 + 65_541, 7 + 200_003
    settings = [TxSetting(noise_var=v, threshold=t) for v in (2, 10) for t in (0, -4)]
    whole = u64(bbb.TxBerSweep(make_tx(k=31, nv=10), settings, chunk_samples=(1 << 16) + 8).run(c - a, a))
    with bbb.TxBerSweep(make_tx(k=31, nv=10), settings) as s:
        cnt = s.run(b - a, a)
        s.run(c - b, b, counters=cnt)
    assert np.array_equal(u64(cnt), whole)
    with bbb.TxBerSweep(make_tx(k=31, nv=10), settings, chunk_samples=(1 << 16) + 8) as s:
        s.run(c - a, a, counters=cnt)
    assert np.array_equal(u64(cnt), 2 * whole)


def test_handle_unaffected(gpu):
    tx = make_tx(k=7, nv=9)
    tx.ber_sweep(3 * (1 << 16) + 11, first_sample=5, chunk_samples=(1 << 16) + 8)
    got = tx.generate(100_000, first_sample=1000, stream_on=False)
    ref = make_tx(k=7, nv=9).generate(100_000, first_sample=1000, stream_on=False)
    assert torch.equal(got, ref)


def test_at_scale_vs_bathtub_only_eye(gpu):
    n, k = 1 << 27, 31
    grid = u64(make_tx(k=k, shape=12).ber_sweep(n, noise_vars=range(16)))
    for v in range(16):
        with bbb.TxEye(make_tx(k=k, nv=v, shape=12)) as e:
            _, tub = e.run(n, 0, want_hist=False)
        assert np.array_equal(grid[0, v], u64(tub)), v


def test_unsupported_handle(gpu):
    """a handle bbb_tx_fill_i16 refuses with noise on (k = 512) is refused here too, and served with noise off"""
    tx = make_tx(k=7, nv=8, lut=512)
    with pytest.raises(_lib.BbbError) as e:
        tx.ber_sweep(1000, noise_vars=[3])
    assert e.value.code == _lib.BBB_EUNSUP
    with pytest.raises(_lib.BbbError) as e2:
        tx.eye(1000)
    assert e2.value.code == _lib.BBB_EUNSUP
    quiet = make_tx(k=7, noise_en=0, lut=512)
    assert np.array_equal(u64(quiet.ber_sweep(5000, noise_vars=[0]))[0, 0], u64(quiet.eye(5000)[1]))


def test_example_tx_sweep(gpu):
    exe = ROOT / "examples" / "bbb_mc"
    n = 1_000_003
    r = subprocess.run([str(exe), "--tx-sweep", "1", "--eye-samples", str(n), "--prbs", "7", "--shape", "16", "--nv-range", "2:5"],
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    head, rows = lines[0], lines[1:]
    assert head["mode"] == "tx-sweep" and head["settings"] == 4
    grid = u64(make_tx(k=7, shape=16).ber_sweep(n, noise_vars=range(2, 6)))
    want = [(16, v, p, int(grid[0, i, p, 0]), int(grid[0, i, p, 1])) for i, v in enumerate(range(2, 6)) for p in range(8)]
    assert [(d["shape"], d["nv"], d["phase"], d["bits"], d["errors"]) for d in rows] == want
