"""BER sweep over transmitter settings, host side (no GPU): the argument checks of bbb_tx_ber_sweep_open, and numpy models
of the sweep kernel's formulation -- the shaped-value table with the 8-bit data window (zero bits below 0), int8 noise and
the two wraps against the shaper oracle's waveform, and the 16-bit sign form of the decision against the plain one."""
import ctypes as C

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from basebandboard_amd.bitshaper import _cfg, rcf_coefficients
from basebandboard_amd.txsweep import TxSetting

BIT_SAMPLE0 = 45


def _base():
    return _cfg([0] * 32 + [254] + [0] * 31, bbb.PRBS(7, device=-1))


def _setting(**kw):
    s = _lib.TxSetting()
    for i, v in enumerate(kw.pop("coeffs", rcf_coefficients(0.5))):
        s.coeffs[i] = v
    s.bit_en, s.noise_en, s.noise_var = kw.pop("bit_en", 1), kw.pop("noise_en", 1), kw.pop("noise_var", 8)
    s.threshold, s.strict, s.reserved = kw.pop("threshold", 0), kw.pop("strict", 0), kw.pop("reserved", 0)
    assert not kw
    return s


def _open(u, settings, nset=None, chunk=0, base=None, out=True):
    lib = _lib.lib()
    arr = (_lib.TxSetting * max(1, len(settings)))(*settings) if settings is not None else None
    h = C.c_void_p()
    b = base if base is not None else _base()
    rc = lib.bbb_tx_ber_sweep_open(u._h, C.byref(b), arr, len(settings) if nset is None else nset, chunk,
                                   C.byref(h) if out else None)
    assert not h.value
    return rc, lib.bbb_last_error_detail()


def test_struct_matches_header():
    assert C.sizeof(_lib.TxSetting) == 64 * 2 + 6 * 4
    assert bbb.TxSetting().shape_sel is None and bbb.TxBerSweep is not None


@pytest.mark.parametrize("case, what", [
    ("nset0", b"nset"), ("nset513", b"nset"), ("noise_var16", b"noise_var"), ("coeff_low", b"coefficients"),
    ("coeff_high", b"coefficients"), ("reserved", b"reserved"), ("null_settings", b"null settings"), ("null_out", b"null out"),
    ("chunk", b"chunk_samples"), ("bad_prbs_k", b"k=8 invalid for PRBS")])
def test_bad_arguments_are_einval(case, what):
    """Every argument check comes before the device check: the host-only handle gives BBB_EINVAL, with a detail."""
    u = bbb.LUTOPT.shipped(256, device=-1)
    good = [_setting(), _setting(noise_var=3)]
    base = None
    settings, nset, chunk, out = good, None, 0, True
    if case == "nset0":
        nset = 0
    elif case == "nset513":
        settings = [_setting()] * 513
    elif case == "noise_var16":
        settings = [_setting(), _setting(noise_var=16)]
    elif case == "coeff_low":
        settings = [_setting(coeffs=[0] * 63 + [-256])]
    elif case == "coeff_high":
        settings = [_setting(coeffs=[256] + [0] * 63)]
    elif case == "reserved":
        settings = [_setting(reserved=1)]
    elif case == "null_settings":
        settings, nset = None, 2
    elif case == "null_out":
        out = False
    elif case == "chunk":
        chunk = (1 << 30) + 1
    elif case == "bad_prbs_k":
        base = _base()
        base.prbs_k = 8
    rc, detail = _open(u, settings, nset=nset, chunk=chunk, base=base, out=out)
    assert rc == _lib.BBB_EINVAL, (case, rc, detail)
    assert what in detail, (case, detail)


def test_valid_open_without_device_is_enodev():
    u = bbb.LUTOPT.shipped(256, device=-1)
    # base fields a setting replaces are ignored (here: a noise_var and coefficients no setting could have)
    base = _base()
    base.noise_var, base.coeffs[0] = 99, 300
    rc, detail = _open(u, [_setting(), _setting(bit_en=0, noise_var=15, threshold=-5, strict=1)], base=base)
    assert rc == _lib.BBB_ENODEV and b"host-only" in detail
    rc, _ = _open(u, [_setting(noise_var=v) for v in range(16)] * 32, chunk=1 << 30)      # the whole 32 x 16 grid
    assert rc == _lib.BBB_ENODEV
    lib = _lib.lib()
    assert lib.bbb_tx_ber_sweep_run(None, 0, 16, C.c_void_p(1 << 20)) == _lib.BBB_EINVAL
    assert lib.bbb_tx_ber_sweep_close(None) == _lib.BBB_EINVAL


def test_python_setting_checks():
    tx_like = type("T", (), {})()
    with pytest.raises(ValueError):
        from basebandboard_amd.txsweep import _c_setting
        tx_like.src_sel, tx_like.prbs_shaper = 0, bbb.PRBSShaper(bbb.PRBS(7, device=-1), 0, [[0] * 64])
        _c_setting(tx_like, TxSetting(shape_sel=3))
    assert _c_setting(tx_like, TxSetting(noise_var=5, threshold=-7, strict=True)).noise_var == 5


# ---- the formulation, against the shaper oracle ----------------------------------------------------------------------

def wrap12(v):
    return ((np.asarray(v, dtype=np.int64) + 2048) & 4095) - 2048


def shaped_table(coeffs):
    """T[ph][q] of tx_waveform_kernel: ROM idx adds +c[8 idx + ph] when q bit 7 - idx is set, else -c; wrap12 of the sum"""
    q = np.arange(256)
    T = np.zeros((8, 256), dtype=np.int64)
    for ph in range(8):
        s = np.zeros(256, dtype=np.int64)
        for idx in range(8):
            c = int(coeffs[8 * idx + ph])
            s += np.where((q >> (7 - idx)) & 1, c, -c)
        T[ph] = wrap12(s)
    return T


def source_bits(oracle, k, pulser, m_hi):
    """data bits 0 .. m_hi - 1"""
    if pulser:
        return ((np.arange(m_hi) & 255) == 0).astype(np.int64)
    return oracle.prbs_bits(k, m_hi)[0].astype(np.int64)


def model_tx(coeffs, bits, g, first, n, bit_en, noise_en, nv):
    """x[n] = wrap12(bit_en * T[ph][q] + noise_en * wrap12(g * nv)), q = bits M-7 .. M (oldest in bit 0, bits < 0 are 0)"""
    nabs = first + np.arange(n, dtype=np.int64)
    r = nabs - 17
    M, ph = r >> 3, r & 7
    q = np.zeros(n, dtype=np.int64)
    for j in range(8):
        m = M - 7 + j
        b = np.where(m >= 0, bits[np.clip(m, 0, len(bits) - 1)], 0)
        q |= b << j
    shaped = shaped_table(coeffs)[ph, q] if bit_en else 0
    nz = wrap12(g.astype(np.int64) * nv) if noise_en else 0
    return wrap12(shaped + nz)


CASES = [
    # (name, coeffs, k, source, bit_en, noise_en, nv, first, n)
    ("prbs7_from0", rcf_coefficients(0.5), 7, 0, 1, 1, 8, 0, 3000),
    ("prbs31_off", rcf_coefficients(0.25), 31, 0, 1, 1, 15, 44, 2500),
    ("prbs7_far", rcf_coefficients(1.0), 7, 0, 1, 1, 3, 100_003, 2000),
    ("pulser", rcf_coefficients(0.5), 7, 1, 1, 1, 4, 0, 5000),
    ("pulser_late", rcf_coefficients(0.0), 7, 1, 1, 0, 0, 2041, 3000),
    ("wrap12", [255] * 64, 7, 0, 1, 1, 15, 0, 3000),
    ("bits_off", rcf_coefficients(0.5), 7, 0, 0, 1, 12, 5, 1000),
]


@pytest.mark.parametrize("name, coeffs, k, source, bit_en, noise_en, nv, first, n", CASES, ids=[c[0] for c in CASES])
def test_formulation_reproduces_the_waveform(oracle, name, coeffs, k, source, bit_en, noise_en, nv, first, n):
    lut = oracle.Lutopt(path=oracle.data_path(256))
    warmup = 16
    g = lut.awgn(1, warmup + first, n)                 # sample n's noise: the CLT value of state A^(warmup + n + 1)
    bits = source_bits(oracle, k, source == 1, (first + n) // 8 + 2)
    got = model_tx(coeffs, bits, g, first, n, bit_en, noise_en, nv)
    ref = oracle.tx(lut, 1, coeffs, k, n, first_sample=first, source=source, bit_en=bit_en, noise_en=noise_en, noise_var=nv,
                    warmup=warmup)
    assert np.array_equal(got, ref.astype(np.int64)), np.nonzero(got != ref)[0][:10]
    if name == "wrap12":
        raw = shaped_table(coeffs)
        assert raw.min() < 0 < raw.max() and np.abs(ref).max() > 1500       # the wraps are exercised


def test_decided_bit_sits_in_the_window():
    """Bit m, decided from sample 8m + 45 + p, is window bit 4 (p < 4) or 3 (p >= 4) of that sample, at table phase (p+4) % 8"""
    for m in range(0, 40):
        for p in range(8):
            n = 8 * m + BIT_SAMPLE0 + p
            M, ph = (n - 17) >> 3, (n - 17) & 7
            assert ph == (p + 4) % 8
            assert m - (M - 7) == (4 if p < 4 else 3)


# ---- the 16-bit sign form of the decision (txsweep_kernels.hip) ------------------------------------------------------

def sign_form_errors(shaped, g, nv, b, threshold, strict):
    """What the kernel computes: y0 = 16 T + 8 (mod 2^16), y = 16 g nv + y0 (mod 2^16) for data bit 1; its complement form
    for bit 0; a saturated subtraction of the bound; the error is the sign."""
    t = min(2048, max(-2048, threshold + (1 if strict else 0)))
    sat = lambda v: min(32767, max(-32768, v))                            # noqa: E731
    t0, t1 = sat(-16 * t), sat(16 * t)
    y0 = (16 * shaped + 8) & 0xffff
    g16 = (16 * g) & 0xffff
    gb = np.where(b == 1, g16, (-g16) & 0xffff)
    yb = np.where(b == 1, y0, y0 ^ 0xffff)
    y = (gb * nv + yb) & 0xffff
    y = np.where(y >= 0x8000, y - 0x10000, y)                              # as int16
    d = np.clip(y - np.where(b == 1, t1, t0), -32768, 32767)
    return (d < 0).astype(np.int64)


@pytest.mark.parametrize("threshold", [-5000, -2049, -2048, -2047, -100, -1, 0, 1, 7, 2046, 2047, 2048, 5000])
@pytest.mark.parametrize("strict", [False, True])
def test_sign_form_equals_the_decision(threshold, strict):
    rng = np.random.default_rng(threshold % 1000 + 7 * strict)
    shaped = np.arange(-2048, 2048, dtype=np.int64)
    # every 12-bit shaped value with every noise value at the extreme gains, and random pairs besides
    S = np.concatenate([np.repeat(shaped, 256), rng.integers(-2048, 2048, 200_000)])
    G = np.concatenate([np.tile(np.arange(-128, 128), 4096), rng.integers(-128, 128, 200_000)])
    for nv in (0, 1, 8, 15):
        x = wrap12(S + wrap12(G * nv))
        dec = (x > threshold) if strict else (x >= threshold)
        for b in (0, 1):
            want = (dec != bool(b)).astype(np.int64)
            got = sign_form_errors(S, G, nv, np.full(len(S), b), threshold, strict)
            assert np.array_equal(got, want), (nv, b, np.nonzero(got != want)[0][:5])
