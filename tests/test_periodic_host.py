"""The conditions under which a tiled record proves anything (tests/periodic.py), asserted on the CPU for every unit that
tests/test_gpu_wide.py tiles: the model is periodic from period 1 on and its counters are linear (the builders assert that as
they cut the model's output), no power of two is a multiple of a period in items, bytes or words, and a unit or an expected
output turned by 2^31 or 2^32 places differs from itself nearly everywhere.  No GPU."""
import time

import numpy as np
import pytest

import periodic as P


def test_the_helpers_on_small_cases():
    assert P.odd_factor(9216) == 9 and P.odd_factor(65536) == 1 and P.odd_factor(65521) == 65521
    assert P.residues(9216) == (8192, 7168) and P.residues(65536) == (0, 0)
    a = np.arange(12)
    assert P.shift_differs(a, 5) == 1.0 and P.shift_differs(a, 12) == 0.0
    b = np.array([0, 0, 0, 0, 0, 1])
    assert P.shift_differs(b, 1) == pytest.approx(2 / 6) and P.shift_differs(b, 1, group=3) == pytest.approx(4 / 6)
    with pytest.raises(AssertionError):
        P.assert_shift_shows(np.arange(4096), "a power of two")
    with pytest.raises(AssertionError):
        P.assert_shift_shows(np.arange(3 * 4096) % 1024, "a period inside the period")
    with pytest.raises(AssertionError):
        P.linear([1, 2], [2, 4], [3, 7])
    assert P.linear([1, 2], [2, 4], [3, 6])(10) == [9, 18]
    out = np.array([9, 1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2])
    e = P.Expect.cut(out, (3, 6, 9), "toy")
    assert e.head.tolist() == [9, 1, 2] and e.period.tolist() == [3, 1, 2] and e.tail.tolist() == [3, 1, 2] and e.length(5) == 18
    with pytest.raises(AssertionError):
        P.Expect.cut(out, (2, 5, 8), "toy, cut where period 0 still shows")
    K = P.periods_past(P.P32, 9216, 127)
    assert (K - 3) * 9216 > P.P32 - 9216 and (K - 4) * 9216 <= P.P32


def test_the_fir_fill_differs_from_itself_shifted():
    """x[i] = (7919 i mod 65521) - 32760 of tests/test_gpu_fir.py: the period 65521 is prime.  The fill it replaces, modulo 65536,
    is its own copy 2^31 and 2^32 places on."""
    i = np.arange(65521, dtype=np.int64)
    P.assert_shift_shows(i * 7919 % 65521 - 32760, "the FIR test's fill", least=0.9999)
    j = np.arange(65536, dtype=np.int64)
    old = (j * 7919 & 0xFFFF) - 32768
    assert P.odd_factor(65536) == 1 and P.shift_differs(old, P.P31 % 65536) == 0.0 and P.shift_differs(old, P.P32 % 65536) == 0.0
    for a in (P.P31, P.P32):
        k = a + np.arange(5000, dtype=np.int64)
        assert np.array_equal(k * 7919 & 0xFFFF, (k - a) * 7919 & 0xFFFF)
        assert (k * 7919 % 65521 != (k - a) * 7919 % 65521).all()


def _built(name):
    t0 = time.time()
    r = getattr(P, name)()
    dt = time.time() - t0
    print(name, f"model {dt:.2f} s")
    assert dt < 10.0, f"{name}: the unit's model took {dt:.1f} s (it takes well under 1 s on an idle core)"
    return r


def _outputs(r, name, items=(), bits=()):
    for key in items:
        P.assert_shift_shows(r["expect"][key].period, f"{name} {key}")
    for key in bits:
        P.assert_shift_shows(r["expect"][key].period, f"{name} {key}", group=64)


def test_carrier_unit():
    r = _built("carrier")
    p = r["p"]
    assert p == 9216 and P.residues(p) == (8192, 7168)
    assert P.odd_factor(p) > 1 and P.odd_factor(4 * p) > 1 and P.odd_factor(p // 64) > 1 and P.odd_factor(p // 24) > 1      # pairs, bytes, words, blocks
    P.assert_shift_shows(r["unit"], "carrier pairs")
    P.assert_shift_shows(r["unit"].reshape(-1), "carrier int16 elements")
    _outputs(r, "carrier", items=("iq", "soft"), bits=("bits",))
    assert P.shift_differs(r["expect"]["phases"].period, (P.P32 // 24) % 384) > 0.9
    blocks, flips, zero, steps = r["per_period"]
    assert blocks == 384 and flips >= 4 and zero == 0 and steps == 2 * 65536            # two turns a period
    assert r["stats"](7) == [a + 5 * b for a, b in zip(r["stats"](2), r["per_period"])]


def test_dfe_unit():
    r = _built("dfe")
    p = r["p"]
    assert p == 3 * 4096 and P.residues(p) == (P.P31 % p, P.P32 % p) == (8192, 4096)
    assert P.odd_factor(p) > 1 and P.odd_factor(2 * p) > 1 and P.odd_factor(p // 64) > 1
    P.assert_shift_shows(r["unit"], "dfe samples")
    _outputs(r, "dfe", items=("soft",), bits=("bits",))
    # period 0 differs from the later ones: its first decisions come from the state word
    assert not np.array_equal(r["expect"]["soft"].head, r["expect"]["soft"].period)
    s2, s5 = r["stats"](2), r["stats"](5)
    assert s5[0] - s2[0] == 9 and s5[3] - s2[3] == 3 * p


@pytest.mark.parametrize("name", ["timing_wraps", "timing_level"])
def test_timing_units(name):
    r = _built(name)
    p = r["p"]
    assert p == 192 * 256 and P.residues(p) == (P.P31 % p, P.P32 % p) == (32768, 16384)
    assert P.odd_factor(p) > 1 and P.odd_factor(2 * p) > 1
    P.assert_shift_shows(r["unit"], name + " samples", least=0.99)
    blocks, moves, up, down = r["per_period"]
    per_bits = len(r["expect"]["bits"].period)
    assert blocks == 192 and up >= 10 and down >= 10 and per_bits == 192 * 64 - up + down
    if name == "timing_wraps":
        assert per_bits % 64 and P.odd_factor(per_bits) > 1                 # the unpack path
    else:
        assert up == down and per_bits == 12288
    _outputs(r, name, items=("soft",), bits=("bits",))
    assert r["nbits"](6) - r["nbits"](5) == per_bits


@pytest.mark.parametrize("name", ["ddc4", "ddc1"])
def test_ddc_units(name):
    r = _built(name)
    u = P.UNITS[name]
    p = r["p"]
    assert (u["fcw"] * p) % (1 << 24) == 0 and u["fcw"] % (1 << 24) != 0
    per = p // u["decim"]
    assert P.odd_factor(p) > 1 and P.odd_factor(per) > 1 and P.odd_factor(4 * per) > 1
    assert P.residues(p) == (8192, 4096)
    P.assert_shift_shows(r["unit"], name + " samples", least=0.999)
    for key in ("iq", "polar"):
        e = r["expect"][key]
        P.assert_shift_shows(e.period, f"{name} {key} pairs", least=0.99)
        P.assert_shift_shows(e.period.reshape(-1), f"{name} {key} int16 elements")
        assert not np.array_equal(e.head, e.period) and np.array_equal(e.head[16:], e.period[16:])      # the filter's history alone
    sat = np.abs(r["expect"]["iq"].period.astype(np.int64)) >= 32767
    assert sat.mean() < 0.01


def test_conv_units():
    r = _built("conv34")
    assert r["T"] == 960 and len(r["encode"].period) == 1280 and len(r["rx_unit"]) == 1280
    for n in (960, 1280, 960 // 64, 1280 // 64):                                 # bits and words, in and out
        assert P.odd_factor(n) > 1
    P.assert_shift_shows(r["data"], "conv34 data", group=64)
    P.assert_shift_shows(r["rx_unit"], "conv34 received bits", group=64)
    P.assert_shift_shows(r["encode"].period, "conv34 transmitted bits", group=64)
    P.assert_shift_shows(r["decode"].period, "conv34 decisions", group=64)
    assert r["errors"] == 0 and int((r["rx_unit"] != r["encode"].period).sum()) == 32
    assert not np.array_equal(r["encode"].head, r["encode"].period)              # the encoder leaves reset in period 0 alone
    s = _built("conv12")
    assert s["T"] == 960 and len(s["unit"]) == 1920 and P.odd_factor(1920) > 1 and P.odd_factor(2 * 1920) > 1
    P.assert_shift_shows(s["unit"], "conv12 values")
    P.assert_shift_shows(s["decode"].period, "conv12 decisions", group=64)
    assert s["errors"] == 0
    for c in (r, s):
        assert c["stats"](9)[0] - c["stats"](8)[0] == 5 and c["stats"](9)[1] - c["stats"](8)[1] == 960


def test_eye_counts_of_a_tiled_record():
    """eye_hist_tiled is the histogram of the record written out, for a period that is odd (every period starts in another
    column) and a first sample that is not 0."""
    rng = np.random.default_rng(3)
    unit = rng.integers(-2048, 2048, 1021).astype(np.int16)
    for first, n in ((0, 5 * 1021 + 77), (12345, 70 * 1021 + 1020), (7, 500)):
        rec = np.tile(unit, n // 1021 + 1)[:n]
        assert np.array_equal(P.eye_hist_tiled(unit, first, n), P.eye_hist(rec, first))
    assert P.eye_hist_tiled(unit, 0, 64 * 1021).sum() == 64 * 1021


def test_mlse_unit():
    import test_mlse_host
    r = _built("mlse")
    u = P.UNITS["mlse"]
    p = r["p"]
    assert test_mlse_host.mlse_shape(1 << (len(u["g"]) - 1), *u["geom"])[0] == 256 and len(u["g"]) - 1 == 2      # 256 threads, four states
    assert p == 1536 and p % u["geom"][0] == 0 and P.residues(p) == (512, 1024)
    assert P.odd_factor(p) > 1 and P.odd_factor(2 * p) > 1 and P.odd_factor(p // 64) > 1
    P.assert_shift_shows(r["unit"], "mlse samples", least=0.97)
    P.assert_shift_shows(r["expect"].period, "mlse decisions", group=64)
    assert 0.3 < r["expect"].period.mean() < 0.7
    assert r["stats"](9)[0] - r["stats"](8)[0] == p // 8 and r["stats"](9)[1] - r["stats"](8)[1] == p


@pytest.mark.parametrize("name", ["rs1", "rs2"])
def test_rs_units(name):
    r = _built(name)
    code = r["code"]
    nf = P.UNITS[name]["frames"]
    for nbytes in (nf * code.frame_bytes, nf * code.data_bytes, nf * code.depth):      # coded bytes, data bytes, status bytes
        assert P.odd_factor(nbytes) > 1
        assert 0 not in P.residues(nbytes)
    P.assert_shift_shows(r["recv"], name + " received bytes", least=0.99)
    P.assert_shift_shows(r["coded"], name + " coded bytes", least=0.99)
    P.assert_shift_shows(r["out"], name + " decoded bytes", least=0.99)
    P.assert_shift_shows(r["data"], name + " data bytes", least=0.99)
    P.assert_shift_shows(r["nerr"], name + " status bytes")
    codewords, clean, failed, symbols, bits = r["unit_stats"]
    assert codewords == nf * code.depth and clean >= 2 and failed >= 2 and codewords - clean - failed >= 40
    assert set(r["nerr"].tolist()) >= {0, 1, 16, 255}
    # a failed codeword's data pass through as they came, a corrected one's are the data
    ok = np.repeat(r["nerr"].reshape(nf, code.depth) != 255, 223, axis=0).reshape(nf, 223, code.depth).reshape(-1) if code.depth == 1 else None
    if ok is not None:
        assert np.array_equal(r["out"][ok], r["data"][ok]) and not np.array_equal(r["out"], r["data"])
    assert r["stats"](3) == [3 * a + b for a, b in zip(r["unit_stats"], r["stats"](0))]


def test_framesync_unit():
    t0 = time.time()
    r = P.framesync()
    sizes = [P.framesync(n) for n in (P.P32 + 3 * r["per"] + P.UNITS["framesync"]["tail_bits"], 1 << 35)]
    assert time.time() - t0 < 10.0
    cfg, per = r["cfg"], r["per"]
    assert cfg.F == 248 and per == 61 * 248 and per % 64 and P.odd_factor(per) > 1 and P.odd_factor(cfg.F) > 1
    assert len(r["words"]) == per and P.odd_factor(len(r["words"])) > 1                  # 64 periods are `per` words
    assert 0 not in P.residues(per) and 0 not in P.residues(61) and 0 not in P.residues(61 * 27)
    P.assert_shift_shows(r["unit"], "framesync bits", group=64)
    P.assert_shift_shows(r["payload"], "framesync payload bytes", least=0.99)
    # the meta words say little (most markers are clean): what a wrapped index does to them shows in the positions, which are
    # compared with j * frame_bits, and in the payloads; the meta words of a period do hold every kind
    kinds = set(r["expect"].period.tolist())
    assert kinds == {0x100, 0x101, 0x103, 0x100 | 0x200 | 10} and r["expect"].head[0] == 0x100 | 0x400
    assert r["per_period"][2:] == [61, 1, 0, 0, 0, 4]                                    # frames, flywheeled, ..., marker bit errors
    for s in sizes:
        assert s["K"] * per + s["tail"] in (P.P32 + 3 * per + P.UNITS["framesync"]["tail_bits"], 1 << 35)
        assert s["state"][2] == s["frames"] and s["state"][0] >> 32 == s["frames"] and s["state"][4] == 1 and s["state"][5] == 0
    assert sizes[1]["frames"] == (1 << 35) // 248
