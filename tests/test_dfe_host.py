"""The decision-feedback equalizer without a GPU: the model against the definition term by term, bbb_dfe_model_host against
the model, the argument checks of bbb_dfe_run through the C ABI, equalizer.dfe_taps, the kernels' per-symbol core and region
rules (basebandboard_amd/csrc/dfe_common.hpp) called from a restatement of the walk on the CPU under ASan/UBSan, and the closed
loop echo channel -> design -> equalize -> count on the CPU oracle's waveform."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib, equalizer
from conftest import ROOT

import fir_model
import grid
import dfe_model as M


def _cfg(taps, fb, spb=1, phase=0, threshold=0, strict=False, shift=0, out_bytes=2, region=0, warmup=0):
    c = _lib.DfeCfg()
    c.ff.ntaps = len(taps)
    for i, v in enumerate(taps):
        c.ff.taps[i] = v
    c.ff.shift, c.ff.decim, c.ff.phase, c.ff.out_bytes = shift, spb, phase, out_bytes
    c.nfb = len(fb)
    for i, v in enumerate(fb[:4]):
        c.fb[i] = v
    c.threshold, c.strict, c.region_symbols, c.warmup_symbols = threshold, int(strict), region, warmup
    return c


# ---- the model ---------------------------------------------------------------------------------------------------------

def test_model_equals_the_definition_term_by_term():
    rng = np.random.default_rng(1)
    for taps, fb, spb, phase, thr, strict, nb, state in (([3], [5], 1, 0, 0, False, 0, 0), ([2, -1, 4], [7, -3], 2, 1, 3, True, 2, 1),
                                                          ([1, 1, 1, 1], [40, 30, -20, 10], 4, 3, -5, False, 5, 9), ([5, 0, -2], [], 3, 2, 1, True, 0, 0),
                                                          ([9], [4, 4, 4], 1, 0, 0, False, 0, 7)):
        x = rng.integers(-12, 13, 41 + nb)
        before, rec = x[:nb], x[nb:]
        xe = lambda j: int(rec[j]) if j >= 0 else (int(before[nb + j]) if -j <= nb else 0)                # noqa: E731
        d, want_bits, want_v = {}, [], []
        for i in range(len(fb)):
            d[-1 - i] = 1 if state >> i & 1 else -1
        for k in range(fir_model.nout(len(rec), spb, phase)):
            n = phase + k * spb
            v = sum(h * xe(n - i) for i, h in enumerate(taps)) - sum(c * d[k - 1 - i] for i, c in enumerate(fb))
            b = v > thr if strict else v >= thr
            d[k] = 1 if b else -1
            want_bits.append(int(b))
            want_v.append(v)
        want_state = sum((d[len(want_bits) - 1 - i] > 0) << i for i in range(len(fb)))
        bits, soft, s = M.run(rec, taps, fb, spb, phase, thr, strict, before, state, 0, 4)
        assert bits.tolist() == want_bits and soft.tolist() == want_v and s == want_state, (taps, fb)
    # state bits from nfb on are ignored; sat16 and the shift of the int16 form
    assert M.run([1, -1, 1], [1], [2], 1, state=0xFFFFFFF0)[2] == M.run([1, -1, 1], [1], [2], 1)[2]
    assert M.soft(np.array([70000, -70000, 37, -37]), 0, 2).tolist() == [32767, -32768, 37, -37]
    assert M.soft(np.array([70000, -37]), 2, 2).tolist() == [17500, -10] and M.soft(np.array([70000]), 2, 4).tolist() == [70000]
    assert M.table([5, 3]) == [-8, 2, -2, 8] and M.table([]) == [0]


def test_nfb_0_is_the_filtered_slicer():
    rng = np.random.default_rng(2)
    x = rng.integers(-2000, 2000, 500)
    bits, _, s = M.run(x, [1, 2, -3, 4], [], 3, 1, 17, True)
    assert np.array_equal(bits, fir_model.decisions(x, [1, 2, -3, 4], 3, 1, 17, True)) and s == 0


def test_stream_equals_one_call():
    rng = np.random.default_rng(3)
    x = rng.integers(-300, 300, 700)
    taps, fb = [3, -1, 2, 5, 1], [400, -250, 100]
    want = M.run(x, taps, fb, 4, 2, 10, False, shift=1)
    got = M.stream(x, taps, fb, 4, [0, 1, 5, 64, 64, 333, 699], 2, 10, False, shift=1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


# ---- the host entry points ---------------------------------------------------------------------------------------------

def _model_host(x, nb, cfg, state, soft_dtype=None):
    lib = _lib.lib()
    x = np.ascontiguousarray(x, dtype=np.int16)
    nin = len(x) - nb
    nsym = fir_model.nout(nin, cfg.ff.decim, cfg.ff.phase)
    bits = np.full((nsym + 63) // 64, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    soft = None if soft_dtype is None else np.zeros(nsym, dtype=soft_dtype)
    st, got = C.c_uint32(state), C.c_uint64()
    rc = lib.bbb_dfe_model_host(C.c_void_p(x.ctypes.data + 2 * nb), nin, nb, C.byref(cfg), C.byref(st), C.c_void_p(bits.ctypes.data),
                                None if soft is None else C.c_void_p(soft.ctypes.data), C.byref(got))
    assert rc == 0 and got.value == nsym
    return np.unpackbits(bits.view(np.uint8), bitorder="little")[:nsym], bits, soft, st.value


def test_model_host_equals_the_model():
    rng = np.random.default_rng(4)
    for nfb, spb, phase, nb, n, thr, strict in ((0, 1, 0, 0, 100, 0, False), (1, 8, 3, 4, 1000, 50, True), (2, 3, 2, 20, 777, -9, False),
                                                (3, 2, 1, 1, 129, 0, True), (4, 256, 255, 7, 5000, 1, False), (4, 1, 0, 0, 64, 0, False), (2, 5, 4, 0, 3, 0, False)):
        taps = rng.integers(-200, 200, 9).tolist()
        fb = rng.integers(-100000, 100000, nfb).tolist()
        x = rng.integers(-32768, 32768, n + nb).astype(np.int16)
        state = int(rng.integers(0, 1 << 32))
        for ob, dt in ((2, np.int16), (4, np.int32)):
            cfg = _cfg(taps, fb, spb, phase, thr, strict, shift=5, out_bytes=ob)
            bits, words, soft, s = _model_host(x, nb, cfg, state, dt)
            wb, ws, wst = M.run(x[nb:], taps, fb, spb, phase, thr, strict, x[:nb], state, 5, ob)
            assert np.array_equal(bits, wb) and np.array_equal(soft, ws) and s == wst, (nfb, spb)
            assert np.array_equal(words, fir_model.pack(wb))                     # the unused bits of the last word are 0


def test_geometry():
    for spb, sym in ((1, 2048), (2, 1024), (3, 683), (8, 256), (256, 8)):
        g = bbb.dfe.geometry(spb)
        assert g == dict(step_samples=2048, step_symbols=sym, wave_symbols=512 if spb == 1 else 64, region_symbols=4096, warmup_symbols=64)
    with pytest.raises(ValueError, match="decim"):
        bbb.dfe.geometry(0)
    assert _lib.lib().bbb_dfe_geometry(8, None, None, None, None, None) == 0


def test_invalid_arguments_return_before_the_device_is_touched():
    """Every pointer here is a number no device ever gave out: a call that got as far as the device would fail otherwise
    (BBB_ENODEV on a machine without a GPU), and the last case shows that a valid call does get that far."""
    import torch
    lib = _lib.lib()
    IN, BITS, SOFT, STATE = 1 << 20, 1 << 24, 1 << 26, 1 << 28

    def rc(cfg, in_dev=IN, nin=4096, nb=0, state=STATE, bits=BITS, soft=None, stats=None):
        return lib.bbb_dfe_run(C.c_void_p(in_dev), nin, nb, C.byref(cfg) if cfg is not None else None, C.c_void_p(state), C.c_void_p(bits),
                               C.c_void_p(soft) if soft else None, C.c_void_p(stats) if stats else None, None, 0, None)

    good = _cfg([1, 1, 1, 1], [100, 50], 8, 3)
    bad = []
    c = _cfg([1], [1, 1, 1, 1], 1)
    c.nfb = 5
    bad.append((c, {}, "nfb"))
    bad.append((_cfg([32767, 32767], [2 ** 31 - 1 - 32768 * 65534 + 1], 1), {}, "2\\^31"))           # one over the int32 bound
    bad.append((_cfg([1], [2 ** 31 - 1, 1], 1), {}, "2\\^31"))
    bad.append((_cfg([32767, 32767, 2], [], 1), {}, "65535"))                                          # a bad ff: the FIR's own rule
    c = _cfg([1], [3], 1)
    c.ff.ntaps = 0
    bad.append((c, {}, "ntaps"))
    bad.append((_cfg([1], [3], 0), {}, "decim"))
    bad.append((_cfg([1], [3], 4, 4), {}, "phase"))
    bad.append((_cfg([1], [3], 1, out_bytes=3), dict(soft=SOFT), "out_bytes"))
    bad.append((_cfg([1], [3], 1, shift=32), dict(soft=SOFT), "shift"))
    bad.append((None, {}, "null"))
    bad.append((good, dict(state=0), "state_dev"))
    bad.append((good, dict(bits=0), "bits_packed_dev"))
    bad.append((good, dict(in_dev=0), "in_dev"))
    bad.append((good, dict(bits=BITS + 4), "misaligned"))
    bad.append((good, dict(soft=SOFT + 1), "misaligned"))
    bad.append((good, dict(bits=IN + 4096 * 2 - 8), "bits_packed_dev overlaps"))                       # the last samples
    bad.append((good, dict(bits=IN - 64, nb=3), "bits_packed_dev overlaps"))                            # the history
    bad.append((good, dict(soft=IN + 64), "soft_dev overlaps"))
    bad.append((good, dict(soft=BITS + 8), "soft_dev overlaps bits_packed_dev"))
    bad.append((_cfg([1], [3], 1, region=1), dict(in_dev=1 << 32, nin=1 << 27), "regions"))
    for cfg, kw, what in bad:
        assert rc(cfg, **kw) == _lib.BBB_EINVAL, what
        assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    # exactly at the bound, and outputs next to the samples but not in them: valid
    assert bbb.DFE([32767, 32767], [2 ** 31 - 1 - 32768 * 65534], 1).fb == [65535]
    if not torch.cuda.is_available():
        assert rc(_cfg([32767, 32767], [2 ** 31 - 1 - 32768 * 65534], 1)) == _lib.BBB_ENODEV
        assert rc(good, bits=IN + 4096 * 2, soft=IN - 512 * 2) == _lib.BBB_ENODEV
        assert rc(good, bits=IN - 64, nb=0) == _lib.BBB_ENODEV


def test_python_argument_checks():
    with pytest.raises(ValueError, match="at most 4"):
        bbb.DFE([1], [1] * 5, 8)
    with pytest.raises(ValueError, match="2\\^31"):
        bbb.DFE([32767, 32767], [65536], 1)
    with pytest.raises(ValueError, match="phase"):
        bbb.DFE([1], [1], 8, phase=8)
    with pytest.raises(ValueError, match="int32"):
        bbb.DFE([1], [2 ** 31], 8)
    d = bbb.DFE(bbb.FIR([1, 2, 3], shift=2), [7, -7], 8, 5, threshold=3, strict=True)
    c = d._cfg()
    assert (c.ff.ntaps, c.ff.shift, c.ff.decim, c.ff.phase, c.nfb, list(c.fb), c.threshold, c.strict) == (3, 2, 8, 5, 2, [7, -7, 0, 0], 3, 1)
    assert d.stats() == dict(regions=0, not_proven=0, repaired=0, symbols=0)
    with pytest.raises(ValueError, match="not both"):
        bbb.RX(7, 8, 0).slice(None, rx_filter=bbb.FIR([1]), dfe=d)


# ---- the design ----------------------------------------------------------------------------------------------------------

def test_dfe_taps():
    rng = np.random.default_rng(5)
    h = np.convolve(np.hanning(17), [1.0, 0, 0, 0, 0, 0, 0, 0, 0.6]) * 100
    for cursor, ntaps, s2 in ((8, 12, 0.5), (11, 9, 3.0), (8, 1, 0.0)):
        ff, fb, delay = equalizer.dfe_taps(h, 8, cursor, ntaps, 0, s2)
        taps, d0 = equalizer.mmse_taps(h, 8, cursor, ntaps, s2)
        assert np.array_equal(ff, taps) and delay == d0 and ff.dtype == np.int16 and len(fb) == 0
    # main path plus an echo one bit later: fb[0] is what the integer feed-forward filter makes of the echo
    spb, g = 4, 0.7
    h2 = np.zeros(3 * spb)
    h2[:spb] = 400.0
    h2[spb:2 * spb] = g * 400.0
    cursor = spb - 1
    ff, fb, delay = equalizer.dfe_taps(h2, spb, cursor, spb, 1, 100.0)
    assert delay == cursor - 0 and len(fb) == 1
    echo = sum(int(ff[j]) * h2[cursor - j + spb] for j in range(spb))
    assert fb[0] == int(np.rint(echo)) and fb[0] == int(np.rint(g * 400.0 * int(ff.sum())))
    # with the echo handed to the feedback nothing but noise is left: the matched filter, flat over the bit
    assert ff.tolist() == [256] * spb
    # two feedback taps see two post-cursors; lags beyond the pulse count as 0
    h3 = rng.normal(size=40)
    h3[10] = 9.0
    ff, fb, _ = equalizer.dfe_taps(h3, 8, 12, 6, 4, 0.1)
    for i in range(4):
        want = sum(int(ff[j]) * (h3[12 - j + 8 * (i + 1)] if 12 - j + 8 * (i + 1) < 40 else 0.0) for j in range(6))
        assert fb[i] == int(np.rint(want))
    with pytest.raises(ValueError, match="nfb"):
        equalizer.dfe_taps(h, 8, 8, 4, 5, 0.1)
    d = bbb.DFE.mmse(h2, spb, cursor, spb, 1, 100.0, phase=3, threshold=2)
    assert d.ff.taps == equalizer.dfe_taps(h2, spb, cursor, spb, 1, 100.0)[0].tolist() and d.design_delay == cursor and (d.spb, d.phase, d.threshold) == (spb, 3, 2)


# ---- the kernels' core on the CPU, under the sanitizers ------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("dfe_host")
    exe = d / "dfe_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", str(ROOT / "tests" / "dfe_host.cpp"), "-o", str(exe)])
    return exe


def _blob(c):
    fb = list(c["fb"]) + [0] * (4 - len(c["fb"]))
    head = np.array([len(c["a"]), len(c["fb"])] + fb + [c["threshold"], int(c["strict"]), c["state"], c["region"], c["warmup"], c["spb"], c["phase"], 0],
                    dtype=np.int64)
    a = np.zeros((len(c["a"]) + 1) // 2 * 2, dtype=np.int32)
    a[:len(c["a"])] = c["a"]
    return head.tobytes() + a.tobytes()


def _host_cases():
    rng = np.random.default_rng(6)
    cases = []

    def add(a, fb, region, warmup, spb=8, phase=0, threshold=0, strict=False, state=0):
        cases.append(dict(a=np.asarray(a, dtype=np.int64), fb=fb, region=region, warmup=warmup, spb=spb, phase=phase, threshold=threshold,
                          strict=strict, state=state))

    for nfb in range(5):
        bound = 2 ** 31 - 1 - 32768 * 65535
        for fb in (rng.integers(-300, 300, nfb).tolist(), [int(v) for v in rng.multinomial(bound, [1 / max(nfb, 1)] * max(nfb, 1))[:nfb] * rng.choice([-1, 1], nfb)]):
            # noisy data around the taps' scale: some starts proven, some speculated, some repaired
            scale = max(1, sum(abs(v) for v in fb))
            a = rng.integers(-2 * scale - 1, 2 * scale + 2, 3000)
            add(a, fb, 37, 5, spb=int(rng.choice([1, 2, 3, 8, 256])), phase=0, threshold=int(rng.integers(-3, 4)), strict=bool(nfb & 1), state=int(rng.integers(0, 16)))
    # all ambiguous: every decision the inverse of the last, odd regions, nothing proven, every other start wrong
    add(np.zeros(5000), [5], 37, 64, spb=1)
    add(np.zeros(2100), [5], 333, 7, spb=3, phase=2, state=1)
    # full-scale sums at the int32 bound
    add(rng.choice([-32768 * 65535, 32767 * 65535], 1500), [bound], 100, 3, spb=2, phase=1)
    # ambiguous stretches longer than the warm-up across a region, a step and a wave boundary (spb 8: 256 symbols per step)
    for at in (370, 512, 576):
        a = rng.choice([-1000, 1000], 1200)
        a[at - 40:at + 40] = 0
        add(a, [5, -2], 370, 16, spb=8)
    add([], [5], 10, 2)                                                          # nothing: the state word is masked
    add([7], [5, 1, 1, 1], 10, 2, state=0xFFFF)
    add(rng.integers(-50, 50, 64 * 9 + 1), [20, 10, 5, 2], 64, 64, spb=1)        # regions of whole words
    add(rng.integers(-50, 50, 5000), [20, 10, 5, 2], 4096, 64, spb=1, state=5)   # the defaults
    return cases


def test_lane_core_on_the_cpu_equals_the_model(host_exe, tmp_path):
    cases = _host_cases()
    (tmp_path / "c.bin").write_bytes(b"".join(_blob(c) for c in cases))
    r = subprocess.run([str(host_exe), str(tmp_path / "c.bin"), str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"cases {len(cases)}" in r.stdout, r.stderr[-3000:]
    lines = (tmp_path / "o.txt").read_text().split("\n")
    repaired = unproven = 0
    for i, c in enumerate(cases):
        bits, v, s, _ = M.decide(c["a"], c["fb"], c["threshold"], c["strict"], c["state"])
        st = M.replay(c["a"], c["fb"], c["threshold"], c["strict"], c["state"], c["region"], c["warmup"])
        head = [int(t) for t in lines[3 * i].split()]
        assert head == [s, st["regions"], st["not_proven"], st["repaired"], st["symbols"]], (i, head, s, st)
        assert [int(t, 16) for t in lines[3 * i + 1].split()] == fir_model.pack(bits).tolist(), i
        assert [int(t) for t in lines[3 * i + 2].split()] == v.tolist(), i
        repaired += st["repaired"]
        unproven += st["not_proven"]
    # the cases do reach the speculation and the repair
    st = M.replay(cases[10]["a"], cases[10]["fb"], region=37, warmup=64)
    assert st["not_proven"] == st["regions"] - 1 and st["repaired"] > st["regions"] // 3
    assert repaired > 100 and unproven > repaired


# ---- the closed loop on the CPU ----------------------------------------------------------------------------------------

def test_closed_loop_on_the_oracle_waveform(oracle):
    """The oracle's waveform through an echo one bit late: the best linear receiver (mmse_taps, 12 taps) leaves errors at the
    cursor's phase, the DFE designed from the same pulse, with one feedback tap, strictly fewer."""
    L = M.LOOP
    y, h, sigma2, ref = M.loop_record(oracle)
    phase = (17 + L["cursor"]) % 8
    lin, _ = equalizer.mmse_taps(h, 8, L["cursor"], L["nff"], sigma2)
    ff, fb, delay = equalizer.dfe_taps(h, 8, L["cursor"], L["nff"], L["nfb"], sigma2)
    e_lin, n_lin = M.loop_errors(fir_model.decisions(y, lin.tolist(), 8, phase), ref)
    e_dfe, n_dfe = M.loop_errors(M.run(y, ff.tolist(), fb.tolist(), 8, phase)[0], ref)
    print("noise power", sigma2, "linear", lin.tolist(), e_lin, "ff", ff.tolist(), "fb", fb.tolist(), e_dfe, "of", n_dfe)
    assert lin.tolist() == M.LOOP_LINEAR_TAPS and ff.tolist() == M.LOOP_FF and fb.tolist() == M.LOOP_FB
    assert n_lin == n_dfe == M.LOOP_BITS
    assert (e_lin, e_dfe) == (M.LOOP_LINEAR_ERRORS, M.LOOP_DFE_ERRORS)
    assert e_lin > 0 and e_dfe < e_lin
    # the raw slicer at the pulse's peak, for scale
    assert M.loop_errors(fir_model.decisions(y, [1], 8, (17 + int(np.abs(h).argmax())) % 8), ref)[0] > e_lin


# ---- past one pass of the grids ----------------------------------------------------------------------------------------------------
# The region kernel takes a region a turn and the repair kernel a region that started wrong, each at most 8 workgroups per
# compute unit at a time (tests/grid.py).  At 16 symbols a region these records are short enough for the model itself, so
# tests/test_gpu_dfe.py holds the GPU to tests/dfe_model.py over the whole of them; here the model says that they do what they
# are for.
MULTIPASS_REGION = 16
MULTIPASS_NOISY = dict(fb=[280, 100, -50], warmup=3)
MULTIPASS_ZERO = dict(taps=[3, -2, 1], fb=[5], warmup=7)


def multipass_noisy(spb, ncus):
    """(samples, taps, fb, phase) of 2 * 8 * ncus + 5 regions, the last cut short: two-level data with an echo of 0.7 one symbol
    late and noise, through a moving average of the symbol's samples."""
    nsym = MULTIPASS_REGION * (grid.passes(grid.DFE, ncus=ncus) - 1) + 9
    rng = np.random.default_rng(60 + spb)
    d = rng.choice([-400, 400], nsym)
    sym = d + np.concatenate([[0], (d[:-1] * 0.7).astype(np.int64)])
    x = np.repeat(sym, spb) // spb + rng.normal(0, 150 / spb, nsym * spb).astype(np.int64)
    return x.astype(np.int16), [1] * spb, MULTIPASS_NOISY["fb"], spb - 1


def multipass_zero(spb, ncus):
    """All-zero samples under fb = {5}: every decision is the inverse of the last, no warm-up proves a start, and with an odd
    warm-up the speculation from state 0 fails for every other region.  2 * (2 * 8 * ncus + 5) + 3 regions, so that the regions
    to repair are more than two passes of the repair kernel's grid."""
    nreg = 2 * grid.passes(grid.DFE, ncus=ncus) + 3
    return np.zeros((MULTIPASS_REGION * (nreg - 1) + 5) * spb, dtype=np.int16)


@pytest.mark.parametrize("spb", (1, 2))
def test_multipass_records_in_the_model(spb):
    ncus = 256
    x, taps, fb, phase = multipass_noisy(spb, ncus)
    a = fir_model.acc(x, taps)[phase::spb]
    st = M.replay(a, fb, 0, False, 5, MULTIPASS_REGION, MULTIPASS_NOISY["warmup"])
    assert st["regions"] == grid.passes(grid.DFE, ncus=ncus) and st["symbols"] % MULTIPASS_REGION and 0 < st["repaired"] <= st["not_proven"] < st["regions"]
    bits = M.decide(a, fb, 0, False, 5)[0]
    assert 0.4 < bits.mean() < 0.6
    z = multipass_zero(spb, ncus)
    a = fir_model.acc(z, MULTIPASS_ZERO["taps"])[spb - 1::spb]
    st = M.replay(a, MULTIPASS_ZERO["fb"], 0, False, 0, MULTIPASS_REGION, MULTIPASS_ZERO["warmup"])
    assert st["not_proven"] == st["regions"] - 1 and st["repaired"] > 2 * grid.DFE * ncus
