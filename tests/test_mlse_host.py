"""The Viterbi sequence detector without a GPU: the model against exhaustive search and its pinned tie rules, bbb_mlse_model_host
and bbb_mlse_plan against the model, the argument checks of bbb_mlse_run through the C ABI, the stream's cutting in the model,
equalizer.mlse_target, the kernel's per-window core (basebandboard_amd/csrc/mlse_common.hpp) called from a restatement of the
kernel's walk on the CPU under ASan/UBSan, and the closed loop channel -> design -> detect -> count on the CPU oracle's
waveform."""
import ctypes as C
import itertools
import re
import subprocess

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib, equalizer
from conftest import ROOT

import fir_model
import grid
import dfe_model
import mlse_model as M


def _cfg(taps, g, spb=1, phase=0, shift=0, init_state=0, B=0, W=0, D=0, out_bytes=2):
    c = _lib.MlseCfg()
    c.ff.ntaps = len(taps)
    for i, v in enumerate(taps):
        c.ff.taps[i] = v
    c.ff.shift, c.ff.decim, c.ff.phase, c.ff.out_bytes = shift, spb, phase, out_bytes
    c.mem = len(g) - 1
    for i, v in enumerate(g[:5]):
        c.g[i] = v
    c.init_state, c.block_symbols, c.warmup_symbols, c.lookahead_symbols = init_state, B, W, D
    return c


# ---- the model ---------------------------------------------------------------------------------------------------------

def test_model_finds_the_maximum_over_all_sequences():
    """One window over everything: the path's total gain is the maximum over all 2^9 sequences from init_state.  Gains are
    compared, not bits: ties exist."""
    rng = np.random.default_rng(1)
    for case in range(60):
        mem = 1 + case % 3
        g = rng.integers(-6, 7, mem + 1).tolist()
        y = rng.integers(-8, 9, 9)
        init = int(rng.integers(0, 1 << mem))
        bits, total = M.viterbi(y, g, init)
        assert total == M.path_gain(y, g, bits, init), (case, "the traced-back path does not earn the metric")
        assert total == max(M.path_gain(y, g, seq, init) for seq in itertools.product((0, 1), repeat=9)), case
        d, w = M.decide(y, 0, g, init_state=init, B=9, W=1, D=1)
        assert d.tolist() == bits and w == 1


def test_tie_rules_on_all_zero_records():
    # every gain is -s^2: g = {3, 3} makes s = 0 where the bit differs from the last, so the path alternates from init_state 0
    assert M.decide(np.zeros(12, dtype=np.int64), 0, [3, 3], init_state=0, B=12, W=1, D=1)[0].tolist() == [1, 0] * 6
    # g = {3, -3, 0}: s = 0 where the bit repeats the last; from state 1 (last bit 1) all ones
    assert M.decide(np.zeros(12, dtype=np.int64), 0, [3, -3, 0], init_state=1, B=12, W=1, D=1)[0].tolist() == [1] * 12
    # every ACS ties (g = 0): c = 0 survives everywhere and the lowest end state wins, so all zeros, from any init_state
    assert not M.decide(np.zeros(40, dtype=np.int64), 0, [0, 0, 0], init_state=3, B=5, W=2, D=3)[0].any()
    # a window that does not start at symbol 0 forgets init_state: two candidates tie at the end, the lowest state wins
    bits, w = M.decide(np.zeros(20, dtype=np.int64), 0, [3, 3], init_state=0, B=5, W=2, D=3)
    assert w == 4 and bits[:5].tolist() == [1, 0, 1, 0, 1]


def test_non_final_rule_and_plan_arithmetic():
    assert M.ndecided(1000, 0, False) == 960 and M.ndecided(1000, 0, True) == 1000
    assert M.ndecided(223, 0, False) == 0 and M.ndecided(224, 0, False) == 192
    assert M.ndecided(7, 0, False, 5, 2, 3) == 0 and M.ndecided(8, 0, False, 5, 2, 3) == 5 and M.ndecided(100, 95, False, 5, 2, 3) == 95
    assert M.ndecided(10, 192, False) == 0 and M.ndecided(300, 192, False) == 192
    assert M.nbefore_wanted(0, 8, 12, 3) == 8 and M.nbefore_wanted(192, 8, 12, 3) == 32 * 8 + 11 - 3
    assert M.nbefore_wanted(10, 8, 12, 0, 5, 2, 3) == 2 * 8 + 11 and M.nbefore_wanted(12, 8, 12, 0, 5, 2, 3) == 4 * 8 + 11
    assert M.nbefore_wanted(3, 8, 1, 7, 5, 2, 3) == 3 * 8 - 7 and M.nbefore_wanted(0, 8, 1, 7) == 0


def test_stream_equals_one_call_in_the_model():
    rng = np.random.default_rng(3)
    x = rng.integers(-300, 300, 700)
    taps, g = [3, -1, 2, 5, 1], [400, -250, 100]
    for geom in ((0, 0, 0), (5, 2, 3), (64, 128, 1)):
        want, _ = M.run(x, taps, g, 4, 2, 1, B=geom[0], W=geom[1], D=geom[2])
        got = M.stream(x, taps, g, 4, [0, 1, 5, 64, 64, 333, 699], 2, 1, B=geom[0], W=geom[1], D=geom[2])
        assert np.array_equal(got, want), geom


# ---- the host entry points ---------------------------------------------------------------------------------------------

def _model_host(x, nb, cfg, first=0, final=True):
    lib = _lib.lib()
    x = np.ascontiguousarray(x, dtype=np.int16)
    nin = len(x) - nb
    nsym, nd, _ = M.plan(nin, cfg.ff.decim, cfg.ff.phase, cfg.ff.ntaps, first, final, cfg.block_symbols, cfg.warmup_symbols, cfg.lookahead_symbols)
    bits = np.full((nd + 63) // 64 + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    got = C.c_uint64()
    rc = lib.bbb_mlse_model_host(C.c_void_p(x.ctypes.data + 2 * nb), nin, nb, first, int(final), C.byref(cfg), C.c_void_p(bits.ctypes.data), C.byref(got))
    assert rc == 0 and got.value == nd, lib.bbb_last_error_detail()
    assert bits[-1] == 0xA5A5A5A5A5A5A5A5, "a word beyond ceil(ndecided / 64) was written"
    return np.unpackbits(bits[:-1].view(np.uint8), bitorder="little")[:nd], bits[:-1]


def test_model_host_equals_the_model():
    rng = np.random.default_rng(4)
    for mem in (1, 2, 3, 4):
        for spb in (1, 2, 3, 8):
            for B, W, D in ((5, 2, 3), (0, 0, 0)):
                for first, nb in ((0, 0), (7, 40), (200, 3), (192, 600)):
                    taps = rng.integers(-20, 20, 5).tolist()
                    g = rng.integers(-300, 300, mem + 1).tolist()
                    x = rng.integers(-300, 300, 1000 + nb)
                    phase, final, init = int(rng.integers(0, spb)), bool(rng.integers(0, 2)), int(rng.integers(0, 16))
                    want, _ = M.run(x[nb:], taps, g, spb, phase, 1, x[:nb], first, final, init, B, W, D)
                    got, words = _model_host(x, nb, _cfg(taps, g, spb, phase, 1, init, B, W, D), first, final)
                    assert np.array_equal(got, want), (mem, spb, B, first, nb, final)
                    assert np.array_equal(words, fir_model.pack(want))           # the unused bits of the last word are 0
    # y saturates at both ends, g at its bound
    taps, g = [32767, 32767], [1 << 19, -(1 << 18), 1 << 18]
    x = rng.choice([-32768, 32767], 600)
    want, _ = M.run(x, taps, g, 2, 1, 3, B=64, W=7, D=9)
    assert np.array_equal(_model_host(x, 0, _cfg(taps, g, 2, 1, 3, 0, 64, 7, 9))[0], want)
    assert set(M.y_values(x, taps, 2, 1, 3, (), 0, 300).tolist()) >= {-32768, 32767}
    # the tie rules through the C model
    z = np.zeros(12, dtype=np.int16)
    assert _model_host(z, 0, _cfg([1], [3, 3], B=12, W=1, D=1))[0].tolist() == [1, 0] * 6
    assert _model_host(z, 0, _cfg([1], [3, -3, 0], init_state=1, B=12, W=1, D=1))[0].tolist() == [1] * 12


def test_plan_equals_the_model():
    lib = _lib.lib()
    rng = np.random.default_rng(5)
    for _ in range(300):
        B, W, D = ((0, 0, 0), (5, 2, 3), (64, 128, 128), (256, 128, 128), (1, 1, 1))[int(rng.integers(0, 5))]
        spb = int(rng.choice([1, 2, 3, 8, 256]))
        phase, ntaps = int(rng.integers(0, spb)), int(rng.integers(1, 40))
        nin, first, final = int(rng.integers(0, 5000)), int(rng.choice([0, 1, 5, 191, 192, 193, 1000, 1 << 40])), bool(rng.integers(0, 2))
        v = [C.c_uint64() for _ in range(3)]
        assert lib.bbb_mlse_plan(C.byref(_cfg([1] * ntaps, [1, 1], spb, phase, B=B, W=W, D=D)), nin, first, int(final), *[C.byref(t) for t in v]) == 0
        assert tuple(t.value for t in v) == M.plan(nin, spb, phase, ntaps, first, final, B, W, D), (B, spb, phase, nin, first, final)
    assert lib.bbb_mlse_plan(C.byref(_cfg([1], [1, 1])), 100, 0, 1, None, None, None) == 0
    m = bbb.MLSE([1] * 12, [5, 4], 8, phase=3)
    assert m.plan(8000) == (1000, 1000, 8) and m.plan(8000, final=False) == (1000, 960, 8) and m.plan(8000, 192, False)[2] == 264


def test_invalid_arguments_return_before_the_device_is_touched():
    """Every pointer here is a number no device ever gave out: a call that got as far as the device would fail otherwise
    (BBB_ENODEV on a machine without a GPU), and the last cases show that a valid call does get that far."""
    import torch
    lib = _lib.lib()
    IN, BITS, STATS = 1 << 20, 1 << 24, 1 << 28

    def rc(cfg, in_dev=IN, nin=4096, nb=0, first=0, final=1, bits=BITS, stats=None):
        return lib.bbb_mlse_run(C.c_void_p(in_dev), nin, nb, first, final, C.byref(cfg) if cfg is not None else None, C.c_void_p(bits),
                                C.c_void_p(stats) if stats else None, None, 0, None)

    good = _cfg([1, 1, 1, 1], [100, 50], 8, 3)
    bad = [(None, {}, "null")]
    for mem in (0, 5):
        c = _cfg([1], [1, 1], 1)
        c.mem = mem
        bad.append((c, {}, "mem"))
    bad.append((_cfg([1], [1 << 19, (1 << 19) + 1], 1), {}, "2\\^20"))                                  # one over the bound
    bad.append((_cfg([1], [1 << 18, -(1 << 18), 1 << 18, -(1 << 18), 1], 1), {}, "2\\^20"))
    bad.append((_cfg([32767, 32767, 2], [1, 1], 1), {}, "65535"))                                       # a bad ff: the FIR's own rules
    c = _cfg([1], [3, 1], 1)
    c.ff.ntaps = 0
    bad.append((c, {}, "ntaps"))
    bad.append((_cfg([1], [3, 1], 0), {}, "decim"))
    bad.append((_cfg([1], [3, 1], 4, 4), {}, "phase"))
    bad.append((_cfg([1], [3, 1], 1, shift=32), {}, "shift"))
    bad.append((_cfg([1], [3, 1], 1, out_bytes=3), {}, "out_bytes"))
    bad.append((_cfg([1], [3, 1], 1, W=129), {}, "warmup"))
    bad.append((_cfg([1], [3, 1], 1, D=129), {}, "lookahead"))
    bad.append((_cfg([1], [3, 1], 1, B=449), {}, "512"))                                                # 449 + 32 + 32
    bad.append((_cfg([1], [3, 1], 1, B=513, W=1, D=1), {}, "512"))
    bad.append((good, dict(in_dev=0), "in_dev"))
    bad.append((good, dict(bits=0), "bits_packed_dev"))
    bad.append((good, dict(bits=BITS + 4), "misaligned"))
    bad.append((good, dict(in_dev=IN + 1), "misaligned"))
    bad.append((good, dict(stats=STATS + 4), "misaligned"))
    bad.append((good, dict(bits=IN + 4096 * 2 - 8), "bits_packed_dev overlaps"))                        # the last samples
    bad.append((good, dict(bits=IN - 64, nb=40, first=192), "bits_packed_dev overlaps"))                # the history the window reaches
    bad.append((good, dict(first=(1 << 58) - 511), "2\\^58"))
    bad.append((good, dict(first=1 << 63), "2\\^58"))
    for cfg, kw, what in bad:
        assert rc(cfg, **kw) == _lib.BBB_EINVAL, what
        assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    # exactly at the bounds, and an output next to the samples but not in them: valid
    assert bbb.MLSE([1], [1 << 19, 1 << 19], 1, block_symbols=256, warmup_symbols=128, lookahead_symbols=128).mem == 1
    if not torch.cuda.is_available():
        assert rc(_cfg([1], [1 << 19, 1 << 19], 1, B=448)) == _lib.BBB_ENODEV
        assert rc(good, bits=IN + 4096 * 2) == _lib.BBB_ENODEV
        assert rc(good, bits=IN - 64, nb=40, first=0) == _lib.BBB_ENODEV          # at symbol 0 only the taps' three samples are read
        assert rc(good, first=(1 << 58) - 512) == _lib.BBB_ENODEV


def test_python_argument_checks():
    with pytest.raises(ValueError, match="2..5"):
        bbb.MLSE([1], [1], 8)
    with pytest.raises(ValueError, match="2..5"):
        bbb.MLSE([1], [1] * 6, 8)
    with pytest.raises(ValueError, match="2\\^20"):
        bbb.MLSE([1], [1 << 20, 1], 8)
    with pytest.raises(ValueError, match="phase"):
        bbb.MLSE([1], [1, 1], 8, phase=8)
    with pytest.raises(ValueError, match="512"):
        bbb.MLSE([1], [1, 1], 8, block_symbols=500)
    d = bbb.MLSE(bbb.FIR([1, 2, 3], shift=2), [7, -7, 1], 8, 5, init_state=2, block_symbols=5, warmup_symbols=2, lookahead_symbols=3)
    c = d._cfg()
    assert (c.ff.ntaps, c.ff.shift, c.ff.decim, c.ff.phase, c.mem, list(c.g), c.init_state) == (3, 2, 8, 5, 2, [7, -7, 1, 0, 0], 2)
    assert (c.block_symbols, c.warmup_symbols, c.lookahead_symbols) == (5, 2, 3) and d.stats() == dict(windows=0, symbols=0)
    rx = bbb.RX(7, 8, 0)
    for kw in (dict(dfe=bbb.DFE([1], [1], 8)), dict(rx_filter=bbb.FIR([1]))):
        with pytest.raises(ValueError, match="not both"):
            rx.slice(None, mlse=d, **kw)
        with pytest.raises(ValueError, match="not both"):
            rx.count_errors(None, mlse=d, **kw)
        with pytest.raises(ValueError, match="not both"):
            rx.detect(None, mlse=d, **kw)


# ---- the design ----------------------------------------------------------------------------------------------------------

def test_mlse_target():
    h = np.convolve(np.hanning(17), [1.0, 0, 0, 0, 0, 0, 0, 0, 0.6]) * 100
    for cursor, nff, mem, s2 in ((8, 12, 1, 0.5), (11, 9, 2, 3.0), (9, 6, 4, 0.1)):
        ff, fb, _ = equalizer.dfe_taps(h, 8, cursor, nff, mem, s2)
        for shift in (None, 0, 3):
            f2, g, sh = equalizer.mlse_target(h, 8, cursor, nff, mem, s2, shift)
            assert np.array_equal(f2, ff) and f2.dtype == np.int16 and len(g) == mem + 1
            main = sum(int(ff[j]) * h[cursor - j] for j in range(nff) if 0 <= cursor - j < len(h))
            assert g[0] == int(np.rint(main / 2 ** sh)) and g[1:].tolist() == np.rint(fb / 2.0 ** sh).astype(np.int64).tolist()
            if shift is None:
                assert int(np.abs(g).sum()) <= 16383
                assert sh == 0 or int(np.abs(equalizer.mlse_target(h, 8, cursor, nff, mem, s2, sh - 1)[1]).sum()) > 16383
            else:
                assert sh == shift
    # main path plus an echo one bit later: the target IS the two paths, as the integer filter passes them
    spb, echo = 4, 0.7
    h2 = np.zeros(3 * spb)
    h2[:spb] = 400.0
    h2[spb:2 * spb] = echo * 400.0
    ff, g, sh = equalizer.mlse_target(h2, spb, spb - 1, spb, 1, 100.0)
    assert ff.tolist() == [256] * spb and sh == 6
    assert g.tolist() == [int(np.rint(400.0 * 1024 / 64)), int(np.rint(echo * 400.0 * 1024 / 64))] and abs(g[1] / g[0] - echo) < 1e-3
    with pytest.raises(ValueError, match="mem"):
        equalizer.mlse_target(h, 8, 8, 4, 5, 0.1)
    with pytest.raises(ValueError, match="mem"):
        equalizer.mlse_target(h, 8, 8, 4, 0, 0.1)
    d = bbb.MLSE.mmse(h2, spb, spb - 1, spb, 1, 100.0, phase=3, block_symbols=64)
    assert (d.ff.taps, d.ff.shift, d.g, d.spb, d.phase, d.design_delay, d.block_symbols) == ([256] * spb, 6, g.tolist(), spb, 3, spb - 1, 64)


# ---- the kernel's core on the CPU, under the sanitizers ------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("mlse_host")
    exe = d / "mlse_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", str(ROOT / "tests" / "mlse_host.cpp"), "-o", str(exe)])
    return exe


def _blob(c):
    g = list(c["g"]) + [0] * (5 - len(c["g"]))
    head = np.array([len(c["y"]), -c["k_lo"], len(c["g"]) - 1] + g + [c["init"], c["B"], c["W"], c["D"], c["first"], int(c["final"]), c["threads"], 0],
                    dtype=np.int64)
    y = np.zeros((len(c["y"]) + 1) // 2 * 2, dtype=np.int32)
    y[:len(c["y"])] = c["y"]
    return head.tobytes() + y.tobytes()


def _host_cases():
    rng = np.random.default_rng(6)
    cases = []

    def add(nsym, g, B=0, W=0, D=0, first=0, final=True, init=0, threads=256, y=None, amp=None):
        Bq, Wq, _ = M.geometry(B, W, D)
        k_lo = min(0, max(0, first // Bq * Bq - Wq) - first)
        amp = amp or max(2, 2 * sum(abs(v) for v in g))
        y = rng.integers(-amp, amp + 1, nsym - k_lo).clip(-32768, 32767) if y is None else np.asarray(y)
        assert len(y) == nsym - k_lo
        cases.append(dict(y=y.astype(np.int64), k_lo=k_lo, g=g, B=B, W=W, D=D, first=first, final=final, init=init, threads=threads))

    for mem in (1, 2, 3, 4):
        for geom in ((5, 2, 3), (64, 0, 0), (0, 0, 0), (256, 128, 128)):
            g = rng.integers(-40, 41, mem + 1).tolist()
            for nsym in (1, geom[0] or 192, (geom[0] or 192) + 1, 1000):
                add(nsym, g, *geom, init=int(rng.integers(0, 1 << mem)), threads=int(rng.choice([64, 128, 256])))
            add(700, g, *geom, first=int(rng.integers(1, 3000)), final=False, threads=64)
            add(3, g, *geom, first=7, final=False)                               # nothing is decided
    add(12, [3, 3], 12, 1, 1, y=np.zeros(12))                                    # every ACS ties
    add(12, [3, -3, 0], 12, 1, 1, init=1, y=np.zeros(12))
    add(300, [0, 0, 0, 0, 0], 5, 2, 3, init=9, y=np.zeros(300))
    add(600, [1 << 18, -(1 << 18), 1 << 18, -(1 << 18)], 448, 32, 32, y=rng.choice([-32768, 32767], 600))     # the metrics' bound
    add(600, [1 << 20, 0], 510, 1, 1, y=np.full(600, -32768))
    return cases


def test_lane_core_on_the_cpu_equals_the_model(host_exe, tmp_path):
    cases = _host_cases()
    (tmp_path / "c.bin").write_bytes(b"".join(_blob(c) for c in cases))
    r = subprocess.run([str(host_exe), str(tmp_path / "c.bin"), str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"cases {len(cases)}" in r.stdout, r.stderr[-3000:]
    lines = (tmp_path / "o.txt").read_text().split("\n")
    for i, c in enumerate(cases):
        bits, windows = M.decide(c["y"], c["k_lo"], c["g"], c["first"], c["final"], c["init"], c["B"], c["W"], c["D"])
        assert [int(t) for t in lines[2 * i].split()] == [len(bits), windows], (i, lines[2 * i])
        assert [int(t, 16) for t in lines[2 * i + 1].split()] == fir_model.pack(bits).tolist(), i
    assert M.decide(cases[-5]["y"], 0, [3, 3], B=12, W=1, D=1)[0].tolist() == [1, 0] * 6


# ---- the closed loop on the CPU ----------------------------------------------------------------------------------------

def test_closed_loop_on_the_oracle_waveform(oracle):
    """The oracle's waveform through an echo of the main path's size one bit late, plus Gaussian noise (mlse_model.LOOP says why):
    the linear receiver, the DFE and the sequence detector designed from the same pulse at the same cursor, 12 feed-forward
    taps each.  The sequence detector leaves strictly fewer errors than the DFE, which leaves at least 50."""
    r = M.loop_counts(oracle)
    print(r)
    assert r["ff"] == r["mlse_ff"] == M.LOOP_FF and r["fb"] == M.LOOP_FB and r["g"] == M.LOOP_G and r["shift"] == M.LOOP_SHIFT
    assert r["linear"][1] == r["dfe"][1] == r["mlse"][1] == M.LOOP_BITS
    assert (r["linear"][0], r["dfe"][0], r["mlse"][0]) == (M.LOOP_LINEAR_ERRORS, M.LOOP_DFE_ERRORS, M.LOOP_MLSE_ERRORS)
    assert r["dfe"][0] >= 50 and r["mlse"][0] < r["dfe"][0]
    # the channels that were tried first leave the DFE without an error: the reason for the added noise
    assert dfe_model.LOOP_DFE_ERRORS == 0


# ---- past one pass of the detector's grid ------------------------------------------------------------------------------------
# The kernel's workgroups take ceil(nblocks / wpg) groups of windows, at most 16 per compute unit at a time (tests/grid.py).
# These records make workgroup 0 take three turns of that loop and leave the last pass ragged.  tests/test_gpu_mlse.py runs
# them on the GPU; the expected bits are bbb_mlse_model_host's, held to the model here on three stretches of the same record
# (windows do not depend on one another).
MULTIPASS_TAPS, MULTIPASS_SHIFT = [2, 1, -1], 1
MULTIPASS = {"NS16": dict(g=[50, -30, 20, 12, -9], geom=(8, 8, 8), threads=256),
             "NS2": dict(g=[60, 45], geom=(8, 8, 8), threads=256),
             # B + W + D = 512.  At sixteen states no geometry leaves the 256-thread kernel (4624 + 4 * 4096 + 2 * (16 * 510 + 2)
             # bytes fit); four states are the most that reach the 64-thread one, with the fewest windows a workgroup
             "threads64": dict(g=[60, 45, -20], geom=(448, 32, 32), threads=64)}


def mlse_shape(ns, B, W, D):
    """(threads, windows per workgroup, LDS bytes) of mlse_kernels.hip's mlse_shape: the FIR image of (256 + 2048) / 2 + 4 words,
    B + W + D survivor words a wave, two bytes a symbol of the span; the workgroup halves until 40 KiB hold it."""
    for threads in (256, 128, 64):
        wpg = threads // ns
        nbytes = (4624 + threads // 64 * (B + W + D) * 8 + 2 * (wpg * B + W + D) + 15) & ~15
        if nbytes <= 40 * 1024:
            break
    return threads, wpg, nbytes


def multipass_record(name, ncus):
    """(samples int16, g, (B, W, D), nblocks, wpg) at one sample a symbol: +-1 data through the target plus uniform noise."""
    c = MULTIPASS[name]
    g, (B, W, D) = c["g"], c["geom"]
    threads, wpg, _ = mlse_shape(1 << (len(g) - 1), B, W, D)
    assert threads == c["threads"]
    nblocks = wpg * grid.passes(grid.MLSE, ncus=ncus) - 1
    n = B * nblocks - 3
    rng = np.random.default_rng(80 + len(g))
    d = rng.integers(0, 2, n + len(g), dtype=np.int16) * 2 - 1
    x = rng.integers(-40, 41, n, dtype=np.int16)
    for i, v in enumerate(g):
        x += np.int16(v) * d[len(g) - i:len(g) - i + n]
    return x, g, (B, W, D), nblocks, wpg


def multipass_expected(name, ncus):
    """(samples, g, geometry, nblocks, expected bits): the whole record from bbb_mlse_model_host, held to the model on the groups
    around the start of pass 2, on groups inside pass 3 and on the ragged end."""
    x, g, (B, W, D), nblocks, wpg = multipass_record(name, ncus)
    taps, shift = MULTIPASS_TAPS, MULTIPASS_SHIFT
    want, _ = _model_host(x, 0, _cfg(taps, g, 1, 0, shift, 1, B, W, D))
    per = grid.MLSE * ncus                                               # groups in a pass
    for glo, ghi in ((per - 1, per + 1), (2 * per + 1, 2 * per + 3), (-(-nblocks // wpg) - 2, None)):
        first = glo * wpg * B
        nb = M.nbefore_wanted(first, 1, len(taps), 0, B, W, D)
        if ghi is None:
            got, _ = M.run(x[first:], taps, g, 1, 0, shift, x[first - nb:first], first, True, 1, B, W, D)
            assert first + len(got) == len(want)
        else:
            got, _ = M.run(x[first:ghi * wpg * B + D], taps, g, 1, 0, shift, x[first - nb:first], first, False, 1, B, W, D)
            assert len(got) == (ghi - glo) * wpg * B
        assert np.array_equal(got, want[first:first + len(got)]), (name, glo)
    return x, g, (B, W, D), nblocks, want


def test_mlse_shape_restated():
    """The shapes the multi-pass cases rely on: 16 and 128 windows a workgroup of 256 threads at B = W = D = 8, and the long
    geometry at four states, which exceeds the 40 KiB target at 256 and at 128 threads and runs the 64-thread kernel."""
    assert mlse_shape(16, 8, 8, 8)[:2] == (256, 16) and mlse_shape(2, 8, 8, 8)[:2] == (256, 128)
    B, W, D = MULTIPASS["threads64"]["geom"]
    assert B + W + D == 512
    at128 = (4624 + 2 * 512 * 8 + 2 * (128 // 4 * B + W + D) + 15) & ~15
    assert at128 == 41616 > 40 * 1024 and mlse_shape(4, B, W, D) == (64, 16, 4624 + 4096 + 2 * (16 * 448 + 64))
    assert mlse_shape(16, 510, 1, 1)[0] == mlse_shape(16, 448, 32, 32)[0] == 256   # sixteen states never leave 256 threads


@pytest.mark.parametrize("name", sorted(MULTIPASS))
def test_multipass_host_model_equals_the_model_on_stretches(name):
    x, g, (B, W, D), nblocks, want = multipass_expected(name, 256)
    assert len(want) == B * nblocks - 3 and 0 < want.mean() < 1
