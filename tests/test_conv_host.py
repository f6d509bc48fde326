"""The convolutional codec without a GPU: the model against exhaustive search, the pins of its convention (impulse response, free
distances, the punctured presets), its tie rules and termination, bbb_conv_model_host, bbb_conv_encode_host and bbb_conv_plan
against the model, the argument checks of bbb_conv_decode and bbb_conv_encode through the C ABI, the stream's cutting in the
model, the kernel's per-lane core (basebandboard_amd/csrc/conv_common.hpp) called from a restatement of the kernel's walk on
the CPU under ASan/UBSan, and the closed loop encode -> noise -> decode -> count."""
import ctypes as C
import itertools
import re
import subprocess

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from conftest import ROOT

import fir_model
import grid
import conv_model as M

G171 = (0o171, 0o133)
GEOMS = ((5, 2, 3), (64, 0, 0), (0, 0, 0), (256, 128, 128))


def _cfg(code, B=0, W=0, D=0):
    c = _lib.ConvCfg()
    c.K, c.n, c.init_state, c.period, c.terminated = code.K, code.n, code.init_state, code.period, int(code.terminated)
    for i in range(code.n):
        c.gen[i], c.keep[i] = code.gens[i], code.keep[i]
    c.block_steps, c.warmup_steps, c.lookahead_steps = B, W, D
    return c


def _random_code(rng, K=None, n=None, period=None, **kw):
    K = K or int(rng.integers(3, 8))
    n = n or int(rng.integers(2, 4))
    period = period or int(rng.choice([1, 2, 3, 7, 16]))
    while True:
        keep = rng.integers(0, 1 << period, n).tolist()
        if all(any(k >> r & 1 for k in keep) for r in range(period)):
            break
    return M.Code(K, rng.integers(1, 1 << K, n).tolist(), period, keep, int(rng.integers(0, 1 << (K - 1))), **kw)


def _noisy(rng, code, nsteps, first=0, sigma=40):
    """(data bits, received int16 values) of nsteps random bits from step `first` on, encoded from a random state."""
    bits = rng.integers(0, 2, nsteps)
    tx, _ = M.encode(code, bits, first, int(rng.integers(0, code.ns)))
    return bits, ((2 * tx.astype(np.int64) - 1) * 64 + np.rint(rng.normal(0, sigma, len(tx)))).astype(np.int16)


# ---- the model ---------------------------------------------------------------------------------------------------------

def test_model_finds_the_maximum_over_all_sequences():
    """One window over everything: the path's total gain is the maximum over all 2^9 sequences from init_state.  Gains are
    compared, not bits: ties exist."""
    rng = np.random.default_rng(1)
    for case in range(45):
        code = _random_code(rng, K=3 + case % 3, period=1)
        r = rng.integers(-8, 9, (9, code.n))
        bits, total = M.viterbi(code, r)
        assert total == M.path_gain(code, r, bits), (case, "the traced-back path does not earn the metric")
        assert total == max(M.path_gain(code, r, seq) for seq in itertools.product((0, 1), repeat=9)), case
        d, w = M.decide(code, r, 0, 0, 9, B=9, W=1, D=1)
        assert d.tolist() == bits and w == 1


def test_pins_of_the_convention():
    tx, state = M.encode(M.Code(7, G171), [1, 0, 0, 0, 0, 0, 0])
    assert "".join(map(str, tx[0::2])) == "1111001" and "".join(map(str, tx[1::2])) == "1011011" and state == 0b1000000 & 63
    assert M.free_distance(M.Code(3, (7, 5))) == 5
    assert M.free_distance(M.Code(7, G171)) == 10
    assert M.free_distance(M.Code(7, (0o133, 0o171, 0o165))) == 15
    assert [M.free_distance(M.Code(7, G171, *M.PRESETS[k])) for k in ("2/3", "3/4", "5/6", "7/8")] == [6, 5, 4, 3]
    assert M.PRESETS == bbb.fec.PRESETS
    # within a step the kept bits go out in order of i; idx counts them
    code = M.Code(7, G171, *M.PRESETS["3/4"])
    assert [M.idx(code, t) for t in range(8)] == [0, 2, 3, 4, 6, 7, 8, 10] and code.rate == 0.75
    full, _ = M.encode(M.Code(7, G171), [1, 1, 0, 1, 0, 0])
    assert M.encode(code, [1, 1, 0, 1, 0, 0])[0].tolist() == full[[0, 1, 3, 4, 6, 7, 9, 10]].tolist()


def test_tie_rules_on_all_zero_input_and_terminated():
    rng = np.random.default_rng(2)
    for K in range(3, 8):
        code = M.Code(K, rng.integers(1, 1 << K, 2).tolist(), init_state=(1 << (K - 1)) - 1)
        # every ACS ties: c = 0 survives everywhere and the lowest end state wins, so all zeros in every window that does not
        # start at step 0; the first window leaves init_state along its only allowed paths and reaches state 0
        got = M.decide(code, np.zeros((40, 2), dtype=np.int64), 0, 0, 40, B=5, W=2, D=3)[0]
        assert not got[K - 1:].any(), K
        assert not M.decide(M.Code(K, code.gens), np.zeros((40, 2), dtype=np.int64), 0, 0, 40, B=5, W=2, D=3)[0].any()
    # terminated: a final call's last window ends in state 0, so its last K - 1 decisions are 0 whatever was received; a call
    # that is not final, and every other window, is as without
    code, term = M.Code(7, G171), M.Code(7, G171, terminated=True)
    vals = rng.integers(-100, 101, 2 * 500).astype(np.int16)
    plain, ended = M.run(code, vals)[0], M.run(term, vals)[0]
    assert plain[-6:].any() and not ended[-6:].any() and np.array_equal(plain[:192], ended[:192])
    assert np.array_equal(M.run(term, vals, final=False)[0], M.run(code, vals, final=False)[0])
    # and it helps where it should: a terminated record whose tail is hit hard
    bits = np.concatenate([rng.integers(0, 2, 94), np.zeros(6, dtype=np.int64)])
    rx = (2 * M.encode(code, bits)[0].astype(np.int64) - 1) * 64
    rx[-10:] = 0
    assert np.array_equal(M.run(term, rx)[0], bits)


def test_non_final_rule_and_plan_arithmetic():
    code = M.Code(7, G171)
    assert M.plan(code, 2000) == (1000, 1000, 0) and M.plan(code, 2000, 0, False) == (1000, 768, 0)
    assert M.plan(code, 2001) == (1000, 1000, 0)                                        # a step cut short is ignored
    assert M.plan(code, 2 * 255, 0, False)[1] == 0 and M.plan(code, 2 * 256, 0, False)[1] == 192
    assert M.plan(code, 600, 192, False) == (300, 192, 128) and M.plan(code, 20, 192, False)[1] == 0
    assert M.plan(code, 0, 200, False)[2] == 2 * (200 - 128) and M.plan(code, 0, 10)[2] == 20
    p34 = M.Code(7, G171, *M.PRESETS["3/4"])
    assert M.plan(p34, 4) == (3, 3, 0) and M.plan(p34, 5) == (3, 3, 0) and M.plan(p34, 6) == (4, 4, 0) and M.plan(p34, 3, 1) == (2, 2, 2)
    assert M.plan(p34, 0, 192, False)[2] == M.idx(p34, 192) - M.idx(p34, 128) == 85 and M.plan(p34, 0, 193, False)[2] == 87
    assert M.ndecided(7, 0, False, 5, 2, 3) == 0 and M.ndecided(8, 0, False, 5, 2, 3) == 5 and M.ndecided(100, 95, False, 5, 2, 3) == 95


def test_stream_equals_one_call_in_the_model():
    rng = np.random.default_rng(3)
    for geom, punct in (((0, 0, 0), "3/4"), ((5, 2, 3), None), ((64, 128, 1), "7/8")):
        code = M.Code(7, G171, *(M.PRESETS[punct] if punct else (1, None)))
        _, rx = _noisy(rng, code, 900)
        want, _ = M.run(code, rx, B=geom[0], W=geom[1], D=geom[2])
        got = M.stream(code, rx, [0, 1, 5, 64, 64, 333, len(rx) - 1], *geom)
        assert np.array_equal(got, want), geom
        hard = (rx >= 0).astype(np.int64)
        assert np.array_equal(M.stream(code, hard, [7, 500], *geom, hard=True), M.run(code, hard, B=geom[0], W=geom[1], D=geom[2], hard=True)[0])


# ---- the host entry points ---------------------------------------------------------------------------------------------

def _pack_at(bits, off):
    """bits 0 / 1 packed LSB first into u64 words from bit `off` on."""
    b = np.zeros((off + len(bits) + 63) // 64 * 64, dtype=np.uint8)
    b[off:off + len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint64)


def _model_host(code, vals, nb, first=0, final=True, B=0, W=0, D=0, hard=False, in_off=0):
    lib = _lib.lib()
    vals = np.asarray(vals)
    nin = len(vals) - nb
    _, nd, _ = M.plan(code, nin, first, final, B, W, D)
    if hard:
        buf = _pack_at(vals, in_off)
    else:
        buf = np.concatenate([np.full(in_off, 0x7ABC, dtype=np.int16), vals.astype(np.int16)])
    bits = np.full((nd + 63) // 64 + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    got = C.c_uint64()
    rc = lib.bbb_conv_model_host(C.c_void_p(buf.ctypes.data), in_off + nb, nin, nb, first, int(final), int(hard), C.byref(_cfg(code, B, W, D)),
                                 C.c_void_p(bits.ctypes.data), C.byref(got))
    assert rc == 0 and got.value == nd, lib.bbb_last_error_detail()
    assert bits[-1] == 0xA5A5A5A5A5A5A5A5, "a word beyond ceil(ndecided / 64) was written"
    return np.unpackbits(bits[:-1].view(np.uint8), bitorder="little")[:nd], bits[:-1]


def test_model_host_equals_the_model():
    rng = np.random.default_rng(4)
    for K in range(3, 8):
        for n in (2, 3):
            for B, W, D in GEOMS:
                for first, nb in ((0, 0), (7, 40), (200, 3), (192, 600), ((1 << 40) + 3, 1000)):
                    code = _random_code(rng, K, n, terminated=bool(rng.integers(0, 2)))
                    _, rx = _noisy(rng, code, 700, first)
                    nb = min(nb, M.idx(code, first))
                    hist = rng.integers(-90, 91, nb).astype(np.int16)
                    vals, final, hard = np.concatenate([hist, rx]), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
                    if hard:
                        vals = (vals >= 0).astype(np.int64)
                    want, _ = M.run(code, vals, nb, first, final, B, W, D, hard)
                    got, words = _model_host(code, vals, nb, first, final, B, W, D, hard, in_off=int(rng.integers(0, 70)))
                    assert np.array_equal(got, want), (K, n, B, first, nb, final, hard)
                    assert np.array_equal(words, fir_model.pack(want))           # the unused bits of the last word are 0
    # the values at both ends of int16, three of them a step, over the longest window
    code = M.Code(7, (0o133, 0o171, 0o165), init_state=5)
    vals = rng.choice([-32768, 32767], 3 * 1200)
    assert np.array_equal(_model_host(code, vals, 0, B=256, W=128, D=128)[0], M.run(code, vals, B=256, W=128, D=128)[0])
    # the tie rule through the C model
    assert not _model_host(M.Code(5, (0o23, 0o35)), np.zeros(80, dtype=np.int16), 0, B=5, W=2, D=3)[0].any()


def _encode_host(code, bits, first=0, state=None):
    lib = _lib.lib()
    nout = M.idx(code, first + len(bits)) - M.idx(code, first)
    out = np.full((nout + 63) // 64 + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    src = _pack_at(bits, 0) if len(bits) else np.zeros(1, dtype=np.uint64)
    got, st = C.c_uint64(), C.c_uint32(state if state is not None else 0)
    rc = lib.bbb_conv_encode_host(C.c_void_p(src.ctypes.data), len(bits), first, C.byref(_cfg(code)), C.byref(st) if state is not None else None,
                                  C.c_void_p(out.ctypes.data), C.byref(got))
    assert rc == 0 and got.value == nout, lib.bbb_last_error_detail()
    assert out[-1] == 0xA5A5A5A5A5A5A5A5
    return np.unpackbits(out[:-1].view(np.uint8), bitorder="little"), nout, st.value


def test_encode_host_equals_the_model():
    rng = np.random.default_rng(5)
    for K in range(3, 8):
        for n in (2, 3):
            for period in (1, 2, 3, 7, 16):
                code = _random_code(rng, K, n, period)
                for nsteps in (1, 63, 64, 65, 700):
                    first = int(rng.choice([0, 1, 5, period + 1, (1 << 40) + 3]))
                    bits = rng.integers(0, 2, nsteps)
                    want, _ = M.encode(code, bits, first)
                    got, nout, _ = _encode_host(code, bits, first)
                    assert nout == len(want) and np.array_equal(got[:nout], want) and not got[nout:].any(), (K, n, period, nsteps, first)
                # a record in pieces with the state word
                bits = rng.integers(0, 2, 300)
                want, end = M.encode(code, bits)
                state, out = code.init_state, []
                for lo, hi in ((0, 1), (1, 3), (3, 3), (3, 130), (130, 300)):
                    got, nout, state = _encode_host(code, bits[lo:hi], lo, state)
                    out.append(got[:nout])
                assert np.array_equal(np.concatenate(out), want) and state == end


def test_plan_equals_the_model():
    lib = _lib.lib()
    rng = np.random.default_rng(6)
    for _ in range(300):
        B, W, D = ((0, 0, 0), (5, 2, 3), (64, 128, 128), (256, 128, 128), (1, 1, 1))[int(rng.integers(0, 5))]
        code = _random_code(rng)
        nin, first, final = int(rng.integers(0, 5000)), int(rng.choice([0, 1, 5, 191, 192, 193, 1000, 1 << 40])), bool(rng.integers(0, 2))
        v = [C.c_uint64() for _ in range(3)]
        assert lib.bbb_conv_plan(C.byref(_cfg(code, B, W, D)), nin, first, int(final), *[C.byref(t) for t in v]) == 0
        assert tuple(t.value for t in v) == M.plan(code, nin, first, final, B, W, D), (B, code.period, code.keep, nin, first, final)
    assert lib.bbb_conv_plan(C.byref(_cfg(M.Code(7, G171))), 100, 0, 1, None, None, None) == 0
    c = bbb.ConvCode(7, G171, "3/4")
    assert c.plan(4000) == (3000, 3000, 0) and c.plan(4000, final=False) == (3000, 2880, 0) and c.plan(0, 192, False)[2] == 85
    assert c.rate == bbb.fec.Fraction(3, 4) and bbb.ConvCode(7, G171).rate == bbb.fec.Fraction(1, 2) and c.idx(7) == 10


def test_invalid_arguments_return_before_the_device_is_touched():
    """Every pointer here is a number no device ever gave out: a call that got as far as the device would fail otherwise
    (BBB_ENODEV on a machine without a GPU), and the last cases show that a valid call does get that far."""
    import torch
    lib = _lib.lib()
    IN, BITS, STATS, OUT = 1 << 20, 1 << 24, 1 << 28, 1 << 26

    def dec(cfg, in_dev=IN, in_first=0, nin=4096, nb=0, first=0, final=1, fmt=0, bits=BITS, stats=None):
        return lib.bbb_conv_decode(C.c_void_p(in_dev), in_first, nin, nb, first, final, fmt, C.byref(cfg) if cfg is not None else None,
                                   C.c_void_p(bits), C.c_void_p(stats) if stats else None, None, 0, None)

    def enc(cfg, bits=IN, nsteps=4096, first=0, state=None, out=OUT):
        return lib.bbb_conv_encode(C.c_void_p(bits), nsteps, first, C.byref(cfg) if cfg is not None else None,
                                   C.c_void_p(state) if state else None, C.c_void_p(out), None, 0, None)

    def changed(**kw):
        c = _cfg(M.Code(7, G171), *[kw.pop(k, 0) for k in ("B", "W", "D")])
        for k, v in kw.items():
            if isinstance(v, (list, tuple)):
                for i, x in enumerate(v):
                    getattr(c, k)[i] = x
            else:
                setattr(c, k, v)
        return c

    good = _cfg(M.Code(7, G171))
    bad_cfg = [(None, "null"), (changed(K=2), "K must"), (changed(K=8), "K must"), (changed(n=1), "n must"), (changed(n=4), "n must"),
               (changed(gen=[0, 0o133]), "gen\\[0\\]"), (changed(gen=[0o171, 128]), "gen\\[1\\]"), (changed(period=0), "period"),
               (changed(period=17), "period"), (changed(period=2, keep=[1, 0]), "keep"),          # step 1 keeps nothing
               (changed(period=2, keep=[3, 4]), "keep"),                                           # a bit beyond the period
               (changed(keep=[0, 0]), "keep"), (changed(W=129), "warmup"), (changed(D=129), "lookahead"),
               (changed(B=385), "512"), (changed(B=513, W=1, D=1), "512")]                         # 385 + 64 + 64
    for cfg, what in bad_cfg:
        for call in (dec, enc):
            assert call(cfg) == _lib.BBB_EINVAL, what
            assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    bad = [(dec, dict(in_dev=0), "in_dev"), (dec, dict(bits=0), "bits_packed_dev"), (dec, dict(fmt=2), "format"),
           (dec, dict(bits=BITS + 4), "misaligned"), (dec, dict(in_dev=IN + 1), "misaligned"), (dec, dict(stats=STATS + 4), "misaligned"),
           (dec, dict(in_dev=IN + 2, fmt=1), "misaligned"),                                        # packed bits sit in u64 words
           (dec, dict(bits=IN + 4096 * 2 - 8), "bits_packed_dev overlaps"),                        # the last values
           (dec, dict(bits=IN + 512 - 8, fmt=1), "bits_packed_dev overlaps"),                      # the last word of 4096 bits
           (dec, dict(bits=IN + 2000 - 256, in_first=1000, nb=128, first=192), "bits_packed_dev overlaps"),   # the history the window reaches
           (dec, dict(stats=IN), "stats_dev overlaps"), (dec, dict(stats=BITS), "stats_dev overlaps"),
           (dec, dict(in_first=10, nb=11), "nbefore"), (dec, dict(nin=(1 << 60) + 1), "2\\^60"),
           (dec, dict(first=(1 << 58) - 2047), "2\\^58"), (dec, dict(first=1 << 63), "2\\^58"),
           (enc, dict(bits=0), "bits_dev"), (enc, dict(out=0), "out_dev"), (enc, dict(bits=IN + 4), "misaligned"),
           (enc, dict(out=OUT + 4), "misaligned"), (enc, dict(state=STATS + 2), "misaligned"),
           (enc, dict(out=IN + 504), "out_dev overlaps"), (enc, dict(state=IN + 508), "state_dev overlaps"),
           (enc, dict(state=OUT + 1020), "state_dev overlaps"), (enc, dict(first=(1 << 58) - 4095), "2\\^58"), (enc, dict(first=1 << 63), "2\\^58")]
    for call, kw, what in bad:
        assert call(good, **kw) == _lib.BBB_EINVAL, what
        assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    if not torch.cuda.is_available():
        # exactly at the bounds, and outputs next to the inputs but not in them: valid
        assert dec(changed(B=256, W=128, D=128)) == _lib.BBB_ENODEV and dec(changed(B=384)) == _lib.BBB_ENODEV
        assert dec(good, bits=IN + 4096 * 2) == _lib.BBB_ENODEV and dec(good, bits=IN + 512, fmt=1) == _lib.BBB_ENODEV
        assert dec(good, bits=IN + 2000 - 256, in_first=1000, nb=128, first=0) == _lib.BBB_ENODEV      # at step 0 no history is read
        assert dec(good, in_first=10, nb=10) == _lib.BBB_ENODEV and dec(good, first=(1 << 58) - 2048) == _lib.BBB_ENODEV
        assert enc(good) == _lib.BBB_ENODEV and enc(good, out=IN + 512, state=IN + 512 + 1024) == _lib.BBB_ENODEV
        assert enc(good, first=(1 << 58) - 4096) == _lib.BBB_ENODEV


def test_python_argument_checks():
    with pytest.raises(ValueError, match="K must"):
        bbb.ConvCode(8, G171)
    with pytest.raises(ValueError, match="2..3"):
        bbb.ConvCode(7, (0o171,))
    with pytest.raises(ValueError, match="gen"):
        bbb.ConvCode(5, G171)
    with pytest.raises(ValueError, match="puncture"):
        bbb.ConvCode(7, G171, "4/5")
    with pytest.raises(ValueError, match="rate 1/2"):
        bbb.ConvCode(7, (0o133, 0o171, 0o165), "3/4")
    with pytest.raises(ValueError, match="keep"):
        bbb.ConvCode(7, G171, (2, (1, 0)))
    with pytest.raises(ValueError, match="512"):
        bbb.ConvCode(7, G171, geometry=(500, 0, 0))
    d = bbb.ConvCode(5, (0o23, 0o35), (3, (0b110, 0b011)), terminated=True, init_state=9, geometry=(5, 2, 3))
    c = d._cfg()
    assert (c.K, c.n, list(c.gen), c.init_state, c.period, list(c.keep), c.terminated) == (5, 2, [0o23, 0o35, 0], 9, 3, [6, 3, 0], 1)
    assert (c.block_steps, c.warmup_steps, c.lookahead_steps) == (5, 2, 3) and d.stats() == dict(windows=0, steps=0) and d.rate == bbb.fec.Fraction(3, 4)


# ---- the kernel's core on the CPU, under the sanitizers ------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("conv_host")
    exe = d / "conv_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", str(ROOT / "tests" / "conv_host.cpp"), "-o", str(exe)])
    return exe


def _blob(c):
    code = c["code"]
    gens, keep = code.gens + [0] * (3 - code.n), code.keep + [0] * (3 - code.n)
    head = np.array([c["mode"], len(c["vals"]), c["nb"], code.K, code.n] + gens + [code.init_state, code.period] + keep +
                    [int(code.terminated), c["B"], c["W"], c["D"], c["first"], int(c["final"]), c["threads"], c["wpg"], int(c["hard"]), c["in_off"], 0],
                    dtype=np.int64)
    assert len(head) == 24
    v = np.zeros((len(c["vals"]) + 3) // 4 * 4, dtype=np.int16)
    v[:len(c["vals"])] = c["vals"]
    return head.tobytes() + v.tobytes()


def _host_cases():
    rng = np.random.default_rng(7)
    cases = []

    def add(code, vals, nb=0, B=0, W=0, D=0, first=0, final=True, threads=256, wpg=None, hard=False, in_off=0):
        cases.append(dict(mode=0, code=code, vals=np.asarray(vals), nb=nb, B=B, W=W, D=D, first=first, final=final, threads=threads,
                          wpg=wpg or threads // code.ns, hard=hard, in_off=in_off))

    for K in range(3, 8):
        for n in (2, 3):
            for geom in GEOMS:
                code = _random_code(rng, K, n, terminated=bool(rng.integers(0, 2)))
                threads = int(rng.choice([64, 128, 256]))
                for nsteps in (1, geom[0] or 192, (geom[0] or 192) + 1, 600):
                    hard = bool(rng.integers(0, 2))
                    rx = _noisy(rng, code, nsteps)[1]
                    add(code, (rx >= 0).astype(np.int16) if hard else rx, 0, *geom, threads=threads, hard=hard, in_off=int(rng.integers(0, 70)))
                first = int(rng.integers(1, 3000))
                nb = int(rng.integers(0, M.nbefore_wanted(code, first, *geom) + 20))
                nb = min(nb, M.idx(code, first))
                add(code, np.concatenate([rng.integers(-90, 91, nb).astype(np.int16), _noisy(rng, code, 500, first)[1]]), nb, *geom, first=first,
                    final=False, threads=64, wpg=max(1, 64 // code.ns // 2), in_off=3)
                add(code, _noisy(rng, code, 3, 7)[1], 0, *geom, first=7, final=False)        # nothing is decided
    for K in range(3, 8):
        add(M.Code(K, rng.integers(1, 1 << K, 2).tolist(), init_state=1), np.zeros(300, dtype=np.int16), B=5, W=2, D=3)      # every ACS ties
    add(M.Code(7, (0o133, 0o171, 0o165), init_state=5), rng.choice([-32768, 32767], 3 * 1200), B=256, W=128, D=128)          # the metrics' bound
    add(M.Code(3, (7, 5, 7)), np.full(3 * 1200, -32768), B=510, W=1, D=1, threads=64, wpg=1)
    return cases


def test_lane_core_on_the_cpu_equals_the_model(host_exe, tmp_path):
    cases = _host_cases()
    rng = np.random.default_rng(8)
    enc = []
    for K in range(3, 8):
        for period in (1, 3, 16):
            code = _random_code(rng, K, None, period)
            for nsteps, first in ((1, 0), (64, 5), (700, period + 1), (130, (1 << 40) + 3)):
                enc.append(dict(mode=1, code=code, vals=rng.integers(0, 2, nsteps), nb=int(rng.integers(0, code.ns)), B=0, W=0, D=0, first=first,
                                final=0, threads=0, wpg=0, hard=0, in_off=0))
    (tmp_path / "c.bin").write_bytes(b"".join(_blob(c) for c in cases + enc))
    r = subprocess.run([str(host_exe), str(tmp_path / "c.bin"), str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"cases {len(cases) + len(enc)}" in r.stdout, r.stderr[-3000:]
    lines = (tmp_path / "o.txt").read_text().split("\n")
    for i, c in enumerate(cases):
        bits, windows = M.run(c["code"], c["vals"], c["nb"], c["first"], c["final"], c["B"], c["W"], c["D"], c["hard"])
        assert [int(t) for t in lines[2 * i].split()] == [len(bits), windows], (i, lines[2 * i])
        assert [int(t, 16) for t in lines[2 * i + 1].split()] == fir_model.pack(bits).tolist(), i
    for i, c in enumerate(enc, len(cases)):
        want, state = M.encode(c["code"], c["vals"], c["first"], c["nb"])
        assert [int(t) for t in lines[2 * i].split()] == [len(want), state], (i, lines[2 * i])
        assert [int(t, 16) for t in lines[2 * i + 1].split()] == fir_model.pack(want).tolist(), i


# ---- the closed loop on the CPU ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("1/2", "3/4"))
def test_closed_loop_counts(name):
    """8192 random bits through (0171, 0133), at rate 1/2 and punctured to 3/4, plus Gaussian noise (conv_model.LOOP): soft
    decoding leaves fewer errors than hard decoding, which leaves fewer than the channel made."""
    r = M.loop_counts(name)
    print(name, r)
    assert r == M.LOOP_COUNTS[name]
    assert r["soft"] < r["hard"] < r["channel"]


# ---- past one pass of the decoder's grid ---------------------------------------------------------------------------------------
# The decode kernel's workgroups take ceil(nblocks / wpg) groups of windows, at most 16 per compute unit at a time
# (tests/grid.py).  These records make workgroup 0 take three turns of that loop and leave the last pass ragged, at the
# smallest geometry there is.  tests/test_gpu_conv.py runs them on the GPU; the expected bits are bbb_conv_model_host's,
# which is held to the model here on three stretches of the same record (windows do not depend on one another).
# Out of reach at this cost: the encoder's grid is capped at 2^20 workgroups of 256 words, 2^34 transmitted bits a pass.
MULTIPASS_GEOM = (8, 8, 8)
MULTIPASS = {"K7_soft": dict(K=7, gens=G171, period=1, keep=None, wpg=4, hard=False),
             "K3_hard_punctured": dict(K=3, gens=(7, 5, 7), period=3, keep=(0b101, 0b011, 0b110), wpg=64, hard=True)}


def multipass_record(name, ncus):
    """(code, values, hard, nblocks, wpg) of a multi-pass case on a device of ncus compute units: random data through
    bbb_conv_encode_host; soft values carry noise of sigma 40 on +-64, hard bits are wrong one time in 16."""
    c = MULTIPASS[name]
    B = MULTIPASS_GEOM[0]
    code = M.Code(c["K"], c["gens"], c["period"], c["keep"], init_state=1)
    nblocks = c["wpg"] * grid.passes(grid.CONV_DECODE, ncus=ncus) - 1
    nsteps = B * nblocks - 3
    rng = np.random.default_rng(70 + c["K"])
    tx, nout, _ = _encode_host(code, rng.integers(0, 2, nsteps))
    tx = tx[:nout]
    if c["hard"]:
        vals = (tx ^ (rng.integers(0, 16, nout) == 0)).astype(np.int64)
    else:
        vals = ((2 * tx.astype(np.int64) - 1) * 64 + np.rint(rng.normal(0, 40, nout))).astype(np.int16)
    assert -(-nblocks // c["wpg"]) == grid.passes(grid.CONV_DECODE, ncus=ncus) and nblocks % c["wpg"] and nsteps % B
    return code, vals, c["hard"], nblocks, c["wpg"]


def multipass_expected(name, ncus):
    """(code, values, hard, nblocks, expected bits): the whole record from bbb_conv_model_host, held to the model on the groups
    around the start of pass 2, on groups inside pass 3 and on the ragged end."""
    code, vals, hard, nblocks, wpg = multipass_record(name, ncus)
    B, W, D = MULTIPASS_GEOM
    want, _ = _model_host(code, vals, 0, B=B, W=W, D=D, hard=hard)
    g = grid.CONV_DECODE * ncus                                          # groups in a pass
    for glo, ghi in ((g - 2, g + 2), (2 * g + 1, 2 * g + 4), (-(-nblocks // wpg) - 3, None)):
        first = glo * wpg * B
        nb = M.nbefore_wanted(code, first, B, W, D)
        lo = M.idx(code, first) - nb
        if ghi is None:
            got, _ = M.run(code, vals[lo:], nb, first, True, B, W, D, hard)
            assert first + len(got) == len(want)
        else:
            got, _ = M.run(code, vals[lo:M.idx(code, ghi * wpg * B + D)], nb, first, False, B, W, D, hard)
            assert len(got) == (ghi - glo) * wpg * B
        assert np.array_equal(got, want[first:first + len(got)]), (name, glo)
    return code, vals, hard, nblocks, want


@pytest.mark.parametrize("name", sorted(MULTIPASS))
def test_multipass_host_model_equals_the_model_on_stretches(name):
    code, vals, hard, nblocks, want = multipass_expected(name, 256)
    assert len(want) == 8 * nblocks - 3 and 0 < want.mean() < 1
