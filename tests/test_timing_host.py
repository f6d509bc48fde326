"""The symbol timing recovery without a GPU: the model against the definition term by term, bbb_timing_model_host against the
model, bbb_timing_plan and the argument checks of bbb_timing_run through the C ABI, the model's streaming property, the three
passes of the device restated on the CPU over basebandboard_amd/csrc/timing_common.hpp under ASan/UBSan, and the closed loop:
the CPU oracle's waveform resampled with a clock offset, where no fixed phase works and the tracker leaves a handful of errors."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from conftest import ROOT

import fir_model
import grid
import timing_model as M


def _cfg(P, taps=(1,), L=0, h=0, threshold=0, strict=False, init=M.ACQUIRE, chunk=0, shift=0, out_bytes=2, decim=1, phase=0):
    c = _lib.TimingCfg()
    c.ff.ntaps = len(taps)
    for i, v in enumerate(taps):
        c.ff.taps[i] = v
    c.ff.shift, c.ff.decim, c.ff.phase, c.ff.out_bytes = shift, decim, phase, out_bytes
    c.spb, c.block_symbols, c.hysteresis_shift, c.threshold, c.strict, c.init_phase, c.chunk_blocks = P, L, h, threshold, int(strict), init, chunk
    return c


# ---- the model -------------------------------------------------------------------------------------------------------------

def _definition(x, before, P, taps, L, h, thr, strict, init, final):
    """The header's definition with every sum written out over Python ints."""
    nb = len(before)
    xe = lambda j: int(x[j]) if j >= 0 else (int(before[nb + j]) if -j <= nb else 0)                        # noqa: E731
    a = lambda n: sum(c * xe(n - i) for i, c in enumerate(taps))                                            # noqa: E731
    nin = len(x)
    nblocks = -(-nin // (L * P)) if final else nin // (L * P)
    nin = min(nin, nblocks * L * P)
    locked, phi, out, phases, stats = False, 0, [], [], [0, 0, 0, 0]
    for j in range(nblocks):
        E = [sum(abs(a(j * L * P + i * P + p) - thr) for i in range(L) if j * L * P + i * P + p < nin) for p in range(P)]
        m = w = 0
        if not locked:
            phi = init if init < P else [p for p in range(P) if E[p] == max(E)][0]
            locked = True
        else:
            cur, up, dn = E[phi], E[(phi + 1) % P], E[(phi - 1) % P]
            if up > cur + (cur >> h) and up >= dn:
                m = 1
            elif dn > cur + (cur >> h):
                m = -1
            phi = (phi + m) % P
            w = 1 if (m == 1 and phi == 0) else (-1 if (m == -1 and phi == P - 1) else 0)
        phases.append(phi)
        stats = [stats[0] + 1, stats[1] + abs(m), stats[2] + (w > 0), stats[3] + (w < 0)]
        out += [a(t) for t in (j * L * P + phi + i * P for i in range(w, L)) if t < nin]
    return out, phases, stats


def test_model_equals_the_definition_term_by_term():
    rng = np.random.default_rng(1)
    seen = [0, 0]
    for P, taps, L, h, thr, strict, init, nb, n, final in ((3, [1], 8, 1, 0, False, M.ACQUIRE, 0, 24 * 40 + 5, True), (4, [2, -1, 3], 8, 2, 3, True, 0, 3, 32 * 40, True),
                                                             (5, [1, 1], 9, 4, -2, False, 4, 1, 45 * 30 + 44, False), (3, [4, 0, -1, 2], 10, 1, 1, True, 2, 9, 30 * 40 + 1, True),
                                                             (4, [1], 8, 1, 0, False, 3, 0, 1, True)):
        x = rng.integers(-12, 13, n + nb)
        before, rec = x[:nb], x[nb:]
        want, phases, stats = _definition(rec, before, P, taps, L, h, thr, strict, init, final)
        r = M.run(rec, P, taps, L, h, thr, strict, init, before, final=final, out_bytes=4)
        assert r["soft"].tolist() == want and r["phases"].tolist() == phases and r["stats"] == stats, (P, taps)
        assert r["bits"].tolist() == [int(v > thr if strict else v >= thr) for v in want]
        assert r["state"] == ((M.LOCKED | phases[-1]), len(want)) and r["nbits"] == len(want)
        gaps = np.diff(r["instants"])
        assert set(gaps.tolist()) <= {P - 1, P, P + 1}                       # no bit twice, none skipped
        seen = [seen[0] + stats[2], seen[1] + stats[3]]
    assert seen[0] > 0 and seen[1] > 0                                       # the cases do wrap, both ways
    assert M.plan(1000, 8, 64) == (2, 1000, 130) and M.plan(1000, 8, 64, final=False) == (1, 512, 65) and M.plan(0, 8, 64) == (0, 0, 0)
    assert M.soft([70000, -70000, 37, -37], 0, 2).tolist() == [32767, -32768, 37, -37] and M.soft([70000], 2, 4).tolist() == [70000]


def test_ramp_records_move_in_every_block():
    for P, direction, start in ((4, 1, 0), (4, -1, 0), (256, 1, 255), (255, -1, 0)):
        L, nblocks = 8, 2 * P + 3 if P < 16 else 5
        r = M.run(M.ramp(P, L, nblocks, direction, start), P, L=L, init_phase=start)
        assert r["moves"].tolist() == [0] + [direction] * (nblocks - 1)
        assert r["phases"].tolist() == [(start + direction * j) % P for j in range(nblocks)]
        wraps = sum(1 for j in range(1, nblocks) if (start + direction * j) % P == (0 if direction > 0 else P - 1))
        assert wraps >= 1 and r["stats"][2 if direction > 0 else 3] == wraps and r["stats"][3 if direction > 0 else 2] == 0
        assert r["nbits"] == nblocks * L - direction * r["stats"][2 if direction > 0 else 3]


def test_the_model_streams_at_block_aligned_cuts():
    rng = np.random.default_rng(2)
    for P, L, taps in ((3, 8, [1]), (8, 16, [3, -1, 2, 5, 1]), (16, 8, list(range(-8, 9)))):
        n = L * P * 40 + int(rng.integers(1, L * P))
        x = rng.integers(-300, 300, n)
        want = M.run(x, P, taps, L, 4, 7, True, shift=1)
        assert want["stats"][1] > 5 and (P > 8 or want["stats"][2] + want["stats"][3] > 0)      # cuts fall between moves and wraps
        for _ in range(3):
            cuts = sorted(set((rng.integers(1, 41, 6) * L * P).tolist()))
            got = M.stream(x, P, cuts, taps, L=L, h=4, threshold=7, strict=True, shift=1)
            for key in ("bits", "soft", "phases"):
                assert np.array_equal(got[key], want[key]), key
            assert got["state"] == want["state"] and got["stats"] == want["stats"]


# ---- the host entry points ---------------------------------------------------------------------------------------------------

def _model_host(x, nb, cfg, state=(0, 0), final=True, soft_dtype=np.int16):
    lib = _lib.lib()
    x = np.ascontiguousarray(x, dtype=np.int16)
    nin = len(x) - nb
    nblocks, _, mb = M.plan(nin, cfg.spb, cfg.block_symbols or 64, final)
    bits = np.full((mb + 63) // 64, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    soft, ph = np.zeros(mb, dtype=soft_dtype), np.zeros(nblocks, dtype=np.uint8)
    st, stats, got = np.array(state, dtype=np.uint64), np.zeros(4, dtype=np.uint64), C.c_uint64()
    rc = lib.bbb_timing_model_host(C.c_void_p(x.ctypes.data + 2 * nb), nin, nb, int(final), C.byref(cfg), C.c_void_p(st.ctypes.data),
                                   C.c_void_p(bits.ctypes.data), C.c_void_p(soft.ctypes.data), C.c_void_p(ph.ctypes.data),
                                   C.c_void_p(stats.ctypes.data), C.byref(got))
    assert rc == 0, lib.bbb_last_error_detail()
    n = got.value
    return dict(bits=np.unpackbits(bits.view(np.uint8), bitorder="little")[:n], words=bits, soft=soft[:n], phases=ph,
                state=tuple(int(v) for v in st), stats=stats.tolist(), nbits=n)


def test_model_host_equals_the_model():
    rng = np.random.default_rng(3)
    for P, L, ntaps, n in ((3, 8, 1, 1000), (8, 0, 7, 30000), (16, 8, 33, 5000), (4, 8, 3, 700), (256, 8, 2, 2048 * 3 + 9), (5, 1024, 1, 5120 * 3)):
        taps = rng.integers(-50, 50, ntaps).tolist()
        nb = ntaps + 2
        x = rng.integers(-3000, 3000, n + nb)
        for final in (True, False):
            for init in (M.ACQUIRE, 0, P - 1):
                for ob, dt in ((2, np.int16), (4, np.int32)):
                    want = M.run(x[nb:], P, taps, L or 64, 3, 5, True, init, before=x[:nb], state=(0, 7), final=final, shift=2, out_bytes=ob)
                    got = _model_host(x, nb, _cfg(P, taps, L, 3, 5, True, init, shift=2, out_bytes=ob), (0, 7), final, dt)
                    for key in ("bits", "soft", "phases"):
                        assert np.array_equal(got[key], want[key]), (key, P, final, init)
                    assert got["state"] == want["state"] and got["stats"] == want["stats"] and got["nbits"] == want["nbits"]
                    assert np.array_equal(got["words"][:(got["nbits"] + 63) // 64], fir_model.pack(want["bits"])) and not got["words"][(got["nbits"] + 63) // 64:].any()
    # a locked state continues; nblocks 0 only rewrites the state
    got = _model_host(x, 0, _cfg(5, [1], 8, 1), (M.LOCKED | 3, 11))
    want = M.run(x, 5, [1], 8, 1, state=(M.LOCKED | 3, 11))
    assert got["state"] == want["state"] and np.array_equal(got["bits"], want["bits"]) and np.array_equal(got["phases"], want["phases"])
    assert abs(int(want["phases"][0]) - 3) <= 1                              # block 0 moved from the state's phase, it did not acquire
    assert _model_host(x[:39], 0, _cfg(5, [1], 8, 1), (M.LOCKED | 3, 11), final=False)["state"] == (M.LOCKED | 3, 11)


def test_plan():
    tr = bbb.TimingRecovery(8, [1, 2, 3])
    assert tr.plan(1000) == dict(nblocks=2, nconsumed=1000, max_bits=130, nbefore_wanted=3)
    assert tr.plan(1000, final=False) == dict(nblocks=1, nconsumed=512, max_bits=65, nbefore_wanted=3)
    assert tr.plan(0) == dict(nblocks=0, nconsumed=0, max_bits=0, nbefore_wanted=3)
    assert bbb.TimingRecovery(256, block_symbols=256).plan(65536 * 3 + 1)["nblocks"] == 4
    assert _lib.lib().bbb_timing_plan(C.byref(_cfg(8)), 100, 1, None, None, None, None) == 0
    assert _lib.lib().bbb_timing_plan(C.byref(_cfg(2)), 100, 1, None, None, None, None) == _lib.BBB_EINVAL


def test_invalid_arguments_return_before_the_device_is_touched():
    """Every pointer here is a number no device ever gave out: a call that got as far as the device would fail otherwise
    (BBB_ENODEV on a machine without a GPU), and the last cases show that a valid call does get that far."""
    import torch
    lib = _lib.lib()
    IN, BITS, SOFT, STATE, PH, STATS, NB = 1 << 20, 1 << 24, 1 << 26, 1 << 28, 1 << 29, 1 << 30, 1 << 31

    def rc(cfg, in_dev=IN, nin=4096, nb=0, final=1, state=STATE, bits=BITS, soft=None, phase=None, stats=None, nbits=NB):
        p = lambda v: C.c_void_p(v) if v else None                                                          # noqa: E731
        return lib.bbb_timing_run(p(in_dev), nin, nb, final, C.byref(cfg) if cfg is not None else None, p(state), p(bits), p(soft), p(phase),
                                  p(stats), p(nbits), 0, None)

    good = _cfg(8, [1, 1, 1, 1])
    bad = [(None, {}, "null"),
           (_cfg(2), {}, "spb"), (_cfg(257), {}, "spb"),
           (_cfg(8, L=7), {}, "block_symbols"), (_cfg(8, L=1025), {}, "block_symbols"), (_cfg(256, L=257), {}, "block_symbols"),
           (_cfg(8, h=64), {}, "hysteresis_shift"),
           (_cfg(8, init=8), {}, "init_phase"),
           (_cfg(8, decim=2), {}, "decim"), (_cfg(8, decim=2, phase=1), {}, "decim"),
           (_cfg(8, [32767, 32767, 2]), {}, "65535"),
           (_cfg(8, out_bytes=3), dict(soft=SOFT), "out_bytes"), (_cfg(8, shift=32), dict(soft=SOFT), "shift"),
           (good, dict(state=0), "state_dev"), (good, dict(bits=0), "bits_packed_dev"), (good, dict(in_dev=0), "in_dev"), (good, dict(nbits=0), "nbits_dev"),
           (good, dict(bits=BITS + 4), "misaligned"), (good, dict(soft=SOFT + 1), "misaligned"), (good, dict(state=STATE + 4), "misaligned"),
           (good, dict(stats=STATS + 4), "misaligned"), (good, dict(nbits=NB + 4), "misaligned"), (good, dict(in_dev=IN + 1), "misaligned"),
           (good, dict(bits=IN + 4096 * 2 - 8), "bits_packed_dev overlaps the samples"),
           (good, dict(soft=IN - 8 - 1040 + 2, nb=4), "soft_dev overlaps the samples"),               # the fourth history sample alone: the early instant's
           (good, dict(soft=IN + 64), "soft_dev overlaps the samples"),
           (good, dict(phase=IN + 3), "phase_dev overlaps the samples"),
           (good, dict(soft=BITS + 8), "soft_dev overlaps bits_packed_dev"),
           (good, dict(phase=BITS + 1), "phase_dev overlaps bits_packed_dev"),
           (good, dict(stats=BITS), "stats_dev overlaps bits_packed_dev"),
           (good, dict(nbits=STATE + 8), "state_dev overlaps nbits_dev"),
           (good, dict(stats=STATE - 24), "state_dev overlaps stats_dev")]
    for cfg, kw, what in bad:
        assert rc(cfg, **kw) == _lib.BBB_EINVAL, what
        assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    if not torch.cuda.is_available():
        assert rc(good) == _lib.BBB_ENODEV
        assert rc(_cfg(256, L=256, h=63, init=255), soft=SOFT, phase=PH, stats=STATS) == _lib.BBB_ENODEV
        assert rc(good, bits=IN + 4096 * 2, soft=IN - 520 * 2 - 8, nb=4) == _lib.BBB_ENODEV      # next to the samples, not in them
        assert rc(good, soft=IN - 8 - 1040 + 2, nb=3) == _lib.BBB_ENODEV                            # history that was not handed over is not read
        assert rc(good, bits=IN + 512 * 2 * 7, final=0, nin=4095) == _lib.BBB_ENODEV                # behind nconsumed: not read
        assert rc(good, nin=0, in_dev=0, bits=0) == _lib.BBB_ENODEV                                 # nothing to do but the state


def test_python_argument_checks():
    for kw, what in ((dict(spb=2), "spb"), (dict(spb=8, block_symbols=7), "block_symbols"), (dict(spb=256, block_symbols=512), "block_symbols"),
                     (dict(spb=8, hysteresis_shift=64), "hysteresis"), (dict(spb=8, init_phase=8), "init_phase"), (dict(spb=8, threshold=2 ** 31), "int32")):
        with pytest.raises(ValueError, match=what):
            bbb.TimingRecovery(**kw)
    tr = bbb.TimingRecovery(8, bbb.FIR([1, 2, 3], shift=2), 16, 3, threshold=3, strict=True, init_phase=5, chunk_blocks=9)
    c = tr._cfg(4)
    assert (c.ff.ntaps, c.ff.shift, c.ff.decim, c.ff.phase, c.ff.out_bytes) == (3, 2, 1, 0, 4)
    assert (c.spb, c.block_symbols, c.hysteresis_shift, c.threshold, c.strict, c.init_phase, c.chunk_blocks) == (8, 16, 3, 3, 1, 5, 9)
    assert bbb.TimingRecovery(8)._cfg().init_phase == M.ACQUIRE and bbb.TimingRecovery(8).ff.taps == [1]
    assert tr.stats() == dict(blocks=0, moves=0, wraps_up=0, wraps_down=0)
    for kw in (dict(rx_filter=bbb.FIR([1])), dict(stride=8), dict(dfe=bbb.DFE([1], [1], 8)), dict(mlse=bbb.MLSE([1], [100, 50], 8))):
        with pytest.raises(ValueError, match="excludes"):
            bbb.RX(7, 8, 0).slice(None, timing=tr, **kw)


def test_clock_offset_from_the_phase_track():
    tr = bbb.TimingRecovery(8)
    # one phase down every 6.4 blocks of 512 samples: 10 / 64 / 512 = 305 ppm, the closed loop's offset
    ph = (-(np.arange(512) * 10 // 64)) % 8
    assert abs(tr.clock_offset_ppm(ph) + 1e6 * 10 / 64 / 512) < 2.0
    assert abs(tr.clock_offset_ppm((np.arange(512) * 10 // 64) % 8) - 1e6 * 10 / 64 / 512) < 2.0
    assert abs(tr.clock_offset_ppm(np.full(100, 3))) < 1e-9 and tr.clock_offset_ppm([3]) == 0.0


# ---- the device's passes on the CPU, under the sanitizers ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("timing_host")
    exe = d / "timing_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", str(ROOT / "tests" / "timing_host.cpp"), "-o", str(exe)])
    return exe


def _blob(c):
    head = np.array([len(c["a"]) - 1, c["P"], c["L"], c["h"], c["threshold"], int(c["strict"]), c["init"], c["chunk"], 0, c["state1"], int(c["final"]), 0],
                    dtype=np.int64)
    head[8] = np.array([c["state0"]], dtype=np.uint64).view(np.int64)[0]
    a = np.zeros((len(c["a"]) + 1) // 2 * 2, dtype=np.int32)
    a[:len(c["a"])] = c["a"]
    return head.tobytes() + a.tobytes()


def _host_cases():
    rng = np.random.default_rng(4)
    cases = []

    def add(a, P, L, h=4, threshold=0, strict=False, init=M.ACQUIRE, chunk=1024, state0=0, state1=0, final=True):
        cases.append(dict(a=np.asarray(a, dtype=np.int64), P=P, L=L, h=h, threshold=threshold, strict=strict, init=init, chunk=chunk, state0=state0,
                          state1=state1, final=final))

    for P, L in ((3, 8), (4, 8), (8, 64), (16, 8), (3, 682), (3, 683), (255, 8), (256, 8), (256, 256), (64, 1024), (5, 9), (17, 120), (16, 128)):
        LP = L * P
        for n in (1, LP - 1, LP, LP + 1, 37 * LP + LP // 3) if LP <= 4096 else (LP + 1, 3 * LP + 77):
            add(rng.integers(-2000, 2000, n + 1), P, L, h=int(rng.integers(1, 6)), threshold=int(rng.integers(-50, 50)), strict=bool(n & 1),
                init=int(rng.choice([M.ACQUIRE, 0, P - 1])), chunk=int(rng.choice([1, 3, 1024])), final=bool(rng.integers(0, 2)))
    for P, d in ((4, 1), (4, -1), (256, 1), (255, -1)):                        # ramps: a move in every block
        add(np.concatenate([[5], M.ramp(P, 8, 3 * P // 2 + 4 if P < 16 else 6, d, 0 if d < 0 else P - 1)]), P, 8, init=0 if d < 0 else P - 1, chunk=3)
    add(np.zeros(8 * 8 * 50 + 1), 8, 8, chunk=3)                               # every comparison ties
    add(rng.integers(-2 ** 31 + 32768, 2 ** 31 - 32768, 3 * 1024 * 8 + 1), 8, 1024, threshold=-2 ** 31, chunk=1)       # the int64 bound
    add(rng.integers(-500, 500, 3000), 8, 16, state0=M.LOCKED | 6, state1=12345, chunk=2)                               # a locked state goes on
    add(rng.integers(-500, 500, 100), 8, 16, state0=M.LOCKED | 6, state1=5, final=False)                                # no block at all
    return cases


def test_the_passes_on_the_cpu_equal_the_model(host_exe, tmp_path):
    cases = _host_cases()
    (tmp_path / "c.bin").write_bytes(b"".join(_blob(c) for c in cases))
    r = subprocess.run([str(host_exe), str(tmp_path / "c.bin"), str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"cases {len(cases)}" in r.stdout, (r.stdout, r.stderr[-3000:])
    lines = (tmp_path / "o.txt").read_text().split("\n")
    ups = downs = 0
    for i, c in enumerate(cases):
        # the model over a(n) itself: one tap {1}, a(-1) as its history
        a = c["a"]
        want = M.run(a[1:], c["P"], [1], c["L"], c["h"], c["threshold"], c["strict"], c["init"], before=a[:1], state=(c["state0"], c["state1"]),
                     final=c["final"], out_bytes=4)
        head = [int(t) for t in lines[4 * i].split()]
        assert head == [want["state"][0], want["state"][1], want["nbits"]] + want["stats"], (i, head, want["state"], want["stats"])
        words = [int(t, 16) for t in lines[4 * i + 1].split()]
        nw = (want["nbits"] + 63) // 64
        assert words[:nw] == fir_model.pack(want["bits"]).tolist() and not any(words[nw:]), i
        assert [int(t) for t in lines[4 * i + 2].split()] == want["phases"].tolist(), i
        assert [int(t) for t in lines[4 * i + 3].split()] == want["soft"].tolist(), i
        ups += want["stats"][2]
        downs += want["stats"][3]
    assert ups >= 4 and downs >= 4          # the ramps alone: three at P 4, one at P 255 / 256, each way


# ---- the closed loop on the CPU ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", M.LOOP["steps"])
def test_closed_loop_on_the_oracle_waveform(oracle, step):
    """A clock offset of 20 / 65536 (305 ppm) slips one sample every 3277: over 2^18 samples the eye passes through every
    fixed phase, and the tracker follows it with one wrap per eight slipped samples."""
    L = M.LOOP
    x, ref = M.loop_waveform(oracle)
    y = M.resample(x, step, L["n"])
    r = M.run(y, L["P"], L=L["L"], h=L["h"])
    errors, lag = M.loop_errors(r["bits"], ref, M.loop_compare_bits())
    fixed, phase = M.fixed_phase_errors(y, ref)
    ppm = bbb.TimingRecovery(L["P"]).clock_offset_ppm(r["phases"])
    print("step", step, "emitted", r["nbits"], "stats", r["stats"], "errors", errors, "of", M.loop_compare_bits(), "at lag", lag,
          "best fixed phase", phase, "leaves", fixed, "clock offset", ppm, "ppm")
    assert errors <= M.LOOP_MAX_ERRORS
    assert fixed > M.LOOP_MIN_FIXED_ERRORS
    up, down = r["stats"][2], r["stats"][3]
    assert (down, up) == ((M.LOOP_WRAPS, 0) if step > 65536 else (0, M.LOOP_WRAPS))
    assert r["nbits"] == L["n"] // L["P"] + down - up
    assert abs(ppm - (65536 - step) / 65536 * 1e6) < 15.0


# ---- past one pass of the grids ----------------------------------------------------------------------------------------------------
# The metric and gather kernels take tiles of 2048 samples, the chunk and walk kernels chunks of blocks, each at most 8
# workgroups per compute unit at a time (tests/grid.py).  These records take all four past two passes and leave the last pass
# ragged; tests/test_gpu_timing.py runs them on the GPU.  The expected values are bbb_timing_model_host's, held to the model here
# on three stretches of blocks, each entered with the state the host model left in front of it (the phase of the block before
# and the bits emitted so far, which the phases of whole blocks give).  spb = 2 is refused by bbb_timing_run, so the smallest
# block is 8 symbols of 3 samples, 85 of them a tile.
MULTIPASS = {"small_blocks": dict(P=3, L=8), "long_blocks": dict(P=8, L=1024)}
MULTIPASS_H, MULTIPASS_THRESHOLD, MULTIPASS_SHIFT = 4, 11, 2


def multipass_record(name, ncus):
    """(samples, taps, P, L, chunk_blocks, nblocks) of the drifting-noise record (timing_model.drift_record).
    small_blocks: 2 * 8 * ncus + 5 tiles, the last with 7 blocks of which the last is cut short, and chunks of as many blocks as
    make more chunks than tiles, so that a chain thread's share is several chunks.
    long_blocks: 8 * ncus + 3 blocks of four tiles each, the last block cut short, one block a chunk."""
    P, L = MULTIPASS[name]["P"], MULTIPASS[name]["L"]
    LP = L * P
    rng = np.random.default_rng(90 + P)
    if name == "small_blocks":
        per_tile, ntiles = 2048 // LP, grid.passes(grid.TIMING, ncus=ncus)
        nblocks = per_tile * (ntiles - 1) + 7
        n, chunk = (nblocks - 1) * LP + 11, nblocks // ntiles
        assert -(-nblocks // per_tile) == ntiles and -(-nblocks // chunk) > 2 * grid.TIMING * ncus
    else:
        assert LP > 2048
        nblocks, chunk = grid.passes(grid.TIMING, k=1, extra=3, ncus=ncus), 1
        n = (nblocks - 1) * LP + 4099
    return M.drift_record(rng, P, L, n).astype(np.int16), M.phase_taps(rng, 7, P), P, L, chunk, nblocks


def multipass_expected(name, ncus):
    """(samples, taps, P, L, chunk_blocks, the host model's dict): the whole record from bbb_timing_model_host, held to the model on
    the blocks around the start of pass 2 of the metric kernel, on blocks inside pass 3 (of the gather kernel's tiles, where a
    block is several) and on the ragged end.  The record moves and wraps both ways."""
    x, taps, P, L, chunk, nblocks = multipass_record(name, ncus)
    h, thr, shift, LP = MULTIPASS_H, MULTIPASS_THRESHOLD, MULTIPASS_SHIFT, L * P
    want = _model_host(x, 0, _cfg(P, taps, L, h, thr, True, M.ACQUIRE, chunk, shift=shift))
    assert want["stats"][0] == nblocks and want["stats"][1] > 8 and want["stats"][2] >= 1 and want["stats"][3] >= 1, want["stats"]
    ph = want["phases"].astype(np.int64)
    d = np.diff(ph)
    wraps = np.concatenate([[0], (d == 1 - P).astype(np.int64) - (d == P - 1)])      # P - 1 -> 0 is up, 0 -> P - 1 is down
    per = grid.TIMING * ncus * (2048 // LP if LP <= 2048 else 1)                     # blocks in a pass of the metric kernel
    third = 2 * per + 3 if LP <= 2048 else 2 * grid.TIMING * ncus * 2048 // LP + 1   # ... and a block of the gather kernel's pass 3
    for j0, j1 in ((per - 2, per + 2), (third, third + 3), (nblocks - 3, None)):
        off = L * j0 - int(wraps[:j0].sum())
        r = M.run(x[j0 * LP:j1 * LP if j1 else None], P, taps, L, h, thr, True, before=x[j0 * LP - len(taps):j0 * LP],
                  state=(M.LOCKED | int(ph[j0 - 1]), off), final=j1 is None, shift=shift)
        assert np.array_equal(r["phases"], want["phases"][j0:j1]), (name, j0)
        assert np.array_equal(r["bits"], want["bits"][off:off + r["nbits"]]) and np.array_equal(r["soft"], want["soft"][off:off + r["nbits"]]), (name, j0)
        if j1 is None:
            assert r["state"] == want["state"] and off + r["nbits"] == want["nbits"]
        else:
            assert r["nbits"] == L * (j1 - j0) - int(wraps[j0:j1].sum())
    return x, taps, P, L, chunk, want


@pytest.mark.parametrize("name", sorted(MULTIPASS))
def test_multipass_host_model_equals_the_model_on_stretches(name):
    x, taps, P, L, chunk, want = multipass_expected(name, 256)
    assert len(want["phases"]) == -(-len(x) // (L * P))
