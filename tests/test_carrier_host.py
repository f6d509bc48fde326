"""The carrier recovery without a GPU: the model against the serial rule written out literally, bbb_carrier_model_host against
the model, bbb_carrier_plan and the argument checks of bbb_carrier_run through the C ABI, the scan identity the device's
formulation rests on, the model's streaming property, the five passes of the device restated on the CPU over
basebandboard_amd/csrc/carrier_common.hpp under ASan/UBSan, and the closed loop: the down-converter's example with the two
oscillators 15 ppm apart, where the sign of Q decides nothing and the block estimator leaves no error."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from conftest import ROOT

import carrier_model as M
import ddc_model
import nco_model


def _cfg(L=0, init=0, threshold=0, strict=False, chunk=0):
    return _lib.CarrierCfg(L, init, threshold, int(strict), chunk)


# ---- the model -------------------------------------------------------------------------------------------------------------

def _definition(pairs, L, init, thr, strict, state, final):
    """The header's definition over Python ints, one pair at a time."""
    rom = nco_model.ROM.tolist()
    x = [(int(i), int(q)) for i, q in pairs]
    nblocks = -(-len(x) // L) if final else len(x) // L
    x = x[:nblocks * L]
    est = state[0] & 0xFFFF if state[0] >> 63 else init
    out, phases, stats = [], [], [0, 0, 0, 0]
    for j in range(nblocks):
        blk = x[j * L:(j + 1) * L]
        sr, si = sum(i * i - q * q for i, q in blk), 2 * sum(i * q for i, q in blk)
        s = max(0, max(abs(sr), abs(si)).bit_length() - 15)
        th = int(ddc_model.cordic(sr >> s, si >> s)[1][0])
        h = (th % 65536) >> 1
        d = (h - est) % 65536
        nxt = h if d < 16384 or d >= 49152 else (h + 32768) % 65536
        step = (nxt - est + 32768) % 65536 - 32768
        stats = [stats[0] + 1, stats[1] + ((nxt >> 15) != (est >> 15)), stats[2] + (sr == 0 and si == 0), stats[3] + step]
        est = nxt
        phases.append(est)
        c, sn = rom[((est >> 6) + 256) % 1024], rom[est >> 6]
        out += [(min(max((i * c + q * sn) >> 15, -32768), 32767), min(max((q * c - i * sn) >> 15, -32768), 32767)) for i, q in blk]
    st = ((M.STARTED | est) if nblocks else state[0], state[1] + len(x))
    return out, phases, stats, st


def test_model_equals_the_definition_term_by_term():
    rng = np.random.default_rng(1)
    flips = 0
    for L, n, init, thr, strict, state, final in ((8, 8 * 30 + 5, 0, 0, False, (0, 0), True), (24, 24 * 20, 40000, 3, True, (0, 5), True),
                                                    (32, 32 * 9 + 31, 16384, -7, False, (M.STARTED | 50000, 77), False), (8, 1, 65535, 0, True, (0, 0), True),
                                                    (16, 15, 1, 0, False, (M.STARTED | 3, 9), False), (1024, 2100, 0, 100, False, (0, 0), True)):
        x = rng.integers(-32768, 32768, (n, 2))
        x[3::50] = (-32768, -32768)
        if L == 8:
            x[8:24] = 0                                                         # two zero blocks
        want, phases, stats, st = _definition(x, L, init, thr, strict, state, final)
        r = M.run(x, L, init, thr, strict, state, final)
        assert r["iq"].tolist() == [list(p) for p in want] and r["phases"].tolist() == phases and r["stats"] == stats and r["state"] == st, (L, n)
        assert r["soft"].tolist() == [p[0] for p in want]
        assert r["bits"].tolist() == [int(p[0] > thr if strict else p[0] >= thr) for p in want]
        assert np.array_equal(np.unpackbits(r["words"].view(np.uint8), bitorder="little")[:len(want)], r["bits"])
        assert not np.unpackbits(r["words"].view(np.uint8), bitorder="little")[len(want):].any()
        flips += stats[1]
    assert flips > 10                                                           # the cases do change sides
    assert M.plan(100, 32) == (4, 100) and M.plan(100, 32, final=False) == (3, 96) and M.plan(0, 8) == (0, 0) and M.plan(7, 8, final=False) == (0, 0)
    assert M.bitlength([0, 1, 2, 3, 32767, 32768, 2 ** 41 - 1, 2 ** 41]).tolist() == [0, 1, 2, 2, 15, 16, 41, 42]


def test_full_scale_pairs_and_the_bounds_of_the_sums():
    """1024 pairs of (-32768, -32768): SI = 2^41, which is why I * Q is summed and the sum doubled; SR = 0.  1024 pairs of
    (-32768, 0): SR = 2^40.  Either is normalised into int16 and the derotation of a pair on the diagonal saturates."""
    x = np.full((1024, 2), -32768)
    h, zero = M.block_h(x, 1024, 1)
    assert (2 * (x[:, 0] * x[:, 1]).sum()) == 2 ** 41 and h.tolist() == [8192] and not zero[0]
    r = M.run(x, 1024, init_phase=8192 + 32768)                                # est = 5/8 turn: the pair is turned onto +I and saturates
    # (Q' is what one step of the ROM, 1/1023 turn, leaves of a vector of length 46341: at most 285)
    assert r["phases"].tolist() == [8192 + 32768] and (r["iq"][:, 0] == 32767).all() and np.abs(r["iq"][:, 1]).max() <= 285
    assert (M.run(x, 1024, init_phase=8192)["iq"][:, 0] == -32768).all()
    y = np.zeros((1024, 2), dtype=np.int64)
    y[:, 0] = -32768
    assert M.block_h(y, 1024, 1)[0].tolist() == [0]


def test_the_scan_identity():
    """est_j = h_j + 32768 b_j with b_j = b_(j-1) XOR f_j, f_j = !near(h_j - h_(j-1)), against the serial rule: random full-range
    h at three block counts and every est_(-1) of a stride; and wrap16(est_j - est_(j-1)) = wrap16(h_j - h_(j-1) + 32768 f_j)."""
    rng = np.random.default_rng(2)
    near = lambda d: (d % 65536 < 16384) | (d % 65536 >= 49152)                                            # noqa: E731
    for n in (1, 7, 3000):
        h = rng.integers(0, 32768, n)
        h[::11] = (h[::11] // 16384) * 16384                                   # ties
        for est0 in list(range(0, 65536, 4099)) + [16383, 16384, 32767, 32768, 49151, 49152, 65535]:
            est, flips, steps = M.unwrap(h, est0)
            hp = np.concatenate([[est0 & 0x7FFF], h[:-1]])
            f = (~near(h - hp)).astype(np.int64)
            b = (est0 >> 15) ^ (np.cumsum(f) & 1)
            assert np.array_equal(est, h + 32768 * b), (n, est0)
            w = (h - hp + 32768 * f + 32768) % 65536 - 32768
            assert flips == f.sum() and steps == w.sum()


def test_the_model_streams_at_block_aligned_cuts():
    rng = np.random.default_rng(3)
    for L in (8, 24, 1024):
        n = L * 40 + int(rng.integers(1, L))
        x = rng.integers(-20000, 20000, (n, 2))
        want = M.run(x, L, 777, 5, True)
        for _ in range(3):
            cuts = sorted(set((rng.integers(1, 41, 5) * L).tolist()))
            got = M.stream(x, cuts, L, init_phase=777, threshold=5, strict=True)
            for key in ("iq", "bits", "soft", "phases"):
                assert np.array_equal(got[key], want[key]), key
            assert got["state"] == want["state"] and got["stats"] == want["stats"]


# ---- the host entry points ---------------------------------------------------------------------------------------------------

def model_host(pairs, L=32, init=0, threshold=0, strict=False, state=(0, 0), final=True, chunk=0):
    """bbb_carrier_model_host: the dict of carrier_model.run."""
    lib = _lib.lib()
    x = np.ascontiguousarray(pairs, dtype=np.int16).reshape(-1, 2)
    nblocks, n = M.plan(len(x), L or 32, final)
    iq, soft, ph = np.zeros((n, 2), dtype=np.int16), np.zeros(n, dtype=np.int16), np.zeros(nblocks, dtype=np.uint16)
    words = np.full((nblocks * (L or 32) + 63) // 64, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    st, stats = np.array(state, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    p = lambda a: C.c_void_p(a.ctypes.data)                                                                # noqa: E731
    cfg = _cfg(L, init, threshold, strict, chunk)
    rc = lib.bbb_carrier_model_host(p(x), len(x), int(final), C.byref(cfg), p(st), p(iq), p(words), p(soft), p(ph), p(stats))
    assert rc == 0, lib.bbb_last_error_detail()
    return dict(iq=iq, bits=np.unpackbits(words.view(np.uint8), bitorder="little")[:n], words=words, soft=soft, phases=ph,
                state=tuple(int(v) for v in st), stats=[int(v) for v in stats[:3]] + [int(stats.view(np.int64)[3])], nblocks=nblocks, nconsumed=n)


def same(got, want, what=""):
    for key in ("iq", "words", "soft", "phases"):
        bad = np.flatnonzero(np.asarray(got[key]).reshape(-1) != np.asarray(want[key]).reshape(-1))
        assert len(bad) == 0, f"{what}: {key} differs in {len(bad)} places, the first at {bad[0]}"
    assert got["state"] == want["state"], f"{what}: state {got['state']} != {want['state']}"
    assert got["stats"] == want["stats"], f"{what}: stats {got['stats']} != {want['stats']}"


def test_model_host_equals_the_model():
    rng = np.random.default_rng(4)
    for L in (8, 24, 32, 1024):
        for n in (1, L - 1, L, L + 1, 40 * L + 3):
            for final in (True, False):
                x = rng.integers(-32768, 32768, (n, 2))
                x[3::61] = (-32768, -32768)
                for state in ((0, 7), (M.STARTED | 40000, 1 << 40)):
                    same(model_host(x, L, 12345, 5, True, state, final), M.run(x, L, 12345, 5, True, state, final), f"L {L} n {n} final {final}")
    assert model_host(np.zeros((31, 2)), 32, 9, state=(M.STARTED | 3, 11), final=False)["state"] == (M.STARTED | 3, 11)
    assert model_host(np.zeros((64, 2)), 0, 9)["stats"] == [2, 0, 2, -9]        # block_pairs 0: 32; zero blocks give h = 0


def test_plan():
    cr = bbb.CarrierRecovery()
    assert cr.plan(100) == dict(nblocks=4, nconsumed=100) and cr.plan(100, final=False) == dict(nblocks=3, nconsumed=96)
    assert cr.plan(0) == dict(nblocks=0, nconsumed=0) and bbb.CarrierRecovery(1024).plan(1023, final=False) == dict(nblocks=0, nconsumed=0)
    lib = _lib.lib()
    assert lib.bbb_carrier_plan(C.byref(_cfg(8)), 100, 1, None, None) == 0
    for bad in (_cfg(7), _cfg(12), _cfg(1032), _cfg(8, init=65536)):
        assert lib.bbb_carrier_plan(C.byref(bad), 100, 1, None, None) == _lib.BBB_EINVAL
    assert lib.bbb_carrier_plan(C.byref(_cfg(8)), (1 << 58) + 1, 1, None, None) == _lib.BBB_EINVAL


IN, IQ, BITS, SOFT, STATE, PH, STATS = 1 << 20, 1 << 24, 1 << 26, 1 << 27, 1 << 28, 1 << 29, 1 << 30


def run_rc(cfg, in_dev=IN, nin=4096, final=1, state=STATE, iq=IQ, bits=None, soft=None, phase=None, stats=None):
    """bbb_carrier_run with pointers that no device ever gave out."""
    p = lambda v: C.c_void_p(v) if v else None                                                          # noqa: E731
    return _lib.lib().bbb_carrier_run(p(in_dev), nin, final, C.byref(cfg) if cfg is not None else None, p(state), p(iq), p(bits), p(soft), p(phase),
                                      p(stats), 0, None)


INVALID = [(None, {}, "null"),
           (_cfg(7), {}, "block_pairs"), (_cfg(20), {}, "block_pairs"), (_cfg(1032), {}, "block_pairs"), (_cfg(4), {}, "block_pairs"),
           (_cfg(8, init=65536), {}, "init_phase"),
           (_cfg(), dict(nin=(1 << 58) + 1), "2\\^58"),
           (_cfg(), dict(state=0), "state_dev"), (_cfg(), dict(in_dev=0), "in_dev"), (_cfg(), dict(iq=0), "no output"),
           (_cfg(), dict(in_dev=IN + 2), "misaligned"), (_cfg(), dict(iq=IQ + 2), "misaligned"), (_cfg(), dict(bits=BITS + 4), "misaligned"),
           (_cfg(), dict(soft=SOFT + 1), "misaligned"), (_cfg(), dict(phase=PH + 1), "misaligned"), (_cfg(), dict(state=STATE + 4), "misaligned"),
           (_cfg(), dict(stats=STATS + 4), "misaligned"),
           (_cfg(), dict(iq=IN + 4096 * 4 - 4), "iq_dev overlaps the pairs"), (_cfg(), dict(iq=IN - 4096 * 4 + 4), "iq_dev overlaps the pairs"),
           (_cfg(), dict(bits=IN + 8), "bits_packed_dev overlaps the pairs"), (_cfg(), dict(soft=IN - 8190), "soft_dev overlaps the pairs"),
           (_cfg(), dict(phase=IN + 4096 * 4 - 2), "phase_dev overlaps the pairs"), (_cfg(), dict(stats=IN - 24), "stats_dev overlaps the pairs"),
           (_cfg(), dict(state=IN + 16), "state_dev overlaps the pairs"),
           (_cfg(), dict(bits=IQ + 8), "bits_packed_dev overlaps iq_dev"), (_cfg(), dict(soft=IQ + 4096 * 4 - 2), "soft_dev overlaps iq_dev"),
           (_cfg(), dict(bits=BITS, soft=BITS + 504), "soft_dev overlaps bits_packed_dev"), (_cfg(), dict(phase=IQ), "phase_dev overlaps iq_dev"),
           (_cfg(), dict(soft=SOFT, phase=SOFT + 8190), "phase_dev overlaps soft_dev"), (_cfg(), dict(stats=IQ + 8), "stats_dev overlaps iq_dev"),
           (_cfg(), dict(stats=STATE - 24), "state_dev overlaps stats_dev"), (_cfg(), dict(state=IQ + 64), "state_dev overlaps iq_dev")]


def test_invalid_arguments_return_before_the_device_is_touched():
    """Every pointer here is a number no device ever gave out: a call that got as far as the device would fail otherwise
    (BBB_ENODEV on a machine without a GPU), and the last cases show that a valid call does get that far."""
    import torch
    lib = _lib.lib()
    for cfg, kw, what in INVALID:
        assert run_rc(cfg, **kw) == _lib.BBB_EINVAL, what
        assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    if not torch.cuda.is_available():
        assert run_rc(_cfg()) == _lib.BBB_ENODEV
        assert run_rc(_cfg(1024, 65535, -5, True, 3), bits=BITS, soft=SOFT, phase=PH, stats=STATS) == _lib.BBB_ENODEV
        assert run_rc(_cfg(), iq=IN + 4096 * 4, soft=IN - 8192) == _lib.BBB_ENODEV                 # next to the pairs, not in them
        assert run_rc(_cfg(), iq=IN + 4064 * 4, nin=4095, final=0) == _lib.BBB_ENODEV              # behind nconsumed: not read
        assert run_rc(_cfg(), iq=0, phase=PH) == _lib.BBB_ENODEV                                   # the phases alone are an output
        assert run_rc(_cfg(), nin=0, in_dev=0) == _lib.BBB_ENODEV                                  # nothing to do but the state


def test_python_argument_checks():
    for kw, what in ((dict(block_pairs=12), "block_pairs"), (dict(block_pairs=2048), "block_pairs"), (dict(init_phase=65536), "init_phase"),
                     (dict(init_phase=-1), "init_phase"), (dict(threshold=2 ** 31), "int32")):
        with pytest.raises(ValueError, match=what):
            bbb.CarrierRecovery(**kw)
    cr = bbb.CarrierRecovery(64, 16384, threshold=-3, strict=True, chunk_blocks=9)
    c = cr._cfg()
    assert (c.block_pairs, c.init_phase, c.threshold, c.strict, c.chunk_blocks) == (64, 16384, -3, 1, 9)
    assert bbb.CarrierRecovery().L == 32 and cr.stats() == dict(blocks=0, flips=0, zero_blocks=0, phase_steps=0) and cr.carrier_offset() == 0.0
    with pytest.raises(ValueError, match="pairs must be"):
        cr.derotate(np.zeros((8, 2), dtype=np.int16))
    with pytest.raises(ValueError, match="outputs"):
        bbb.CarrierStream(cr, "soft")


# ---- the device's passes on the CPU, under the sanitizers ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("carrier_host")
    exe = d / "carrier_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", str(ROOT / "tests" / "carrier_host.cpp"), "-o", str(exe)])
    return exe


def _blob(c):
    head = np.array([len(c["x"]), c["L"], c["init"], c["threshold"], int(c["strict"]), c["chunk"], 0, c["state"][1], int(c["final"])], dtype=np.int64)
    head[6] = np.array([c["state"][0]], dtype=np.uint64).view(np.int64)[0]
    x = np.zeros((2 * len(c["x"]) + 3) // 4 * 4, dtype=np.int16)
    x[:2 * len(c["x"])] = c["x"].reshape(-1)
    return head.tobytes() + x.tobytes()


_TIES = {}


def tie_blocks(L):
    """Blocks of one constant vector each, at angles searched so that h_j - h_(j-1) modulo 2^16 takes the values 16383, 16384,
    49151 and 49152, the four edges of near(), and their neighbours 16385 and 49153.  Returns (pairs, the h of every block)."""
    if L not in _TIES:                                                         # (h depends on L: the sums are normalised)
        ang = np.arange(1 << 17) / float(1 << 18)                              # the vector's angle in turns, over half a turn
        v = np.stack([np.round(15000 * np.cos(2 * np.pi * ang)), np.round(15000 * np.sin(2 * np.pi * ang))], axis=1).astype(np.int64)
        h = M.block_h(np.repeat(v, L, axis=0), L, len(v))[0]
        by_h = {int(x): i for i, x in enumerate(h.tolist())}
        base = next(a for a in range(100, 16000) if all(a + d in by_h for d in (0, 16383, 16384, 16385)))
        seq = [base, base + 16383, base, base + 16384, base, base + 16385, base, base + 16384, base]
        _TIES[L] = (v[[by_h[x] for x in seq]], seq)
    return np.repeat(_TIES[L][0], L, axis=0), list(_TIES[L][1])


def host_cases():
    rng = np.random.default_rng(5)
    cases = []

    def add(x, L, init=0, threshold=0, strict=False, chunk=1024, state=(0, 0), final=True):
        cases.append(dict(x=np.asarray(x, dtype=np.int16).reshape(-1, 2), L=L, init=init, threshold=threshold, strict=strict, chunk=chunk, state=state, final=final))

    for L in (8, 16, 24, 32, 40, 64, 128, 192, 1000, 1024):
        tile = 2048 // L * L
        for n in (1, L - 1, L, L + 1, tile - 1, tile, tile + 1, 3 * tile + 5 * L + 3):
            x = rng.integers(-32768, 32768, (n, 2))
            x[3::61] = (-32768, -32768)
            add(x, L, int(rng.integers(0, 65536)), int(rng.integers(-50, 50)), bool(n & 1), int(rng.choice([1, 3, 1024])), final=bool(rng.integers(0, 2)))
    add(rng.integers(-3000, 3000, (8 * 3000 + 5, 2)), 8, chunk=1)                # more chunks than chain threads: shares of 12
    add(rng.integers(-3000, 3000, (8 * 700, 2)), 8, chunk=300)                   # chunks that end inside a thread's 8 blocks
    add(rng.integers(-3000, 3000, (8 * 5000, 2)), 8, chunk=4500)                 # a chunk of more than one turn of 2048 blocks
    add(np.zeros((8 * 50 + 3, 2)), 8, init=40000, chunk=3)                       # zero blocks: h = 0
    for init in (0, 32768, 16384, 49152):
        add(tie_blocks(24)[0], 24, init=init, chunk=3)
    add(rng.integers(-500, 500, (300, 2)), 32, state=(M.STARTED | 54321, 12345), chunk=2)       # a started state goes on
    add(rng.integers(-500, 500, (31, 2)), 32, state=(M.STARTED | 6, 5), final=False)            # no block at all
    x = np.full((64, 2), -32768)
    add(x, 32, init=8192 + 32768)                                                # saturates
    return cases


def test_the_passes_on_the_cpu_equal_the_model(host_exe, tmp_path):
    cases = host_cases()
    (tmp_path / "c.bin").write_bytes(b"".join(_blob(c) for c in cases))
    (tmp_path / "rom.bin").write_bytes(nco_model.ROM.astype(np.int16).tobytes())
    r = subprocess.run([str(host_exe), str(tmp_path / "c.bin"), str(tmp_path / "o.txt"), str(tmp_path / "rom.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"cases {len(cases)}" in r.stdout, (r.stdout, r.stderr[-3000:])
    lines = (tmp_path / "o.txt").read_text().split("\n")
    flips = zeros = sat = 0
    for i, c in enumerate(cases):
        want = M.run(c["x"], c["L"], c["init"], c["threshold"], c["strict"], c["state"], c["final"])
        same(model_host(c["x"], c["L"], c["init"], c["threshold"], c["strict"], c["state"], c["final"], c["chunk"]), want, f"host model, case {i}")
        head = [int(t) for t in lines[5 * i].split()]
        assert head == list(want["state"]) + want["stats"], (i, head, want["state"], want["stats"])
        assert [int(t, 16) for t in lines[5 * i + 1].split()] == want["words"].tolist(), i
        assert [int(t) for t in lines[5 * i + 2].split()] == want["phases"].tolist(), i
        assert [int(t) for t in lines[5 * i + 3].split()] == want["iq"].reshape(-1).tolist(), i
        assert [int(t) for t in lines[5 * i + 4].split()] == want["soft"].tolist(), i
        flips, zeros, sat = flips + want["stats"][1], zeros + want["stats"][2], sat + int((np.abs(want["iq"].astype(np.int64)) >= 32767).sum())
    assert flips > 1000 and zeros >= 50 and sat >= 64


def test_the_tie_blocks_hit_the_boundaries_of_near():
    x, hs = tie_blocks(8)
    d = [(b - a) % 65536 for a, b in zip(hs[:-1], hs[1:])]
    assert {16383, 16384, 49151, 49152} <= set(d), d
    assert M.block_h(x, 8, len(hs))[0].tolist() == hs
    # f_j by the definition of near(): 0 for the steps 0, 16383, 49153 and 49152, 1 for 16384, 16385 and 49151
    r = M.run(x, 8, init_phase=hs[0])
    b = (r["phases"].astype(np.int64) >> 15).tolist()
    assert [u ^ v for u, v in zip([0] + b[:-1], b)] == [0, 0, 0, 1, 0, 1, 1, 1, 0], r["phases"]


# ---- the closed loop on the CPU ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def loop():
    return M.loop_capture()


@pytest.mark.parametrize("off", M.LOOP["offsets"])
def test_closed_loop_on_the_model_waveform(loop, off):
    """The converter's fcw 256 off the transmitter's: 15 ppm of the sample rate, one turn of the baseband vector per 1024 bits.
    The sign of Q is right and wrong in turns; the block estimator with init_phase 16384 returns the data."""
    capture, data = loop
    pairs = M.loop_pairs(capture, off)
    assert len(pairs) == 4095
    r = M.run(pairs, M.LOOP["L"], M.LOOP["init_phase"])
    errors = int((r["bits"] != data[:4095]).sum())
    q_errors = int(((pairs[:, 1] > 0) != (data[:4095] == 1)).sum())
    offset = r["stats"][3] / (r["stats"][0] * M.LOOP["L"] * 65536.0)
    print("offset", off, "errors", errors, "of 4095, the sign of Q leaves", q_errors, "stats", r["stats"], "carrier offset", offset, "ideal", M.loop_ideal_offset(off))
    assert errors < 0.01 * 4095
    assert q_errors > 0.40 * 4095
    assert offset * off > 0 and abs(offset - M.loop_ideal_offset(off)) < 0.02 * abs(M.loop_ideal_offset(off))
    same(model_host(pairs, M.LOOP["L"], M.LOOP["init_phase"]), r, "host model")
