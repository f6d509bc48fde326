"""The frame synchroniser without a GPU: pins that do not come from the model, the model against the literal transcription of
its rules on every stream of 20 bits, bbb_framesync_model_host / bbb_frame_extract_host / bbb_frame_attach_host against the model on the
grid, cutting invariance, the argument checks of the device entry points through the C ABI, the Python argument checks, the
kernels' per-lane core (basebandboard_amd/csrc/framesync_common.hpp) called from a restatement of the kernels' walks on the CPU
under ASan/UBSan, and the closed loop RS -> markers -> convolutional code -> inverted noisy channel -> Viterbi -> find -> RS."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from conftest import ROOT

import grid
import framesync_model as M

GUARD = 0xA5A5A5A5A5A5A5A5


def cfg_of(c):
    k = _lib.FrameSyncCfg()
    k.marker, k.marker_bits, k.frame_bits, k.tol_search, k.tol_lock, k.verify, k.flywheel = c.marker, c.M, c.F, c.tol_search, c.tol_lock, c.v, c.w
    k.both_polarities = int(c.both)
    if c.rand is not None:
        k.rand_poly, k.rand_seed = c.rand
    return k


def host_run(c, bits, first_bit=0, final=True, state=None, max_frames=None):
    """bbb_framesync_model_host between guards: (pos, meta, the eight state words)."""
    lib = _lib.lib()
    mf = len(bits) // c.F + 2 if max_frames is None else max_frames
    words = np.concatenate([[GUARD], M.pack(bits), [GUARD]]).astype(np.uint64)
    before = words.copy()
    st = np.array([GUARD] + (state if state is not None else [0, first_bit, 0, 0, 0, 0, 0, 0]) + [GUARD], dtype=np.uint64)
    pos = np.full(mf + 2, GUARD, dtype=np.uint64)
    meta = np.full(mf + 2, 0xA5A5, dtype=np.uint16)
    rc = lib.bbb_framesync_model_host(C.c_void_p(words[1:].ctypes.data), len(bits), first_bit, int(final), C.byref(cfg_of(c)),
                                      C.c_void_p(st[1:].ctypes.data), C.c_void_p(pos[1:].ctypes.data), C.c_void_p(meta[1:].ctypes.data), mf)
    assert rc == 0, lib.bbb_last_error_detail()
    assert np.array_equal(words, before) and st[0] == st[-1] == GUARD and pos[0] == pos[-1] == GUARD and meta[0] == meta[-1] == 0xA5A5
    n = min(int(st[1]) >> 32, mf)
    assert (pos[1 + n:] == GUARD).all() and (meta[1 + n:] == 0xA5A5).all()
    return pos[1:1 + n].tolist(), meta[1:1 + n].tolist(), st[1:-1].tolist()


# ---- pins that do not come from the model -------------------------------------------------------------------------------------------

def test_pins_of_the_convention():
    assert M.rand_bytes(M.CCSDS_RAND, 8).tolist() == [0xFF, 0x48, 0x0E, 0xC0, 0x9A, 0x0D, 0x70, 0xBC]
    assert M.rand_period(M.CCSDS_RAND) == 255
    assert np.array([M.CCSDS_MARKER], dtype="<u4").tobytes() == bytes([0x1A, 0xCF, 0xFC, 0x1D])
    fs = bbb.FrameSync.ccsds(4)
    assert (fs.marker, fs.marker_bits, fs.frame_bits, fs.randomizer, fs.payload_bytes) == (0x1DFCCF1A, 32, 32 + 8 * 1020, (0x1A9, 0xFF), 1020)
    # one known frame through bbb_frame_attach_host: an 8-bit marker 0xB1 and the payload 00 FF 12 under the CCSDS randomiser
    c = M.Cfg(0xB1, 8, 32, rand=M.CCSDS_RAND)
    out = np.zeros(1, dtype=np.uint64)
    pay = np.array([0x00, 0xFF, 0x12], dtype=np.uint8)
    assert _lib.lib().bbb_frame_attach_host(C.c_void_p(pay.ctypes.data), 1, C.byref(cfg_of(c)), C.c_void_p(out.ctypes.data)) == 0
    assert out.tobytes() == bytes([0xB1, 0x00 ^ 0xFF, 0xFF ^ 0x48, 0x12 ^ 0x0E, 0, 0, 0, 0])
    assert np.array_equal(M.pack(M.attach(c, pay)), out)
    # without a randomiser, at a marker that is no whole number of bytes: 13 bits 0x1ACF, then the payload byte 0x81 from bit 13 on
    c = M.Cfg(0x1ACF, 13, 21)
    pay = np.array([0x81], dtype=np.uint8)
    assert _lib.lib().bbb_frame_attach_host(C.c_void_p(pay.ctypes.data), 1, C.byref(cfg_of(c)), C.c_void_p(out.ctypes.data)) == 0
    assert int(out[0]) == 0x1ACF | 0x81 << 13


# ---- the model against the literal rules -------------------------------------------------------------------------------------------

LITERAL = ((0, 0, (0, 0)), (1, 0, (0, 2)), (1, 2, (1, 2)), (3, 1, (0, 1)))


def _literal(c, bits):
    """(pos, meta, counters, mode, pol, misses, position) as `brute` says."""
    frames, counters, (mode, pol, misses, pos) = M.brute(c, bits.tolist())
    return [f[0] for f in frames], [f[1] | f[2] << 8 | f[3] << 9 | f[4] << 10 for f in frames], counters, mode, pol, misses, pos


@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("v,w,tol", LITERAL)
def test_model_equals_the_literal_rules_on_every_stream_of_20_bits(v, w, tol, part):
    """EVERY stream of 20 bits at M = 8, F = 16, a quarter of the 2^20 a case: frames, counters and state of `run` are those of
    the literal transcription of the two rules.  The transcription walks a quarter's streams side by side (`brute_all`: a bit
    position or a frame a round, every distance bit by bit); every 53rd of them it is itself held to the one-stream `brute`."""
    c = M.Cfg(0xB1, 8, 16, tol[0], tol[1], v, w)
    first = part << 18
    B = ((np.arange(first, first + (1 << 18), dtype=np.int64)[:, None] >> np.arange(20)) & 1).astype(np.uint8)
    fpos, fmeta, nf, cnt, mode, pol, misses, pos = M.brute_all(c, B)
    for r in range(0, len(B), 53):
        lp, lm, lc, lmode, lpol, lmisses, lposn = _literal(c, B[r])
        assert (fpos[r, :nf[r]].tolist(), fmeta[r, :nf[r]].tolist(), mode[r], misses[r], pos[r]) == (lp, lm, lmode, lmisses, lposn), B[r]
        assert {k: cnt[k][r] for k in M.COUNTERS} == lc and (lmode == M.SEARCH or pol[r] == lpol), B[r]
    want = zip(fpos.tolist(), fmeta.tolist(), nf.tolist(), mode.tolist(), pol.tolist(), misses.tolist(), pos.tolist(),
               *[cnt[k].tolist() for k in M.COUNTERS])
    for bits, (wp, wm, n, wmode, wpol, wmisses, wposn, *wc) in zip(B, want):
        gpos, gmeta, st = M.run(c, bits)
        assert gpos == wp[:n] and gmeta == wm[:n], bits
        assert [st[k] for k in M.COUNTERS] == wc and (st["mode"], st["misses"], st["pos"]) == (wmode, wmisses, wposn), bits
        assert wmode == M.SEARCH or st["pol"] == wpol, bits
    # without confirmations the quarter's streams end in both modes, with frames; with them 20 bits hold no confirmed chain
    # (p + 16 + 8 > 20) and every candidate is rejected: the chains are the next test's
    assert (set(mode.tolist()) == {M.SEARCH, M.LOCK} and nf.any()) if v == 0 else (cnt["rejected"].any() and not nf.any())


@pytest.mark.parametrize("v,w,tol", LITERAL)
def test_model_equals_the_literal_rules_on_damaged_frames(v, w, tol):
    """What 20 bits have no room for, `run` against the one-stream `brute`: a run of v + 2 frames and half a frame with every one
    bit flipped, and a run of v + 4 frames with every subset of the markers damaged beyond tol_lock, all in both polarities.
    These reach confirmed chains, flywheeled frames and losses under every setting."""
    c = M.Cfg(0xB1, 8, 16, tol[0], tol[1], v, w)
    frame = np.concatenate([c.mbits, np.zeros(8, dtype=np.uint8)])
    streams = []
    base = np.concatenate([frame] * (v + 3))[:16 * (v + 2) + 8]
    for i in range(len(base)):
        streams.append(base.copy())
        streams[-1][i] ^= 1
    for subset in range(1 << (v + 4)):
        bits = np.concatenate([frame] * (v + 4))
        for f in range(v + 4):
            if subset >> f & 1:
                bits[16 * f:16 * f + tol[1] + 1] ^= 1
        streams.append(bits)
    seen = set()
    for bits in [x ^ q for x in streams for q in (0, 1)]:
        lp, lm, lc, lmode, lpol, lmisses, lposn = _literal(c, bits)
        gpos, gmeta, st = M.run(c, bits)
        assert (gpos, gmeta) == (lp, lm), bits
        assert {k: st[k] for k in M.COUNTERS} == lc and (st["mode"], st["misses"], st["pos"]) == (lmode, lmisses, lposn), bits
        assert lmode == M.SEARCH or st["pol"] == lpol
        seen.add((lc["acquisitions"] > 0, lc["flywheeled"] > 0, lc["losses"] > 0, lc["rejected"] > 0))
    assert any(s[0] for s in seen) and any(s[2] for s in seen) and (w == 0 or any(s[1] for s in seen)) and (v == 0 or any(s[3] for s in seen)), seen


# ---- the host entry points against the model ----------------------------------------------------------------------------------------

def test_host_entry_points_equal_the_model_on_the_grid():
    lib = _lib.lib()
    kinds, losses, rejected, fly, inverted = set(), 0, 0, 0, 0
    for i, case in enumerate(M.grid_cases()):
        c, bits = case["cfg"], case["bits"]
        pos, meta, st = host_run(c, bits)
        assert (pos, meta, st) == (case["pos"], case["meta"], case["words"]), (i, case["kind"], c.M, c.F, c.v, c.w, st, case["words"])
        kinds.add(case["kind"])
        losses, rejected, fly = losses + st[5], rejected + st[6], fly + st[3]
        inverted += any(m >> 8 & 1 for m in meta)
        if (c.F - c.M) % 8 or not pos:
            continue
        # extract of what was found, and attach of what extract gave at the found polarity: the frames' own bits again
        words = M.pack(bits)
        pay = np.full(len(pos) * c.payload_bytes + 16, 0xA5, dtype=np.uint8)
        p, m, s = np.array(pos, dtype=np.uint64), np.array(meta, dtype=np.uint16), np.array(st, dtype=np.uint64)
        assert lib.bbb_frame_extract_host(C.c_void_p(words.ctypes.data), len(bits), 0, C.c_void_p(p.ctypes.data), C.c_void_p(m.ctypes.data),
                                          C.c_void_p(s.ctypes.data), len(pos), C.byref(cfg_of(c)), C.c_void_p(pay[8:].ctypes.data)) == 0
        want = M.extract(c, bits, pos, meta)
        assert np.array_equal(pay[8:-8], want) and (pay[:8] == 0xA5).all() and (pay[-8:] == 0xA5).all(), (i, case["kind"])
        back = np.full((len(pos) * c.F + 63) // 64 + 2, GUARD, dtype=np.uint64)
        assert lib.bbb_frame_attach_host(C.c_void_p(want.ctypes.data), len(pos), C.byref(cfg_of(c)), C.c_void_p(back[1:].ctypes.data)) == 0
        assert back[0] == back[-1] == GUARD and np.array_equal(back[1:-1], M.pack(M.attach(c, want)))
        clean = [j for j, mm in enumerate(meta) if mm & 0x3FF == 0]             # a clean marker in true polarity: bit for bit
        got = np.unpackbits(back[1:-1].view(np.uint8), bitorder="little")
        for j in clean[:3]:
            assert np.array_equal(got[j * c.F:(j + 1) * c.F], bits[pos[j]:pos[j] + c.F])
    assert kinds >= set(M.stream_kinds()) | {"inverted, one polarity", "all candidates", "all candidates, rejected"}
    assert losses > 50 and rejected > 50 and fly > 50 and inverted > 20


def test_named_cases():
    """What the issue names, each with the outcome written out here, not taken from the model."""
    rng = np.random.default_rng(5)
    c = M.Cfg(0x1DFCCF1A, 32, 200, 2, 6, 1, 2)
    fr = M._frames(c, rng, 8)
    clean = np.concatenate(fr)
    pos, meta, st = host_run(c, clean)
    assert pos == [200 * j for j in range(8)] and meta == [1 << 10] + [0] * 7 and st == [M.LOCK | 8 << 32, 1600, 8, 0, 1, 0, 0, 0]
    junk = rng.integers(0, 2, 77).astype(np.uint8)
    pos, meta, st = host_run(c, np.concatenate([junk, clean ^ 1]))
    assert pos == [77 + 200 * j for j in range(8)] and meta == [1 << 10 | 1 << 8] + [1 << 8] * 7 and st[0] == M.LOCK | 1 << 8 | 8 << 32
    one = M.Cfg(0x1DFCCF1A, 32, 200, 2, 6, 1, 2, both=False)
    pos, meta, st = host_run(one, np.concatenate([junk, clean ^ 1]))
    assert pos == [] and st == [0, 77 + 1600 - 31, 0, 0, 0, 0, 0, 0]
    # exactly tol_search and tol_search + 1 errors in the first marker; exactly w and w + 1 bad markers in a row
    for k, first in ((2, 0), (3, 200)):
        s = clean.copy()
        s[[1, 9, 30][:k]] ^= 1
        pos, meta, st = host_run(c, s)
        assert pos[0] == first and meta[0] == (k if k == 2 else 0) | 1 << 10 and st[7] == (2 if k == 2 else 0)
    for nbad, want_losses in ((2, 0), (3, 1)):
        s = clean.copy()
        for j in range(2, 2 + nbad):
            s[200 * j:200 * j + 7] ^= 1
        pos, meta, st = host_run(c, s)
        if not want_losses:
            assert pos == [200 * j for j in range(8)] and [m >> 9 & 1 for m in meta] == [0, 0, 1, 1, 0, 0, 0, 0] and st[2:6] == [8, 2, 1, 0]
        else:                                       # frames 2 and 3 flywheeled, lost at 4, found again at 5 (confirmed by 6)
            assert pos == [0, 200, 400, 600, 1000, 1200, 1400] and st[2:6] == [7, 2, 2, 1] and meta[4] == 1 << 10
    # records that end inside a marker, inside a frame, at a frame's end; max_frames smaller than the count
    for cut, nf, mode_pos in ((1600 + 16, 8, 1600), (1600 + 100, 8, 1600), (1600, 8, 1600), (1599, 7, 1400)):
        pos, meta, st = host_run(c, np.concatenate([clean, fr[0]])[:cut])
        assert len(pos) == nf and st[1] == mode_pos and st[0] & 0xFF == M.LOCK
    pos, meta, st = host_run(c, clean, max_frames=3)
    assert pos == [0, 200, 400] and st[0] == M.LOCK | M.OVERFLOW | 8 << 32 and st[2] == 8
    # the data behind the state's position: the flag and nothing else
    pos, meta, st = host_run(c, clean, first_bit=64, state=[M.LOCK, 63, 5, 4, 3, 2, 1, 0])
    assert pos == [] and st == [M.LOCK | M.ERROR, 63, 5, 4, 3, 2, 1, 0]
    # an all-zero stream under an all-zero marker: position 0 is confirmed at once
    z = M.Cfg(0, 16, 40, 0, 2, 3, 1)
    pos, meta, st = host_run(z, np.zeros(1000, dtype=np.uint8))
    assert pos == list(range(0, 1000, 40)) and st[2:] == [25, 0, 1, 0, 0, 0]


def _cut_run(c, bits, cuts, hold):
    """The record in pieces at `cuts` (word multiples), each call's data the last `hold` bits before the cut's start and on."""
    st, pos, meta, lo = [0] * 8, [], [], 0
    edges = [0] + cuts + [len(bits)]
    for a, b in zip(edges[:-1], edges[1:]):
        lo = max(0, a - hold)
        p, m, st = host_run(c, bits[lo:b], first_bit=lo, final=b == len(bits) and (a, b) == tuple(edges[-2:]), state=st)
        pos, meta = pos + p, meta + m
    return pos, meta, st


def test_cutting_gives_one_call():
    rng = np.random.default_rng(77)
    lib = _lib.lib()
    cases = M.grid_cases()
    for i in list(range(0, len(cases), 7)) + [len(cases) - 1, len(cases) - 2]:
        c, bits = cases[i]["cfg"], cases[i]["bits"]
        plan = _lib.FrameSyncPlan()
        assert lib.bbb_framesync_plan(len(bits), C.byref(cfg_of(c)), C.byref(plan)) == 0
        hold = plan.holdback_bits
        assert hold % 64 == 0 and 0 <= hold - (max(c.v, 1) * c.F + c.M) < 64 and plan.tile_bits % 64 == 0
        nw = len(bits) // 64
        for cuts in ([], sorted(set((64 * rng.integers(0, nw + 1, 5)).tolist())), [64 * k for k in range(1, min(nw, 12))]):
            cuts = [int(x) for x in cuts]
            pos, meta, st = _cut_run(c, bits, cuts, hold)
            want = cases[i]["words"]
            # the last call's own count is not the record's: the other words are
            assert (pos, meta) == (cases[i]["pos"], cases[i]["meta"]), (i, cuts)
            assert st[1:] == want[1:] and st[0] & 0xFFFFFFFF == want[0] & 0xFFFFFFFF, (i, cuts, st, want)
            # ... and the model cuts the same way
            ms, mp = M.new_state(), []
            edges = [0] + cuts + [len(bits)]
            for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
                lo = max(0, a - hold)
                p, _, ms = M.run(c, bits[lo:b], lo, k == len(edges) - 2, ms)
                mp += p
            assert mp == pos and M.words(ms)[1:] == want[1:]


# ---- the argument checks ------------------------------------------------------------------------------------------------------------

def test_invalid_arguments_return_before_the_device_is_touched():
    """Every pointer here is a number no device ever gave out: a call that got as far as the device would fail otherwise
    (BBB_ENODEV on a machine without a GPU), and the last cases show that a valid call does get that far."""
    import torch
    lib = _lib.lib()
    IN, STATE, POS, META, SCR, OUT = 1 << 20, 1 << 24, 1 << 26, 1 << 28, 1 << 30, 1 << 32
    NB, MF = 100_000, 20                            # 1563 words of input; CCSDS depth 4: frames of 8192 bits, 1020 payload bytes

    def changed(**kw):
        k = cfg_of(M.ccsds(4, tol_search=2, tol_lock=6))
        for n, v in kw.items():
            if n == "reserved":
                k.reserved[2] = v
            else:
                setattr(k, n, v)
        return k

    def ref(k):
        return C.byref(k) if k is not None else None

    def run(k, in_=IN, nbits=NB, first=0, state=STATE, pos=POS, meta=META, mf=MF, scr=SCR):
        return lib.bbb_framesync_run(C.c_void_p(in_), nbits, first, 1, ref(k), C.c_void_p(state), C.c_void_p(pos), C.c_void_p(meta), mf,
                                     C.c_void_p(scr), 0, None)

    def ext(k, in_=IN, nbits=NB, first=0, pos=POS, meta=META, state=STATE, mf=MF, out=OUT):
        return lib.bbb_frame_extract(C.c_void_p(in_), nbits, first, C.c_void_p(pos), C.c_void_p(meta), C.c_void_p(state), mf, ref(k),
                                     C.c_void_p(out), 0, None)

    def att(k, pay=IN, nf=MF, out=OUT):
        return lib.bbb_frame_attach(C.c_void_p(pay), nf, ref(k), C.c_void_p(out), 0, None)

    def plan(k):
        return lib.bbb_framesync_plan(NB, ref(k), C.byref(_lib.FrameSyncPlan()))

    def model(k):
        return lib.bbb_framesync_model_host(None, 0, 0, 1, ref(k), C.c_void_p(STATE), None, None, 0)

    good = changed()
    bad_cfg = [(None, "null"), (changed(marker_bits=7, marker=1), "marker_bits must"), (changed(marker_bits=65), "marker_bits must"),
               (changed(marker=1 << 32), "bits above"), (changed(frame_bits=39), "frame_bits must"), (changed(frame_bits=(1 << 20) + 1), "frame_bits must"),
               (changed(tol_lock=9), "tol_lock must"), (changed(tol_search=7), "tol_search must"), (changed(verify=8), "verify must"),
               (changed(flywheel=8), "flywheel must"), (changed(both_polarities=2), "both_polarities must"),
               (changed(rand_poly=0x0A9), "rand_poly must"), (changed(rand_poly=0x1A8), "rand_poly must"), (changed(rand_poly=0x3A9), "rand_poly must"),
               (changed(rand_seed=0), "rand_seed"), (changed(rand_seed=256), "rand_seed"), (changed(reserved=1), "reserved")]
    for k, what in bad_cfg:
        for call in (run, ext, att, plan, model):
            assert call(k) == _lib.BBB_EINVAL, what
            assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    nin = 8 * 1563
    bad = [(run, dict(in_=0), "null in_packed"), (run, dict(state=0), "null state"), (run, dict(pos=0), "null pos"), (run, dict(meta=0), "null meta"),
           (run, dict(scr=0), "null scratch"), (run, dict(in_=IN + 4), "misaligned in_packed"), (run, dict(state=STATE + 4), "misaligned state"),
           (run, dict(pos=POS + 4), "misaligned pos"), (run, dict(meta=META + 1), "misaligned meta"), (run, dict(scr=SCR + 4), "misaligned scratch"),
           (run, dict(state=IN + nin - 8), "state overlaps the input"), (run, dict(pos=IN - 8 * MF + 8), "pos overlaps the input"),
           (run, dict(meta=IN + nin - 2), "meta overlaps the input"), (run, dict(scr=IN + nin - 8), "scratch overlaps the input"),
           (run, dict(pos=STATE + 56), "pos overlaps state"), (run, dict(meta=STATE - 2 * MF + 2), "meta overlaps state"),
           (run, dict(scr=STATE + 56), "scratch overlaps state"), (run, dict(meta=POS + 8 * MF - 2), "meta overlaps pos"),
           (run, dict(scr=POS + 8 * MF - 8), "scratch overlaps pos"), (run, dict(scr=META + 2 * MF - 8), "scratch overlaps meta"),
           (run, dict(nbits=(1 << 35) + 1), "2\\^35"), (run, dict(first=(1 << 48) - NB + 1), "2\\^48"), (run, dict(first=1 << 63), "2\\^48"),
           (run, dict(mf=(1 << 35) + 1), "max_frames"),
           (ext, dict(in_=0), "null in_packed"), (ext, dict(pos=0), "null pos"), (ext, dict(meta=0), "null meta"), (ext, dict(state=0), "null state"),
           (ext, dict(out=0), "null out"), (ext, dict(out=OUT + 4), "misaligned out"), (ext, dict(pos=POS + 2), "misaligned pos"),
           (ext, dict(out=IN + nin - 8), "out overlaps the input"), (ext, dict(out=STATE + 56), "out overlaps state"),
           (ext, dict(out=POS + 8 * MF - 8), "out overlaps pos"), (ext, dict(out=META - 1020 * MF + 8), "out overlaps meta"),
           (ext, dict(first=(1 << 48)), "2\\^48"), (ext, dict(mf=(1 << 40) // 1020 + 1), "2\\^40"),
           (att, dict(pay=0), "null payload"), (att, dict(out=0), "null out_packed"), (att, dict(out=OUT + 4), "misaligned out_packed"),
           (att, dict(out=IN + 1020 * MF - 8), "out_packed overlaps"), (att, dict(out=IN - 1024 * MF + 8), "out_packed overlaps"),
           (att, dict(nf=(1 << 40) // 8192 + 1), "2\\^40")]
    for call, kw, what in bad:
        assert call(good, **kw) == _lib.BBB_EINVAL, (what, kw)
        assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    odd = changed(marker_bits=13, marker=0x1ACF, tol_lock=3, tol_search=2)       # payload of 8179 bits
    for call in (ext, att):
        assert call(odd) == _lib.BBB_EINVAL and b"multiple of 8" in lib.bbb_last_error_detail()
    if not torch.cuda.is_available():
        for k in (good, odd, changed(marker_bits=8, marker=0xFF, frame_bits=16, tol_lock=2, tol_search=2), changed(verify=7, flywheel=7),
                  changed(frame_bits=1 << 20), changed(rand_poly=0), changed(rand_poly=0x101, rand_seed=255), changed(marker_bits=64, tol_lock=16)):
            assert run(k) == _lib.BBB_ENODEV, lib.bbb_last_error_detail()
        assert ext(good) == _lib.BBB_ENODEV and att(good) == _lib.BBB_ENODEV
        assert run(good, state=IN + nin, pos=IN - 8 * MF, meta=STATE + 64, scr=POS + 8 * MF) == _lib.BBB_ENODEV
        assert run(good, first=(1 << 48) - NB) == _lib.BBB_ENODEV and run(good, pos=0, meta=0, mf=0) == _lib.BBB_ENODEV
        assert ext(good, out=IN + nin) == _lib.BBB_ENODEV and att(good, out=IN + 1020 * MF) == _lib.BBB_ENODEV


def test_python_argument_checks():
    with pytest.raises(ValueError, match="marker_bits must"):
        bbb.FrameSync(1, 7, 100)
    with pytest.raises(ValueError, match="bits above"):
        bbb.FrameSync(0x100, 8, 100)
    with pytest.raises(ValueError, match="frame_bits must"):
        bbb.FrameSync(1, 32, 39)
    with pytest.raises(ValueError, match="tol_lock must"):
        bbb.FrameSync(1, 32, 100, 0, 9)
    with pytest.raises(ValueError, match="tol_search must"):
        bbb.FrameSync(1, 32, 100, 3, 2)
    with pytest.raises(ValueError, match="verify must"):
        bbb.FrameSync(1, 32, 100, verify=8)
    with pytest.raises(ValueError, match="flywheel must"):
        bbb.FrameSync(1, 32, 100, flywheel=8)
    with pytest.raises(ValueError, match="out of range"):
        bbb.FrameSync(-1, 32, 100)
    with pytest.raises(ValueError, match="randomizer must"):
        bbb.FrameSync(1, 32, 100, randomizer=(0, 1))
    with pytest.raises(ValueError, match="rand_poly must"):
        bbb.FrameSync(1, 32, 100, randomizer=(0xA9, 1))
    with pytest.raises(ValueError, match="CCSDS"):
        bbb.FrameSync.ccsds(4, 200)
    fs = bbb.FrameSync(0x1ACF, 13, 100)
    assert fs.tol_lock == 0 and fs.verify == 1 and fs.flywheel == 2 and fs.both_polarities
    with pytest.raises(ValueError, match="multiple of 8"):
        fs.payload_bytes
    fs = bbb.FrameSync.ccsds(4, tol_search=2, tol_lock=6)
    k = fs._cfg()
    assert (k.marker, k.marker_bits, k.frame_bits, k.tol_search, k.tol_lock, k.verify, k.flywheel, k.both_polarities, k.rand_poly, k.rand_seed,
            list(k.reserved)) == (0x1DFCCF1A, 32, 8192, 2, 6, 1, 2, 1, 0x1A9, 0xFF, [0, 0, 0])
    scratch, hold, tile = fs.plan(100_000)
    assert hold == 8256 and tile % 64 == 0 and scratch >= 100_000 // 8
    assert fs.stats() == dict.fromkeys(M.COUNTERS, 0)
    with pytest.raises(ValueError, match="CUDA tensor"):
        fs.attach(np.zeros(1020, dtype=np.uint8))
    with pytest.raises(ValueError, match="CUDA tensor"):
        fs.find(np.zeros(10, dtype=np.int64), 640)
    rs, cc = bbb.ReedSolomon.ccsds(4), bbb.ConvCode(7, (0o171, 0o133))
    assert bbb.Concatenated(rs, cc).sync is None and bbb.Concatenated(rs, cc, sync=fs).sync is fs
    with pytest.raises(ValueError, match="sync must"):
        bbb.Concatenated(rs, cc, sync=rs)
    with pytest.raises(ValueError, match="one coded frame"):
        bbb.Concatenated(rs, cc, sync=bbb.FrameSync.ccsds(2))


# ---- the kernels' core on the CPU, under the sanitizers ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("framesync_host")
    exe = d / "framesync_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", str(ROOT / "tests" / "framesync_host.cpp"), "-o", str(exe)])
    return exe


def _mf(i, case):
    """max_frames of case i in the walk: room for one more, or (every fifth) for one less than there are."""
    return max(0, len(case["pos"]) + 1 - 2 * (i % 5 == 0))


def _blob(c, bits, first_bit, off, max_frames):
    words = M.pack(bits)
    rand = c.rand or (0, 0)
    head = np.array([c.marker, c.M, c.F, c.tol_search, c.tol_lock, c.v, c.w, int(c.both), rand[0], rand[1], len(bits), first_bit, off, max_frames,
                     len(words)], dtype=np.uint64)
    return head.tobytes() + words.tobytes()


def test_lane_core_on_the_cpu_equals_the_model(host_exe, tmp_path):
    """tests/framesync_host.cpp walks the search pass, the chain pass, extract and attach lane by lane around
    framesync_common.hpp, with the input at byte offsets 0 and 8 between guard words and every buffer of exactly its size on
    the heap, under ASan and UBSan: records, state words, payloads and re-attached frames are the model's."""
    cases = M.grid_cases()
    firsts = (0, 1, 63, 1 << 40)
    blobs = [_blob(c["cfg"], c["bits"], firsts[i % 4], 8 * (i // 4 % 2), _mf(i, c)) for i, c in enumerate(cases)]
    (tmp_path / "c.bin").write_bytes(b"".join(blobs))
    r = subprocess.run([str(host_exe), str(tmp_path / "c.bin"), str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and f"cases {len(blobs)}" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    lines = (tmp_path / "o.txt").read_text().split("\n")
    for i, c in enumerate(cases):
        first, mf = firsts[i % 4], _mf(i, c)
        cfg = c["cfg"]
        want = list(c["words"])
        want[1] += first
        if len(c["pos"]) > mf:
            want[0] |= M.OVERFLOW
        assert [int(t) for t in lines[5 * i].split()] == want, (i, c["kind"], lines[5 * i], want)
        n = min(len(c["pos"]), mf)
        assert [int(t) for t in lines[5 * i + 1].split()] == [p + first for p in c["pos"][:n]], i
        assert [int(t) for t in lines[5 * i + 2].split()] == c["meta"][:n], i
        if (cfg.F - cfg.M) % 8 == 0:
            pay = M.extract(cfg, c["bits"], c["pos"][:n], c["meta"][:n])
            assert bytes.fromhex(lines[5 * i + 3]) == pay.tobytes(), i
            assert bytes.fromhex(lines[5 * i + 4]) == M.pack(M.attach(cfg, pay)).tobytes(), i


# ---- the closed loop on the CPU models -----------------------------------------------------------------------------------------------

def test_closed_loop_counts():
    got = M.sync_loop_counts()
    print(got)
    assert got["inverted"] == 1                                                   # the polarity is found as inverted
    assert got["pos"] == [M.SYNC_LOOP["junk"] + 8192 * j for j in range(16)]        # all 16 frames at their positions
    assert got["data_bits"] == 0 and got["failed"] == 0                           # no data bit wrong behind the Reed-Solomon decoder
    assert got["blind_failed"] == got["blind_codewords"] == 64                    # without sync every codeword fails
    got.pop("pos")
    assert got == M.SYNC_LOOP_COUNTS


# ---- past one pass of the grids ----------------------------------------------------------------------------------------------------
# The search pass takes tiles of 16384 bits, extract and attach a word a lane, each at most 16 workgroups of 256 lanes per
# compute unit at a time (tests/grid.py).  Extract writes the payload alone, (F - M) / F of the stream, so two passes of the
# search tiles can never be two passes of extract: the stream is three passes and five tiles long, which takes search and
# attach through a fourth turn and extract through a third.  tests/test_gpu_framesync.py runs it on the GPU.  The expected
# records are bbb_framesync_model_host's, held to the model here on three stretches, each entered in LOCK at a record of the
# host model's whose predecessor was no miss; the expected bytes are the payloads that were attached, which
# bbb_frame_extract_host is held to here as well.
MULTIPASS_CFG = M.Cfg(M.CCSDS_MARKER, 32, 200, 1, 4, 2, 1, rand=M.CCSDS_RAND)
MULTIPASS_JUNK, MULTIPASS_TILE = 1237, 16384
MULTIPASS_GAPS = ((-1, 2), (60, 63), (1, 3))         # pass 2 (from the tile before it on), pass 3 and the ragged pass 4


def multipass_stream(ncus):
    """(packed words, nbits, payload bytes, framed words, nframes, which frames are inverted): frames of 200 bits from
    bbb_frame_attach_host behind 1237 junk bits, a ragged tail of 77 bits behind the last tile and part of a frame at the end.  Every seventh marker has one wrong bit;
    every 1000th frame's marker is missed (flywheeled); every 3000th and its successor are missed: the lock is lost and found
    again two frames on; the frames of forty tiles from the middle of pass 3's second tile on are inverted; and in every later
    pass of the search every marker of some whole tiles is missed (MULTIPASS_GAPS, in tiles from the pass's first), so that
    the chain searches through tiles that the search pass wrote on a workgroup's second, third and fourth turn."""
    c, J, T = MULTIPASS_CFG, MULTIPASS_JUNK, MULTIPASS_TILE
    G = grid.FRAMESYNC * ncus
    nbits = T * grid.passes(grid.FRAMESYNC, k=3, ncus=ncus) + 77
    nframes = (nbits - J - 150) // c.F
    rng = np.random.default_rng(97)
    pay = rng.integers(0, 256, nframes * c.payload_bytes, dtype=np.uint8)
    framed = np.zeros((nframes * c.F + 63) // 64, dtype=np.uint64)
    assert _lib.lib().bbb_frame_attach_host(C.c_void_p(pay.ctypes.data), nframes, C.byref(cfg_of(c)), C.c_void_p(framed.ctypes.data)) == 0
    bits = np.empty(nbits, dtype=np.uint8)
    bits[:J] = rng.integers(0, 2, J, dtype=np.uint8)
    bits[J:J + nframes * c.F] = np.unpackbits(framed.view(np.uint8), bitorder="little")[:nframes * c.F]
    bits[J + nframes * c.F:] = rng.integers(0, 2, nbits - J - nframes * c.F, dtype=np.uint8)
    fr = np.arange(nframes, dtype=np.int64)
    bits[J + c.F * fr[3::7] + 5] ^= 1
    gaps = [np.arange(-(-((p * G + lo) * T - J) // c.F), ((p * G + hi) * T - J) // c.F) for p, (lo, hi) in enumerate(MULTIPASS_GAPS, 1)]
    missed = np.unique(np.concatenate([fr[500::1000], fr[1700::3000], fr[1701::3000]] + gaps))
    for b in (0, 6, 11, 17, 23, 30):
        bits[J + c.F * missed + b] ^= 1
    i0, i1 = ((2 * G + 1) * T + T // 2 - J) // c.F, ((2 * G + 41) * T - J) // c.F
    bits[J + c.F * i0:J + c.F * i1] ^= 1
    return M.pack(bits), nbits, pay, framed, nframes, (fr >= i0) & (fr < i1)


def multipass_expected(ncus):
    """(words, nbits, payload, framed words, nframes, inverted, pos, meta, state words) with the records of
    bbb_framesync_model_host, held to the model on the tiles around the start of pass 2 (a gap of missed markers among them),
    on tiles inside pass 3 (where the inverted stretch begins) and on the ragged pass 4."""
    c, T = MULTIPASS_CFG, MULTIPASS_TILE
    words, nbits, pay, framed, nframes, inv = multipass_stream(ncus)
    mf = nbits // c.F + 2
    st = np.zeros(8, dtype=np.uint64)
    pos, meta = np.zeros(mf, dtype=np.uint64), np.zeros(mf, dtype=np.uint16)
    rc = _lib.lib().bbb_framesync_model_host(C.c_void_p(words.ctypes.data), nbits, 0, 1, C.byref(cfg_of(c)), C.c_void_p(st.ctypes.data),
                                             C.c_void_p(pos.ctypes.data), C.c_void_p(meta.ctypes.data), mf)
    assert rc == 0, _lib.lib().bbb_last_error_detail()
    n = int(st[0]) >> 32
    pos, meta, st = pos[:n].astype(np.int64), meta[:n], st.tolist()
    G = grid.FRAMESYNC * ncus
    for lo, hi in (((G - 3) * T, (G + 4) * T), ((2 * G + 1) * T, (2 * G + 3) * T), (3 * G * T, None)):
        k = int(np.searchsorted(pos, lo))
        while meta[k - 1] >> 9 & 1 or meta[k] >> 10 & 1:              # entered in LOCK with no miss carried
            k += 1
        a, b = int(pos[k]), nbits if hi is None else hi
        s = M.new_state(a)
        s.update(mode=M.LOCK, pol=int(meta[k]) >> 8 & 1)
        piece = _bits_of(words, a, b)
        gpos, gmeta, s = M.run(c, piece, a, hi is None, s)
        assert len(gpos) >= (b - a - 3 * T) // c.F - 8 and gpos == pos[k:k + len(gpos)].tolist() and gmeta == meta[k:k + len(gpos)].tolist(), (lo, k)
        if hi is None:
            assert k + len(gpos) == n and M.words(s)[1] == st[1] and M.words(s)[0] & 0xFFFFFFFF == st[0] & 0xFFFFFFFF
        else:
            assert s["losses"] >= 1 and s["acquisitions"] >= 1, "the stretch holds no loss of lock"
    return words, nbits, pay, framed, nframes, inv, pos, meta, st


def multipass_payloads(pay, inv, pos, meta):
    """What extract returns for the records: every one is a frame that was attached, so its payload, complemented where the
    record's polarity is not the frame's (a frame flywheeled over where the inverted stretch begins or ends)."""
    c = MULTIPASS_CFG
    idx, rem = np.divmod(pos - MULTIPASS_JUNK, c.F)
    assert not rem.any() and idx[-1] == len(inv) - 1
    wrong_pol = ((meta >> 8 & 1) != inv[idx]).astype(np.uint8)
    assert 0 < int(wrong_pol.sum()) <= 2
    return (pay.reshape(len(inv), c.payload_bytes)[idx] ^ (0xFF * wrong_pol)[:, None]).reshape(-1)


def _bits_of(words, a, b):
    """The bits [a, b) of packed words."""
    w0, w1 = a // 64, (b + 63) // 64
    return np.unpackbits(words[w0:w1].view(np.uint8), bitorder="little")[a - 64 * w0:b - 64 * w0]


def test_multipass_host_model_equals_the_model_on_stretches():
    c = MULTIPASS_CFG
    words, nbits, pay, framed, nframes, inv, pos, meta, st = multipass_expected(256)
    lanes = grid.FRAMESYNC * 256 * 256                                   # a pass of extract or attach, a word a lane
    assert nbits > 3 * lanes * 64 and len(framed) > 2 * lanes and len(pos) * c.payload_bytes // 8 + 1 > 2 * lanes
    # what the machine made of it: the junk passed over, both polarities, losses every 3000 frames, all but the lost frames found
    assert pos[0] == MULTIPASS_JUNK and st[5] >= nframes // 3000 + 3 and st[4] == st[5] + 1 and st[3] >= nframes // 1000
    want = multipass_payloads(pay, inv, pos, meta)
    out = np.full(len(want) + 8, 0xA5, dtype=np.uint8)
    state = np.array(st, dtype=np.uint64)
    p, m = pos.astype(np.uint64), np.ascontiguousarray(meta)
    assert _lib.lib().bbb_frame_extract_host(C.c_void_p(words.ctypes.data), nbits, 0, C.c_void_p(p.ctypes.data), C.c_void_p(m.ctypes.data),
                                             C.c_void_p(state.ctypes.data), len(pos), C.byref(cfg_of(c)), C.c_void_p(out.ctypes.data)) == 0
    assert np.array_equal(out[:len(want)], want) and (out[len(want):] == 0xA5).all()
    assert 0 < int((meta >> 8 & 1).sum()) < len(meta) and nframes - 2 * st[5] - 8 * MULTIPASS_TILE // c.F - 4 <= len(pos) <= nframes
    assert st[0] & 0xFF == M.LOCK and nframes // 7 - st[3] - 2 * st[5] <= st[7] <= nframes // 7 + 1    # (a missed marker's wrong bits are not counted)
