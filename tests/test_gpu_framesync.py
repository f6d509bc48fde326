"""bbb_framesync_run, bbb_frame_extract and bbb_frame_attach on the GPU, bit for bit against tests/framesync_model.py: the grid
of tests/test_framesync_host.py through the C ABI (records, the count, all state words) at first_bit 0, 1, 63 and 2^40, every
buffer between guard words and the scratch of exactly the plan's size, stream lengths around the search pass's tile, a wave's and
a lane's share, markers that straddle a word, a wave's share and a tile at every offset, frames on tile boundaries, two calls
that add to one state, the error flag, max_frames overflow, the adversarial streams, extract and attach against their host forms
at every bit offset, a stream of more than two passes of every kernel's grid, and the Python classes: FrameSync, FrameSyncStream cut at random word multiples, and Concatenated(sync=)
through RX.count_errors on the closed loop of tests/test_framesync_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import grid
import framesync_model as M
import test_framesync_host as H

pytestmark = pytest.mark.gpu

GUARD = -0x5A5A5A5A5A5A5A5B                          # 0xA5A5A5A5A5A5A5A5 as int64
FIRSTS = (0, 1, 63, 1 << 40)
G171 = (0o171, 0o133)


def cfg_of(c):
    from basebandboard_amd import _lib
    k = _lib.FrameSyncCfg()
    k.marker, k.marker_bits, k.frame_bits, k.tol_search, k.tol_lock, k.verify, k.flywheel = c.marker, c.M, c.F, c.tol_search, c.tol_lock, c.v, c.w
    k.both_polarities = int(c.both)
    if c.rand is not None:
        k.rand_poly, k.rand_seed = c.rand
    return k


def _plan(c, nbits):
    from basebandboard_amd import _lib
    p = _lib.FrameSyncPlan()
    assert _lib.lib().bbb_framesync_plan(nbits, C.byref(cfg_of(c)), C.byref(p)) == 0
    return p


class Slab:
    """Device buffers cut out of one int64 tensor of guard words, a guard word between any two: what lies outside them must
    not change."""

    def __init__(self, **words):
        self.at, n = {}, 1
        for name, w in words.items():
            self.at[name] = (n, w)
            n += w + 1
        self.t = torch.full((n,), GUARD, dtype=torch.int64, device="cuda:0")
        self.mask = np.ones(n, dtype=bool)
        for a, w in self.at.values():
            self.mask[a:a + w] = False

    def put(self, name, arr):
        a, w = self.at[name]
        self.t[a:a + len(arr)] = torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda:0")

    def ptr(self, name):
        return C.c_void_p(self.t.data_ptr() + 8 * self.at[name][0])

    def read(self):
        got = self.t.cpu().numpy()
        assert (got[self.mask] == GUARD).all(), "words outside the buffers were written"
        return {name: got[a:a + w].view(np.uint64) for name, (a, w) in self.at.items()}


def gpu_run(c, bits, first_bit=0, final=True, state=None, max_frames=None, meta_off=0):
    """One bbb_framesync_run through the C ABI: (pos, meta, the eight state words).  The meta words beyond the count and the
    pos words beyond it stay guard words.  meta_off: meta_dev begins that many uint16 behind an 8-byte boundary."""
    from basebandboard_amd import _lib
    mf = len(bits) // c.F + 2 if max_frames is None else max_frames
    words = M.pack(bits)
    plan = _plan(c, len(bits))
    assert plan.scratch_bytes % 8 == 0
    s = Slab(inp=len(words), state=8, pos=mf, meta=(mf + meta_off + 3) // 4, scratch=plan.scratch_bytes // 8)
    s.put("inp", words)
    s.put("state", np.array(state if state is not None else [0, first_bit, 0, 0, 0, 0, 0, 0], dtype=np.uint64))
    rc = _lib.lib().bbb_framesync_run(s.ptr("inp"), len(bits), first_bit, int(final), C.byref(cfg_of(c)), s.ptr("state"), s.ptr("pos"),
                                      C.c_void_p(s.ptr("meta").value + 2 * meta_off), mf, s.ptr("scratch"), 0, C.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    assert rc == 0, _lib.lib().bbb_last_error_detail()
    got = s.read()
    assert np.array_equal(got["inp"], words), "the input was written"
    st = got["state"].tolist()
    n = min(st[0] >> 32, mf) if not st[0] & M.ERROR or state is None else 0
    assert (got["meta"].view(np.uint16)[:meta_off] == 0xA5A5).all(), "meta words in front of meta_dev were written"
    meta = got["meta"].view(np.uint16)[meta_off:]
    assert (got["pos"][n:] == np.uint64(GUARD & (2 ** 64 - 1))).all() and (meta[n:] == 0xA5A5).all(), "records beyond the count were written"
    return got["pos"][:n].tolist(), meta[:n].tolist(), st


def _same(c, bits, first_bit=0, **kw):
    pos, meta, st = gpu_run(c, bits, first_bit, **kw)
    mf = kw.get("max_frames")
    wpos, wmeta, ws = M.run(c, bits, first_bit, max_frames=mf)
    assert (pos, meta, st) == (wpos, wmeta, M.words(ws)), (c.M, c.F, c.v, c.w, len(bits), first_bit, st, M.words(ws))
    return pos, meta, st


def test_run_equals_the_model_on_the_grid(gpu):
    for i, case in enumerate(M.grid_cases()):
        c, first = case["cfg"], FIRSTS[i % 4]
        pos, meta, st = gpu_run(c, case["bits"], first, meta_off=i // 4 % 4)    # meta_dev 0, 2, 4 and 6 bytes off an 8-byte boundary
        want = list(case["words"])
        want[1] += first
        assert pos == [p + first for p in case["pos"]] and meta == case["meta"], (i, case["kind"], c.M, c.F, c.v, c.w)
        assert st == want, (i, case["kind"], c.M, c.F, c.v, c.w, st, want)


def test_lengths_around_the_tile_the_wave_and_the_lane(gpu):
    rng = np.random.default_rng(90)
    c = M.Cfg(0x1DFCCF1A, 32, 200, 1, 4, 2, 1)
    tile = _plan(c, 0).tile_bits
    assert tile % 64 == 0 and tile >= 4096
    stream = np.concatenate([rng.integers(0, 2, 131).astype(np.uint8)] + M._frames(c, rng, 4 * tile // 200 + 4))
    for n in (0, 1, 31, 32, 63, 64, 65, 4095, 4096, 4097, tile - 1, tile, tile + 1, tile + 31, tile + 32, tile + 33, 2 * tile, 3 * tile + 17, 4 * tile):
        pos, meta, st = _same(c, stream[:n])
    assert len(pos) == (4 * tile - 131) // 200       # the last and longest: every frame that ends inside the data


@pytest.mark.parametrize("M_", (32, 64))
def test_markers_that_straddle_every_boundary(gpu, M_):
    """The true chain's first marker begins 1 .. M - 1 bits in front of a word's, a wave's share's and a tile's boundary; the bits
    in front of it are junk in which the model, too, may find false candidates."""
    rng = np.random.default_rng(91 + M_)
    c = M.Cfg(M._marker(rng, M_), M_, 520, 0, 2, 1, 1)
    tile = _plan(c, 0).tile_bits
    frames = np.concatenate(M._frames(c, rng, 4))
    for boundary in (64 * 5, 4096, tile, 2 * tile):
        junk = rng.integers(0, 2, boundary).astype(np.uint8)
        for off in range(1, M_):
            pos, meta, st = _same(c, np.concatenate([junk[:boundary - off], frames]))
            assert pos[-4:] == [boundary - off + 520 * j for j in range(4)]


def test_frames_on_tile_boundaries(gpu):
    rng = np.random.default_rng(92)
    c = M.ccsds(4, tol_search=2, tol_lock=6)
    tile = _plan(c, 0).tile_bits
    assert tile % c.F == 0 or c.F % tile == 0       # every frame, or every other, starts a tile
    bits = np.concatenate(M._frames(c, rng, 9))
    pos, meta, st = _same(c, bits)
    assert pos == [8192 * j for j in range(9)]
    pos, meta, st = _same(c, np.concatenate([bits[:8192 * 4], bits[8192 * 4 + 1:]]))    # a slip of one bit: lost and found again
    assert st[5] == 1 and st[4] == 2


def test_two_calls_add_to_one_state(gpu):
    rng = np.random.default_rng(93)
    c = M.Cfg(0x1ACF, 13, 141, 1, 3, 1, 2)
    bits = np.concatenate([rng.integers(0, 2, 77).astype(np.uint8)] + M._frames(c, rng, 40))
    cut = 64 * 40
    hold = _plan(c, 0).holdback_bits
    ms = M.new_state()
    p1, m1, s1 = gpu_run(c, bits[:cut], 0, final=False)
    w1 = M.run(c, bits[:cut], 0, False, ms)
    assert (p1, m1, s1) == (w1[0], w1[1], M.words(ms))
    lo = cut - hold
    p2, m2, s2 = gpu_run(c, bits[lo:], lo, final=True, state=s1)
    w2 = M.run(c, bits[lo:], lo, True, ms)
    assert (p2, m2, s2) == (w2[0], w2[1], M.words(ms))
    one = M.run(c, bits)
    assert p1 + p2 == one[0] and m1 + m2 == one[1] and s2[1:] == M.words(one[2])[1:] and len(p1) > 5 and len(p2) > 5
    # the data begin behind the state's position: the flag, and nothing else is written (gpu_run checks the records' guard words)
    state = [M.LOCK, lo - 1, 5, 4, 3, 2, 1, 0]
    pos, meta, st = gpu_run(c, bits[lo:], lo, state=state)
    assert pos == [] and st == [M.LOCK | M.ERROR] + state[1:]
    # max_frames smaller than the count; and none at all
    pos, meta, st = _same(c, bits, max_frames=7)
    assert len(pos) == 7 and st[0] & M.OVERFLOW and st[0] >> 32 == 40
    pos, meta, st = _same(c, bits, max_frames=0)
    assert st[2] == 40


def test_adversarial_streams(gpu):
    for v in (0, 1, 3):
        c = M.Cfg(0, 16, 40, 0, 2, v, 1)
        _same(c, np.zeros(70_000, dtype=np.uint8))                                 # every position a candidate, the first confirmed
        z = np.zeros(40_000, dtype=np.uint8)
        z[16::17] = 1                              # a candidate every 17 bits; 40 bits on, inside a frame, there is never one
        pos, meta, st = _same(M.Cfg(0, 16, 40, 0, 0, v, 1), z)
        assert st[6] > 2000 if v else st[5] > 400 # every candidate rejected; without confirmations every lock is lost again
    rng = np.random.default_rng(94)
    c = M.Cfg(0x1DFCCF1A, 32, 72, 0, 2, 1, 1)
    pos, meta, st = _same(c, M.make_stream(c, rng, "lose and regain", nframes=228)[:1 << 16])   # 2^16 bits, a loss every five frames
    assert st[5] > 150 and st[4] > 150


def _extract_gpu(c, words, nbits, first_bit, pos, meta, count, max_frames):
    from basebandboard_amd import _lib
    pb = c.payload_bytes
    s = Slab(inp=len(words), state=8, pos=max(1, len(pos)), meta=(len(pos) + 3) // 4 + 1, out=(max_frames * pb + 7) // 8)
    s.put("inp", words)
    s.put("state", np.array([count << 32, 0, 0, 0, 0, 0, 0, 0], dtype=np.uint64))
    s.put("pos", np.array(pos, dtype=np.uint64))
    mt = np.zeros(((len(pos) + 3) // 4 + 1) * 4, dtype=np.uint16)
    mt[:len(meta)] = meta
    s.put("meta", mt.view(np.uint64))
    rc = _lib.lib().bbb_frame_extract(s.ptr("inp"), nbits, first_bit, s.ptr("pos"), s.ptr("meta"), s.ptr("state"), max_frames, C.byref(cfg_of(c)),
                                      s.ptr("out"), 0, C.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    assert rc == 0, _lib.lib().bbb_last_error_detail()
    got = s.read()
    assert np.array_equal(got["inp"], words)
    return got["out"].view(np.uint8)


def _extract_host(c, words, nbits, first_bit, pos, meta, count, max_frames):
    from basebandboard_amd import _lib
    out = np.full((max_frames * c.payload_bytes + 7) // 8 * 8, 0xA5, dtype=np.uint8)
    p, m, st = np.array(pos + [0], dtype=np.uint64), np.array(meta + [0], dtype=np.uint16), np.array([count << 32] + [0] * 7, dtype=np.uint64)
    assert _lib.lib().bbb_frame_extract_host(C.c_void_p(words.ctypes.data), nbits, first_bit, C.c_void_p(p.ctypes.data), C.c_void_p(m.ctypes.data),
                                             C.c_void_p(st.ctypes.data), max_frames, C.byref(cfg_of(c)), C.c_void_p(out.ctypes.data)) == 0
    return out


@pytest.mark.parametrize("pb", (1, 15, 16, 17, 1020))
def test_extract_and_attach_equal_their_host_forms(gpu, pb):
    """Three frames whose first begins 0 .. 63 bits into the data, in both polarities, with and without the randomiser: the
    device's bytes are the host loop's, and the model's; the bytes behind the count stay as they were.  Attach: the device's words
    are the host loop's, and the model's."""
    from basebandboard_amd import _lib
    rng = np.random.default_rng(95 + pb)
    for rand in (None, M.CCSDS_RAND):
        c = M.Cfg(0x1DFCCF1A, 32, 32 + 8 * pb, rand=rand)
        pay = rng.integers(0, 256, 3 * pb).astype(np.uint8)
        frames = M.attach(c, pay)
        src = torch.from_numpy(pay).to("cuda:0")
        s = Slab(out=(3 * c.F + 63) // 64)
        rc = _lib.lib().bbb_frame_attach(C.c_void_p(src.data_ptr()), 3, C.byref(cfg_of(c)), s.ptr("out"), 0, C.c_void_p(torch.cuda.current_stream(0).cuda_stream))
        assert rc == 0, _lib.lib().bbb_last_error_detail()
        host = np.zeros((3 * c.F + 63) // 64, dtype=np.uint64)
        assert _lib.lib().bbb_frame_attach_host(C.c_void_p(pay.ctypes.data), 3, C.byref(cfg_of(c)), C.c_void_p(host.ctypes.data)) == 0
        got = s.read()["out"]
        assert np.array_equal(got, host) and np.array_equal(got, M.pack(frames))
        for pol in (0, 1):
            for off in range(64):
                bits = np.concatenate([rng.integers(0, 2, off).astype(np.uint8), frames ^ pol, rng.integers(0, 2, 5).astype(np.uint8)])
                first = FIRSTS[off % 4]
                pos, meta = [first + off + c.F * j for j in range(3)], [pol << 8 | (j == 0) << 10 for j in range(3)]
                words = M.pack(bits)
                for count, mf in ((3, 3), (2, 3), (3, 2)):
                    dev = _extract_gpu(c, words, len(bits), first, pos, meta, count, mf)
                    host = _extract_host(c, words, len(bits), first, pos, meta, count, mf)
                    n = min(count, mf) * pb
                    assert np.array_equal(dev[:n], host[:n]) and np.array_equal(dev[:n], pay[:n]), (pb, rand, pol, off, count, mf)
                    assert (dev[n:] == 0xA5).all() and (host[n:] == 0xA5).all()
        # a record that does not lie inside the data gives zeros, on both sides
        bits = np.concatenate([frames, rng.integers(0, 2, 5).astype(np.uint8)])
        pos, meta = [0, c.F, 2 * c.F + 6], [0, 0, 0]
        dev = _extract_gpu(c, M.pack(bits), len(bits), 0, pos, meta, 3, 3)
        host = _extract_host(c, M.pack(bits), len(bits), 0, pos, meta, 3, 3)
        assert np.array_equal(dev[:3 * pb], host[:3 * pb]) and not dev[2 * pb:3 * pb].any() and np.array_equal(dev[:2 * pb], pay[:2 * pb])


def test_more_than_two_passes_of_the_grids(gpu):
    """One stream of three passes and five tiles of the search pass and a ragged tail (tests/test_framesync_host.py builds it and
    holds bbb_framesync_model_host, the expected records here, to the model on three stretches): frames of 200 bits behind junk,
    wrong marker bits, flywheeled frames, a loss of lock every 3000 frames and at the tile where pass 2 begins, forty tiles
    inverted.  Attach on the GPU against the host's words, the search and chain passes against the host model's positions, meta
    and eight state words, extract against the payloads that were attached: search and attach take a fourth turn of their
    loops, extract (the payload is 168 / 200 of the stream) a third."""
    from basebandboard_amd import _lib
    c = H.MULTIPASS_CFG
    words, nbits, pay, framed, nframes, inv, wpos, wmeta, wst = H.multipass_expected(grid.cus())
    lanes = grid.FRAMESYNC * grid.cus() * 256
    assert nbits > 3 * lanes * 64 and len(framed) > 2 * lanes and len(wpos) * c.payload_bytes // 8 + 1 > 2 * lanes
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    src = torch.from_numpy(pay).to("cuda:0")
    s = Slab(out=len(framed))
    rc = _lib.lib().bbb_frame_attach(C.c_void_p(src.data_ptr()), nframes, C.byref(cfg_of(c)), s.ptr("out"), 0, stream)
    assert rc == 0, _lib.lib().bbb_last_error_detail()
    assert np.array_equal(s.read()["out"], framed), "attach differs from bbb_frame_attach_host"
    del s, src
    mf = nbits // c.F + 2
    plan = _plan(c, nbits)
    s = Slab(inp=len(words), state=8, pos=mf, meta=(mf + 3) // 4, scratch=plan.scratch_bytes // 8, out=(mf * c.payload_bytes + 7) // 8)
    s.put("inp", words)
    s.put("state", np.zeros(8, dtype=np.uint64))
    rc = _lib.lib().bbb_framesync_run(s.ptr("inp"), nbits, 0, 1, C.byref(cfg_of(c)), s.ptr("state"), s.ptr("pos"), s.ptr("meta"), mf, s.ptr("scratch"), 0, stream)
    assert rc == 0, _lib.lib().bbb_last_error_detail()
    rc = _lib.lib().bbb_frame_extract(s.ptr("inp"), nbits, 0, s.ptr("pos"), s.ptr("meta"), s.ptr("state"), mf, C.byref(cfg_of(c)), s.ptr("out"), 0, stream)
    assert rc == 0, _lib.lib().bbb_last_error_detail()
    got = s.read()
    n = len(wpos)
    assert got["state"].tolist() == wst, (got["state"].tolist(), wst)
    assert np.array_equal(got["inp"], words), "the input was written"
    assert np.array_equal(got["pos"][:n].astype(np.int64), wpos), int(np.flatnonzero(got["pos"][:n].astype(np.int64) != wpos)[0])
    assert np.array_equal(got["meta"].view(np.uint16)[:n], wmeta), int(np.flatnonzero(got["meta"].view(np.uint16)[:n] != wmeta)[0])
    assert (got["pos"][n:] == np.uint64(GUARD & (2 ** 64 - 1))).all() and (got["meta"].view(np.uint16)[n:] == 0xA5A5).all(), "records beyond the count were written"
    out = got["out"].view(np.uint8)
    want = H.multipass_payloads(pay, inv, wpos, wmeta)
    assert np.array_equal(out[:len(want)], want), int(np.flatnonzero(out[:len(want)] != want)[0])
    assert (out[len(want):] == 0xA5).all(), "bytes beyond the count's payloads were written"


def _dev(bits):
    return torch.from_numpy(M.pack(bits).view(np.int64)).to("cuda:0")


def test_python_classes(gpu):
    rng = np.random.default_rng(96)
    fs = gpu.FrameSync.ccsds(1, tol_search=2, tol_lock=6)
    c = M.ccsds(1, tol_search=2, tol_lock=6)
    pay = rng.integers(0, 256, 30 * 255).astype(np.uint8)
    framed, nb = fs.attach(torch.from_numpy(pay).to("cuda:0"))
    want = M.attach(c, pay)
    assert nb == len(want) and np.array_equal(framed.cpu().numpy().view(np.uint64), M.pack(want))
    bits = np.concatenate([rng.integers(0, 2, 333).astype(np.uint8), want ^ 1, rng.integers(0, 2, 90).astype(np.uint8)])
    wpos, wmeta, ws = M.run(c, bits)
    pos, meta, count = fs.find(_dev(bits), len(bits))
    n = int(count.item())
    assert n == len(wpos) == 30 and pos[:n].cpu().tolist() == wpos and (meta[:n].cpu().numpy().view(np.uint16)).tolist() == wmeta
    out = fs.extract(_dev(bits), len(bits), pos, meta, count)
    assert np.array_equal(out[:n * 255].cpu().numpy(), pay)
    frames, n2 = fs.sync(_dev(bits), len(bits))
    assert n2 == 30 and np.array_equal(frames.cpu().numpy(), pay)
    assert fs.stats() == {k: 2 * ws[k] for k in M.COUNTERS}
    # the stream, cut at random word multiples: the frames, records and state of one call
    for trial in range(3):
        fs2 = gpu.FrameSync.ccsds(1, tol_search=2, tol_lock=6)
        st = fs2.stream()
        words = _dev(bits)
        cuts = sorted(set(rng.integers(0, len(bits) // 64, 6).tolist()))
        got, gpos, edges = [], [], [0] + cuts
        for a, b in zip(edges, edges[1:] + [None]):
            if b is None:
                fr, p, m, cnt = st.finish(words[a:], len(bits) - 64 * a)
            else:
                fr, p, m, cnt = st.push(words[a:b])
            k = int(cnt.item())
            got.append(fr[:k * 255].cpu().numpy())
            gpos += p[:k].cpu().tolist()
        assert gpos == wpos and np.array_equal(np.concatenate(got), pay), (trial, cuts)
        assert st.state.cpu().numpy().view(np.uint64).tolist()[1:] == M.words(ws)[1:]
        assert fs2.stats() == {k: ws[k] for k in M.COUNTERS}


def test_closed_loop_through_rx(gpu):
    """The loop of tests/test_framesync_host.py on the GPU: RX.count_errors(fec=Concatenated(..., sync=...)) over the inverted,
    noisy record with 1237 junk bits in front finds all 16 frames and counts no wrong data bit, with exactly the CPU's counts;
    without `sync` every codeword fails."""
    import rs_model
    c, data, framed, tx, rx, vit = M.sync_loop_record()
    want = M.SYNC_LOOP_COUNTS
    outer, inner = gpu.ReedSolomon.ccsds(4), gpu.ConvCode(7, G171)
    fs = gpu.FrameSync.ccsds(4, tol_search=M.SYNC_LOOP["tol_search"], tol_lock=M.SYNC_LOOP["tol_lock"], verify=M.SYNC_LOOP["verify"],
                             flywheel=M.SYNC_LOOP["flywheel"])
    cat = gpu.Concatenated(outer, inner, sync=fs)
    outer_tx = gpu.ReedSolomon.ccsds(4)
    fs_tx = gpu.FrameSync.ccsds(4)
    coded = outer_tx.encode(torch.from_numpy(data).to("cuda:0"))
    att, na = fs_tx.attach(coded)
    assert na == len(framed) - M.SYNC_LOOP["junk"]
    assert np.array_equal(np.unpackbits(att.cpu().numpy().view(np.uint8), bitorder="little")[:na], framed[M.SYNC_LOOP["junk"]:])
    cat_tx = gpu.Concatenated(outer_tx, inner, sync=fs_tx)
    t, ntx = cat_tx.encode(torch.from_numpy(data).to("cuda:0"))                     # the transmit side closes on itself: no junk, no noise
    back, nback = cat_tx.decode(t, hard=True, nbits=ntx)
    assert ntx == 2 * na and nback // 8 >= 15 * 4 * 223 and np.array_equal(back.cpu().numpy().view(np.uint8)[:15 * 892], data[:15 * 892])
    xt = torch.from_numpy(rx).to("cuda:0")
    r = gpu.RX(rs_model.LOOP["prbs"][0], 1, 0)
    errors, nbits = r.count_errors(xt, fec=cat)
    st, ost = fs.stats(), outer.stats()
    got = dict(frames=st["frames"], flywheeled=st["flywheeled"], acquisitions=st["acquisitions"], losses=st["losses"], rejected=st["rejected"],
               marker_bit_errors=st["marker_bit_errors"], failed=ost["failed"], symbols=ost["symbols_corrected"],
               data_bits=errors)
    print(got)
    assert nbits == 8 * len(data) and got == {k: want[k] for k in got}
    blind = gpu.ReedSolomon.ccsds(4)
    gpu.RX(rs_model.LOOP["prbs"][0], 1, 0).count_errors(xt, fec=gpu.Concatenated(blind, inner))
    assert (blind.stats()["failed"], blind.stats()["codewords"]) == (want["blind_failed"], want["blind_codewords"])


def test_example_sync(gpu):
    """examples/bbb_mc --rs 4 --sync 1237: the closed loop with markers, 1237 random bits in front and the channel inverted,
    through the C ABI alone (its noise is the example's own, so the counts are not the model's): the polarity is found, all 16
    frames, and no data bit is wrong behind the Reed-Solomon decoder."""
    import json
    import pathlib
    import subprocess
    exe = pathlib.Path(__file__).resolve().parent.parent / "examples" / "bbb_mc"
    r = subprocess.run([str(exe), "--rs", "4", "--sync", "1237", "--eye-samples", "114176"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    sync, rs = [json.loads(line) for line in r.stdout.strip().split("\n")[-2:]]
    print(sync, rs)
    assert sync["mode"] == "sync" and (sync["junk_bits"], sync["inverted"], sync["frames_found"], sync["acquisitions"], sync["losses"]) == (1237, 1, 16, 1, 0)
    assert rs["mode"] == "rs" and (rs["frames"], rs["coded_bits"], rs["data_errors"], rs["failed"], rs["codewords"]) == (16, 2 * (1237 + 16 * 8192), 0, 0, 64)
    assert 0 < rs["viterbi_errors"] < rs["channel_errors"]
