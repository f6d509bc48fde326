"""bbb_rs_decode and bbb_rs_encode on the GPU, bit for bit against tests/rs_model.py: the grid of tests/test_rs_host.py (fields,
first roots, root spacings, 2..32 parity symbols, lengths around the lane and tile sizes, depths 1, 3 and 8, every error
pattern), the statistics added to over two calls, frame counts that fill and do not fill a workgroup's four frames, buffers
that start 0, 1, 3 and 15 bytes off alignment between guard bytes, the outputs that may be left out, a record with clean,
corrected and failed codewords in one workgroup, more than two passes of the decoder's grid, the encoder against bbb_rs_encode_host, and the Python classes: ReedSolomon,
RSStream cut at random points, and Concatenated through RX.count_errors on the closed loop of tests/test_rs_host.py.

Out of reach at a test's cost: more than one pass of the encoder's grid, which is capped at 2^16 workgroups of one codeword a
thread (2^24 codewords a pass)."""
import ctypes as C

import numpy as np
import pytest
import torch

import grid
import rs_model as M
import test_rs_host as H

pytestmark = pytest.mark.gpu

GUARD = 0xA5
OFFS = (0, 1, 3, 15)
G171 = (0o171, 0o133)


def _cfg(code):
    from basebandboard_amd import _lib
    c = _lib.RSCfg()
    c.prim_poly, c.fcr, c.prim, c.nroots, c.n, c.depth = code.prim_poly, code.fcr, code.prim, code.nroots, code.n, code.depth
    return c


def _guarded(nbytes, off):
    """A device buffer of GUARD bytes and the address `off` bytes past a 16-byte boundary inside it where nbytes are expected."""
    t = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    assert t.data_ptr() % 16 == 0
    return t, 16 + off


def _payload(t, start, nbytes):
    got = t.cpu().numpy()
    assert (got[:start] == GUARD).all() and (got[start + nbytes:] == GUARD).all(), "bytes outside the output were written"
    return got[start:start + nbytes]


def _decode(gpu, code, recv, nframes, in_off=0, out_off=0, want_nerr=True, stats=None):
    """One bbb_rs_decode through the C ABI.  stats: a device int64[5] that is added to, or None.  Returns (data, nerr), nerr
    empty when it was left out."""
    from basebandboard_amd import _lib
    src, s0 = _guarded(len(recv), in_off)
    src[s0:s0 + len(recv)] = torch.from_numpy(np.ascontiguousarray(recv)).to("cuda:0")
    nd, ne = nframes * code.data_bytes, nframes * code.depth
    data, d0 = _guarded(nd, out_off)
    nerr, e0 = _guarded(ne, (out_off + 1) % 16)
    rc = _lib.lib().bbb_rs_decode(C.c_void_p(src.data_ptr() + s0), nframes, C.byref(_cfg(code)), C.c_void_p(data.data_ptr() + d0),
                                  C.c_void_p(nerr.data_ptr() + e0) if want_nerr else None, C.c_void_p(stats.data_ptr()) if stats is not None else None,
                                  0, C.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    assert rc == 0, _lib.lib().bbb_last_error_detail()
    assert np.array_equal(_payload(src, s0, len(recv)), recv), "the input was written"
    return _payload(data, d0, nd), _payload(nerr, e0, ne if want_nerr else 0)   # (not wanted: none of its bytes may change)


def _encode(gpu, code, data, nframes, in_off=0, out_off=0):
    from basebandboard_amd import _lib
    src, s0 = _guarded(len(data), in_off)
    src[s0:s0 + len(data)] = torch.from_numpy(np.ascontiguousarray(data)).to("cuda:0")
    nc = nframes * code.frame_bytes
    out, o0 = _guarded(nc, out_off)
    rc = _lib.lib().bbb_rs_encode(C.c_void_p(src.data_ptr() + s0), nframes, C.byref(_cfg(code)), C.c_void_p(out.data_ptr() + o0), 0,
                                  C.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    assert rc == 0, _lib.lib().bbb_last_error_detail()
    return _payload(out, o0, nc)


def test_decode_equals_the_model_on_the_grid(gpu):
    for i, c in enumerate(M.grid_cases()):
        code = c["code"]
        stats = torch.tensor([5, 4, 3, 2, 1], dtype=torch.int64, device="cuda:0")
        data, nerr = _decode(gpu, code, c["recv"], c["nframes"], OFFS[i % 4], OFFS[(i // 4) % 4], stats=stats)
        assert np.array_equal(nerr, c["nerr"]), (i, code.n, code.nroots, code.depth, nerr, c["nerr"])
        assert np.array_equal(data, c["out"]), (i, code.n, code.nroots, code.depth)
        # the second call: no nerr, the same statistics added again
        data, nerr = _decode(gpu, code, c["recv"], c["nframes"], OFFS[(i + 1) % 4], OFFS[(i // 4 + 1) % 4], want_nerr=False, stats=stats)
        assert np.array_equal(data, c["out"]) and len(nerr) == 0
        assert stats.cpu().tolist() == [2 * a + b for a, b in zip(c["stats"], (5, 4, 3, 2, 1))], (i, stats.cpu().tolist(), c["stats"])
        # and without statistics
        data, nerr = _decode(gpu, code, c["recv"], c["nframes"], 0, 0)
        assert np.array_equal(data, c["out"]) and np.array_equal(nerr, c["nerr"])


def test_encode_equals_encode_host_on_the_grid(gpu):
    from basebandboard_amd import _lib
    for i, c in enumerate(M.grid_cases()):
        code = c["code"]
        host = np.zeros(len(c["coded"]), dtype=np.uint8)
        src = np.ascontiguousarray(c["data"])
        assert _lib.lib().bbb_rs_encode_host(C.c_void_p(src.ctypes.data), c["nframes"], C.byref(_cfg(code)), C.c_void_p(host.ctypes.data)) == 0
        got = _encode(gpu, code, c["data"], c["nframes"], OFFS[i % 4], OFFS[(i // 4) % 4])
        assert np.array_equal(got, host) and np.array_equal(got, c["coded"]), (i, code.n, code.nroots, code.depth)


@pytest.fixture(scope="module")
def counted():
    """Records of 1, 2, 5 and 7 frames (a workgroup takes four at a time) of the CCSDS code at depth 4 and of a short code at depth
    3, every pattern in them."""
    rng = np.random.default_rng(45)
    return [M.make_case(code, rng, nf, M.PATTERNS) for code in (M.ccsds(4), M.Code(40, 36, 0x12B, 1, 11, 3)) for nf in (1, 2, 5, 7)]


def test_frame_counts_and_offsets(gpu, counted):
    for i, c in enumerate(counted):
        for off in OFFS:
            stats = torch.zeros(5, dtype=torch.int64, device="cuda:0")
            data, nerr = _decode(gpu, c["code"], c["recv"], c["nframes"], off, OFFS[(i + off) % 4], stats=stats)
            assert np.array_equal(nerr, c["nerr"]) and np.array_equal(data, c["out"]), (i, off)
            assert stats.cpu().tolist() == c["stats"]
            assert np.array_equal(_encode(gpu, c["code"], c["data"], c["nframes"], off, OFFS[(i + off + 1) % 4]), c["coded"])


def test_clean_corrected_and_failed_in_one_workgroup(gpu):
    rng = np.random.default_rng(46)
    c = M.make_case(M.ccsds(4), rng, 4, ("clean", "t", "t+1", "one"))
    assert {0, 1, 16, M.FAILED} <= set(c["nerr"].tolist()) and len(c["nerr"]) == 16           # sixteen codewords: one workgroup's four frames
    stats = torch.zeros(5, dtype=torch.int64, device="cuda:0")
    data, nerr = _decode(gpu, c["code"], c["recv"], 4, 3, 1, stats=stats)
    assert np.array_equal(nerr, c["nerr"]) and np.array_equal(data, c["out"]) and stats.cpu().tolist() == c["stats"]
    failed = np.repeat(c["nerr"].reshape(4, 4) == M.FAILED, 223, axis=0).reshape(4, 223, 4)      # [frame, symbol, codeword]
    got, recv = data.reshape(4, 223, 4), c["recv"].reshape(4, 255, 4)[:, :223, :]
    assert np.array_equal(got[failed], recv[failed])                                          # a failed codeword's data pass through


@pytest.mark.parametrize("which", (7, 3), ids=("short", "ccsds"))
def test_more_than_two_passes_of_the_grid(gpu, counted, which):
    """The seven-frame records repeated to 4 * (2 * 16 * cus + 5) + 1 frames, neither a multiple of 7 nor of 4: workgroup 0 takes
    three turns of its loop over the groups of four frames, re-using the stage and the waves' scratch and carrying its counters,
    every pattern meets every slot of a group, and the last group holds one frame.  Frames are independent, so the expected data
    and nerr are the model's, tiled, and the statistics the model's times the whole tiles plus the remainder's
    (tests/test_rs_host.py holds that arithmetic to bbb_rs_model_host).  The encoder's loop is out of reach at this cost: its
    grid is capped at 2^16 workgroups of 256 codewords a pass."""
    c = counted[which]
    code, nframes = c["code"], H.multipass_frames(grid.cus())
    assert c["nframes"] == 7 and nframes % 7 and nframes % 4
    recv, out, want_nerr, want_stats = H.tile_case(c, nframes)
    stats = torch.tensor([5, 4, 3, 2, 1], dtype=torch.int64, device="cuda:0")
    data, nerr = _decode(gpu, code, recv, nframes, 3, 1, stats=stats)
    assert np.array_equal(nerr, want_nerr), int(np.flatnonzero(nerr != want_nerr)[0])
    assert np.array_equal(data, out), int(np.flatnonzero(data != out)[0])
    assert stats.cpu().tolist() == [a + b for a, b in zip(want_stats, (5, 4, 3, 2, 1))]
    data, nerr = _decode(gpu, code, recv, nframes, 3, 1, want_nerr=False)
    assert np.array_equal(data, out) and len(nerr) == 0


def test_nothing_is_written_for_no_frames(gpu):
    from basebandboard_amd import _lib
    g = torch.full((64,), GUARD, dtype=torch.uint8, device="cuda:0")
    st = torch.full((5,), 7, dtype=torch.int64, device="cuda:0")
    cfg = _cfg(M.ccsds(4))
    assert _lib.lib().bbb_rs_decode(None, 0, C.byref(cfg), C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr() + 32), C.c_void_p(st.data_ptr()), 0, None) == 0
    assert _lib.lib().bbb_rs_encode(None, 0, C.byref(cfg), C.c_void_p(g.data_ptr()), 0, None) == 0
    torch.cuda.synchronize()
    assert (g.cpu().numpy() == GUARD).all() and st.cpu().tolist() == [7] * 5


def test_reed_solomon_class_and_stream(gpu, counted):
    c = counted[3]                                                                            # seven CCSDS frames at depth 4
    rs = gpu.ReedSolomon.ccsds(4)
    data = torch.from_numpy(c["data"]).to("cuda:0")
    coded = rs.encode(data)
    assert coded.dtype == torch.uint8 and np.array_equal(coded.cpu().numpy(), c["coded"])
    packed = torch.from_numpy(c["data"][:2 * 892].view(np.int64)).to("cuda:0")                   # two frames are whole words
    assert torch.equal(rs.encode(packed), coded[:2 * 1020])                                   # the packed view is the same bytes
    out, nerr = rs.decode(torch.from_numpy(c["recv"]).to("cuda:0"))
    assert np.array_equal(out.cpu().numpy(), c["out"]) and np.array_equal(nerr.cpu().numpy(), c["nerr"])
    assert list(rs.stats().values()) == c["stats"]
    with pytest.raises(ValueError, match="whole frames"):
        rs.decode(torch.zeros(1021, dtype=torch.uint8, device="cuda:0"))
    rng = np.random.default_rng(47)
    recv = torch.from_numpy(c["recv"]).to("cuda:0")
    for cuts in ([0, 1, 1019, 1020, 1021], sorted(rng.integers(0, len(c["recv"]) + 1, 9).tolist())):
        s, got, ne = rs.stream(), [], []
        edges = [0] + cuts + [len(c["recv"])]
        for lo, hi in zip(edges[:-1], edges[1:]):
            d, e = s.push(recv[lo:hi])
            got.append(d.cpu().numpy())
            ne.append(e.cpu().numpy())
        assert s.finish() == 0
        assert np.array_equal(np.concatenate(got), c["out"]) and np.array_equal(np.concatenate(ne), c["nerr"]), cuts
        assert np.array_equal(M.stream(c["code"], c["recv"], cuts)[0], c["out"])               # the same cuts in the model
    s = rs.stream()
    d, _ = s.push(recv[:1020 + 17])
    assert d.numel() == 892 and s.finish() == 17
    dvb = gpu.ReedSolomon.dvb()
    word = torch.arange(188, dtype=torch.uint8, device="cuda:0")
    assert np.array_equal(dvb.encode(word).cpu().numpy(), M.encode(M.dvb(), np.arange(188, dtype=np.uint8)))


@pytest.mark.parametrize("depth", (4, 1))
def test_concatenated_closed_loop_through_rx(gpu, depth):
    """The recipe of tests/test_rs_host.py on the GPU: Concatenated.encode gives the model's transmitted bits, and
    RX.count_errors(fec=Concatenated) of the noisy values counts the data bits the model found wrong behind both decoders."""
    code, data, coded, tx, rx = M.loop_record(depth)
    want = M.LOOP_COUNTS[depth]
    outer, inner = gpu.ReedSolomon.ccsds(depth), gpu.ConvCode(7, G171)
    cat = gpu.Concatenated(outer, inner)
    t, ntx = cat.encode(torch.from_numpy(data).to("cuda:0"))
    assert ntx == len(tx) and np.array_equal(np.unpackbits(t.cpu().numpy().view(np.uint8), bitorder="little")[:ntx], tx)
    xt = torch.from_numpy(rx).to("cuda:0")
    r = gpu.RX(M.LOOP["prbs"][0], 1, 0)
    hard, nh = r.slice(xt)
    channel = int((np.unpackbits(hard.cpu().numpy().view(np.uint8), bitorder="little")[:nh] != tx).sum())
    vit, nv = inner.decode(hard, hard=True, nbits=nh)
    viterbi = int((np.unpackbits(vit.cpu().numpy().view(np.uint8), bitorder="little")[:nv] != np.unpackbits(coded, bitorder="little")).sum())
    errors, nbits = r.count_errors(xt, fec=cat)
    st = outer.stats()
    got = dict(channel=channel, viterbi=viterbi, failed=st["failed"], data_bits=errors, symbols=st["symbols_corrected"])
    print(depth, got)
    assert nbits == 8 * len(data) and got == {k: want[k] for k in got}
    bits, nb = cat.decode(xt)                                                                 # soft decisions do at least as well here
    assert nb == nbits and int(np.unpackbits(bits.cpu().numpy().view(np.uint8)[:len(data)] ^ data).sum()) <= errors
    # terminated: K - 1 zero steps behind the frames, and a trailing partial frame is dropped
    term = gpu.Concatenated(outer, gpu.ConvCode(7, G171, terminated=True))
    t2, n2 = term.encode(torch.from_numpy(data[:code.data_bytes]).to("cuda:0"))
    assert n2 == 2 * (8 * code.frame_bytes + 6)
    clean = (2 * np.unpackbits(t2.cpu().numpy().view(np.uint8), bitorder="little")[:n2].astype(np.int16) - 1) * 64
    bits, nb = term.decode(torch.from_numpy(clean).to("cuda:0"))
    assert nb == 8 * code.data_bytes and np.array_equal(bits.cpu().numpy().view(np.uint8)[:code.data_bytes], data[:code.data_bytes])
