"""bbb_ldpc_decode and bbb_ldpc_encode on the GPU, bit for bit against tests/ldpc_model.py: the grid of tests/test_ldpc_host.py
(Z 2..512, J 1..32, K up to 64, the LDS maxima, row degrees 2 and 32, soft and hard values at starts that are odd and straddle
words, every kind of codeword in one group), data, iters and statistics, between guard words, the statistics added to over two
calls, the outputs that may be left out; the encoder against bbb_ldpc_encode_host; the Python classes LDPC, LDPCStream cut at
ragged points and RX.slice(fec=LDPC); more than two passes of the decoder's capped grid; one call whose value indices pass 2^31
and 2^32; and the closed loop's counts."""
import ctypes as C

import numpy as np
import pytest
import torch

import grid
import ldpc_model as M
import periodic as P
import test_ldpc_host as H

pytestmark = pytest.mark.gpu

LDPC_DECODE = 8    # ldpc_kernels.hip, ldpc_decode_launch(): min(ngrp, max(1, cus) * 8), a group of codewords a workgroup's turn

GUARD = H.GUARD - (1 << 64)                                                          # as int64
OFFS = (0, 1, 3, 7)

unit7 = H.unit7                                                                    # the module's fixture: seven codewords of array(31, 3, 6)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def _guarded_words(nwords, off):
    """A device buffer of guard words and the index of the first of nwords expected words."""
    t = torch.full((nwords + 8 + off,), GUARD, dtype=torch.int64, device="cuda:0")
    return t, 4 + off


def _payload(t, start, n, guard):
    got = t.cpu().numpy()
    assert (got[:start] == guard).all() and (got[start + n:] == guard).all(), "memory outside the output was written"
    return got[start:start + n]


def _decode(gpu, c, in_off=0, out_off=0, want_iters=True, stats=None, ncw=None, buf=None):
    """One bbb_ldpc_decode through the C ABI: the case's buffer in_off halfwords (words for HARD) behind an allocation's start.
    stats: a device int64[5] that is added to, or None.  Returns (packed data words as uint64, iters)."""
    from basebandboard_amd import _lib
    code, ncw = c["code"], c["ncw"] if ncw is None else ncw
    host = H.in_buffer(c) if buf is None else buf
    host = host.view(np.int64) if c["hard"] else host
    src = torch.zeros(len(host) + in_off, dtype=torch.int64 if c["hard"] else torch.int16, device="cuda:0")
    src[in_off:] = torch.from_numpy(host).to("cuda:0")
    before = src.clone()
    nw = (ncw * code.k + 63) // 64
    bits, b0 = _guarded_words(nw, out_off)
    iters = torch.full((ncw + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    e0 = 16 + (out_off + 1) % 16
    rc = _lib.lib().bbb_ldpc_decode(C.c_void_p(src.data_ptr() + in_off * src.element_size()), c["in_first"], ncw, int(c["hard"]), C.byref(H._cfg(code)),
                                    C.c_void_p(bits.data_ptr() + 8 * b0), C.c_void_p(iters.data_ptr() + e0) if want_iters else None,
                                    C.c_void_p(stats.data_ptr()) if stats is not None else None, 0, _stream())
    assert rc == 0, _lib.lib().bbb_last_error_detail()
    assert torch.equal(src, before), "the input was written"
    return _payload(bits, b0, nw, GUARD).view(np.uint64), _payload(iters, e0, ncw if want_iters else 0, 0xA5)


def _encode(gpu, code, data, ncw, in_off=0, out_off=0):
    from basebandboard_amd import _lib
    words = M.pack(data).view(np.int64)
    src = torch.zeros(len(words) + in_off, dtype=torch.int64, device="cuda:0")
    src[in_off:] = torch.from_numpy(words).to("cuda:0")
    nw = (ncw * code.n + 63) // 64
    out, o0 = _guarded_words(nw, out_off)
    rc = _lib.lib().bbb_ldpc_encode(C.c_void_p(src.data_ptr() + 8 * in_off), ncw, C.byref(H._cfg(code)), C.c_void_p(out.data_ptr() + 8 * o0), 0, _stream())
    assert rc == 0, _lib.lib().bbb_last_error_detail()
    return _payload(out, o0, nw, GUARD).view(np.uint64)


def test_decode_equals_the_model_on_the_grid(gpu):
    for i, c in enumerate(M.grid_cases()):
        code = c["code"]
        what = (i, code.Z, code.J, code.K, c["hard"], c["in_first"])
        stats = torch.tensor([5, 4, 3, 2, 1], dtype=torch.int64, device="cuda:0")
        bits, iters = _decode(gpu, c, OFFS[i % 4], OFFS[(i // 4) % 4], stats=stats)
        assert np.array_equal(iters, c["iters"]), (what, iters, c["iters"])
        assert np.array_equal(bits, M.pack(c["out"])), what
        # the second call: no iters, the same statistics added again
        bits, iters = _decode(gpu, c, OFFS[(i + 1) % 4], OFFS[(i // 4 + 1) % 4], want_iters=False, stats=stats)
        assert np.array_equal(bits, M.pack(c["out"])) and len(iters) == 0
        assert stats.cpu().tolist() == [2 * a + b for a, b in zip(c["stats"], (5, 4, 3, 2, 1))], (what, stats.cpu().tolist(), c["stats"])
        # and without statistics
        bits, iters = _decode(gpu, c)
        assert np.array_equal(bits, M.pack(c["out"])) and np.array_equal(iters, c["iters"])


def test_encode_equals_encode_host_on_the_grid(gpu):
    n = 0
    for i, c in enumerate(M.grid_cases()):
        code = c["code"]
        if not code.triangular:
            continue
        host = H._encode_host(code, c["data"], c["ncw"])
        got = _encode(gpu, code, c["data"], c["ncw"], OFFS[i % 4], OFFS[(i // 4) % 4])
        assert np.array_equal(got, host) and np.array_equal(got, M.pack(c["coded"])), (i, code.Z, code.J, code.K)
        n += 1
    assert n >= 20


def test_codeword_counts_around_a_group(gpu, unit7):
    """1, 2, 7, 8 and 9 codewords of array(31, 3, 6), whose group is eight: groups that are not full, one that is, one and one more."""
    code = unit7["code"]
    nine = H.tile_case(unit7, 9)
    for ncw in (1, 2, 7, 8, 9):
        c = dict(unit7, ncw=ncw)
        stats = torch.zeros(5, dtype=torch.int64, device="cuda:0")
        bits, iters = _decode(gpu, c, ncw % 8, 1, stats=stats, ncw=ncw, buf=nine[0][:ncw * code.n])
        want = H.tile_case(unit7, ncw)
        assert np.array_equal(bits, M.pack(want[1])) and np.array_equal(iters, want[2]) and stats.cpu().tolist() == want[3], ncw
        assert np.array_equal(_encode(gpu, code, np.tile(unit7["data"], 2)[:ncw * code.k], ncw, 1, 2),
                              M.pack(np.tile(unit7["coded"], 2)[:ncw * code.n]))



def test_more_than_two_passes_of_the_grid(gpu, unit7):
    """The seven-codeword record repeated to 8 * (2 * LDPC_DECODE * cus + 5) + 3 codewords, neither a multiple of 7 nor of 8:
    workgroup 0 takes three turns of its loop over the groups, re-using its LDS and carrying its counters, every kind meets every
    slot of a group, and the last group holds three codewords.  Codewords are independent, so the expected values are the model's,
    tiled (tests/test_ldpc_host.py holds that arithmetic to bbb_ldpc_model_host)."""
    ncw = H.multipass_codewords(LDPC_DECODE, grid.cus())
    assert ncw % 7 and ncw % 8 == 3
    vals, out, want_iters, want_stats = H.tile_case(unit7, ncw)
    stats = torch.tensor([5, 4, 3, 2, 1], dtype=torch.int64, device="cuda:0")
    bits, iters = _decode(gpu, dict(unit7, ncw=ncw), 3, 1, stats=stats, ncw=ncw, buf=vals)
    assert np.array_equal(iters, want_iters), int(np.flatnonzero(iters != want_iters)[0])
    assert np.array_equal(bits, M.pack(out)), int(np.flatnonzero(bits != M.pack(out))[0])
    assert stats.cpu().tolist() == [a + b for a, b in zip(want_stats, (5, 4, 3, 2, 1))]
    # the encoder: one codeword a workgroup's turn, its grid capped at 16 workgroups per compute unit
    nenc = 2 * 16 * grid.cus() + 5
    data = np.tile(unit7["data"], -(-nenc // 7))[:nenc * unit7["code"].k]
    coded = np.tile(unit7["coded"], -(-nenc // 7))[:nenc * unit7["code"].n]
    assert np.array_equal(_encode(gpu, unit7["code"], data, nenc, 1, 3), M.pack(coded))


def test_nothing_is_written_for_no_codewords(gpu):
    from basebandboard_amd import _lib
    g = torch.full((8,), GUARD, dtype=torch.int64, device="cuda:0")
    st = torch.full((5,), 7, dtype=torch.int64, device="cuda:0")
    cfg = H._cfg(M.array(31, 3, 6))
    assert _lib.lib().bbb_ldpc_decode(None, 0, 0, 0, C.byref(cfg), C.c_void_p(g.data_ptr()), C.c_void_p(g.data_ptr() + 32), C.c_void_p(st.data_ptr()), 0, None) == 0
    assert _lib.lib().bbb_ldpc_encode(None, 0, C.byref(cfg), C.c_void_p(g.data_ptr()), 0, None) == 0
    torch.cuda.synchronize()
    assert (g.cpu().numpy() == GUARD).all() and st.cpu().tolist() == [7] * 5


def test_ldpc_class_stream_and_rx(gpu):
    c = M.grid_cases()[3]                                                            # nine codewords of array(31, 3, 6), every kind
    code, vals = c["code"], c["values"]
    ld = gpu.LDPC.array(31, 3, 6)
    coded, nc = ld.encode(torch.from_numpy(M.pack(c["data"]).view(np.int64)).to("cuda:0"), 9)
    assert nc == 9 * 186 and np.array_equal(coded.cpu().numpy().view(np.uint64), M.pack(c["coded"]))
    xt = torch.from_numpy(vals).to("cuda:0")
    bits, nb = ld.decode(xt)
    assert nb == 9 * 93 and np.array_equal(bits.cpu().numpy().view(np.uint64), M.pack(c["out"]))
    assert np.array_equal(ld.iterations().cpu().numpy(), c["iters"]) and list(ld.stats().values()) == c["stats"]
    bits, nb = ld.decode(xt[:186 * 4 + 100])                                         # a ragged tail is ignored
    assert nb == 4 * 93 and np.array_equal(bits.cpu().numpy().view(np.uint64), M.pack(c["out"][:4 * 93])) and ld.iterations().numel() == 4
    rng = np.random.default_rng(57)
    for cuts in ([0, 1, 185, 186, 187], sorted(rng.integers(0, len(vals) + 1, 9).tolist())):
        s, got, its = ld.stream(), [], []
        edges = [0] + cuts + [len(vals)]
        for lo, hi in zip(edges[:-1], edges[1:]):
            b, n, it = s.push(xt[lo:hi])
            got.append(M.unpack(b.cpu().numpy(), n))
            its.append(it.cpu().numpy())
        assert s.finish() == 0
        assert np.array_equal(np.concatenate(got), c["out"]) and np.array_equal(np.concatenate(its), c["iters"]), cuts
        assert np.array_equal(M.stream(code, vals, cuts)[0], c["out"])               # the same cuts in the model
    s = ld.stream()
    b, n, _ = s.push(xt[:186 + 17])
    assert n == 93 and s.finish() == 17
    # RX.slice(fec=LDPC): the hard decisions of the samples are the received bits of the codewords, one call
    want = M.decode(code, (vals > 0).astype(np.uint8), hard=True)
    r = gpu.RX(31, 1, 0)
    hard, nh = r.slice(xt, strict=True)
    assert nh == len(vals)
    one, n1 = ld.decode(hard, hard=True, nbits=nh)
    got, n2 = r.slice(xt, strict=True, fec=ld)
    assert n1 == n2 == 9 * 93 and torch.equal(one, got) and np.array_equal(got.cpu().numpy().view(np.uint64), M.pack(want[0]))
    assert np.array_equal(ld.iterations().cpu().numpy(), want[1])


def test_closed_loop_counts(gpu):
    """The recipe of tests/test_ldpc_host.py on the GPU: LDPC.encode gives the model's coded bits, and decoding the noisy values
    gives the model's counts at sigma 32, at sigma 40 and from hard decisions."""
    for sigma, hard in ((32, False), (40, False), (32, True)):
        code, data, coded, vals = M.loop_record(sigma)
        ld = gpu.LDPC.array(M.LOOP["p"], M.LOOP["J"], M.LOOP["K"])
        tx, ntx = ld.encode(torch.from_numpy(M.pack(data).view(np.int64)).to("cuda:0"), M.LOOP["ncw"])
        assert ntx == len(coded) and np.array_equal(tx.cpu().numpy().view(np.uint64), M.pack(coded))
        xt = torch.from_numpy(vals).to("cuda:0")
        if hard:
            hb, nh = gpu.RX(31, 1, 0).slice(xt, strict=True)
            bits, nb = ld.decode(hb, hard=True, nbits=nh)
        else:
            bits, nb = ld.decode(xt)
        st = ld.stats()
        got = dict(channel=int(((vals > 0) != coded).sum()), data=int((M.unpack(bits.cpu().numpy(), nb) != data).sum()), failed=st["failed"],
                   iters=st["iterations"])
        print(sigma, hard, got)
        assert nb == len(data) and got == M.LOOP_COUNTS[(sigma, hard)]


def test_value_indices_past_2_32(gpu):
    """Seven codewords of array(31, 3, 6) (tests/test_ldpc_host.py, wide_unit: five clean, two that need iterations) tiled until
    the index of a value passes 2^32 (the index of a data bit passes 2^31 on the way), with three periods and a ragged tail
    behind it, in one call.  Data, iters and statistics against the model's, tiled."""
    u = H.wide_unit()
    code = u["code"]
    p, tail_cw, extra = len(u["values"]), 3, 100
    K = P.periods_past(P.P32, p, tail_cw * code.n + extra)
    nvals = K * p + tail_cw * code.n + extra
    ncw = 7 * K + tail_cw
    assert nvals > P.P32 + 3 * p and ncw * code.k > P.P31
    ld = gpu.LDPC.array(31, 3, 6)
    rec = P.tile(P.to_dev(u["values"]), nvals)
    bits, nb = ld.decode(rec)
    del rec
    assert nb == ncw * code.k
    ex = P.Expect(u["out"], u["out"], u["out"][:tail_cw * code.k])
    assert P.assert_tiled_bits(bits, ex, K, what="ldpc data bits") == nb
    P.assert_tiled(ld.iterations(), u["iters"][:0], u["iters"], u["iters"][:tail_cw], what="ldpc iters")
    tail = M.decode(code, u["values"][:tail_cw * code.n])[2]
    assert list(ld.stats().values()) == [K * a + b for a, b in zip(u["stats"], tail)]
