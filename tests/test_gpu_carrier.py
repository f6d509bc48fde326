"""bbb_carrier_run on the GPU against tests/carrier_model.py, bit for bit: the pairs turned back, the decisions, the soft values,
the estimate of every block, the state words and the counters of stats_dev, with guard values around every output, the input
at 4 modulo 16 bytes and the outputs off 16-byte alignment (and all of them on it: the wide loads and stores); records of
more than two passes of every capped grid and of more chunks than one chain thread's share; and the closed loop."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import carrier_model as M
import grid
import test_carrier_host as H

pytestmark = pytest.mark.gpu

# carrier_common.hpp, kCarrierGridPerCu; carrier_kernels.hip, carrier_launch(): cap = max(1, cus) * 8 workgroups for the sum and
# rotate kernels (a tile of floor(2048 / L) blocks a step) and for the flag and est kernels (a chunk a step)
CARRIER_TILES = 8
CARRIER_CHUNKS = 8
CHAIN_THREADS = 256        # carrier_chain_kernel: a thread owns ceil(nchunks / 256) chunks

GUARD = -0x0123456789ABCDEF
FILL16 = 0x5A5A
STATS0 = np.array([1000, 2000, 3000, 4000])


def _call(x, L=32, init=0, threshold=0, strict=False, chunk=0, state=(0, 0), final=True, aligned=False, outs=("iq", "bits", "soft", "phase")):
    """One bbb_carrier_run through the C ABI.  Every output lies between guard values that must stay as they were.  aligned:
    every pointer on a 16-byte boundary; otherwise the input at 4 modulo 16 bytes, the pairs out at 12, the words at 8, the
    soft values at 2.  Returns the model's dict (the outputs not asked for are missing)."""
    from basebandboard_amd import _lib
    dev = torch.device("cuda", 0)
    x = np.ascontiguousarray(x, dtype=np.int16).reshape(-1, 2)
    nblocks, n = M.plan(len(x), L, final)
    nwords = (nblocks * L + 63) // 64
    in_off, iq_off, bits_off, soft_off, ph_off = (4, 4, 2, 8, 8) if aligned else (1, 3, 1, 1, 1)
    buf = torch.zeros((in_off + len(x) + 4, 2), dtype=torch.int16, device=dev)
    buf[in_off:in_off + len(x)] = torch.from_numpy(x).to(dev)
    iq = torch.full((iq_off + n + 2, 2), FILL16, dtype=torch.int16, device=dev)
    bits = torch.full((bits_off + nwords + 1,), GUARD, dtype=torch.int64, device=dev)
    sv = torch.full((soft_off + n + 3,), FILL16, dtype=torch.int16, device=dev)
    ph = torch.full((ph_off + nblocks + 3,), FILL16, dtype=torch.int16, device=dev)
    to_i64 = lambda v: int(np.array([v], dtype=np.uint64).view(np.int64)[0])                                # noqa: E731
    st = torch.tensor([GUARD, to_i64(state[0]), to_i64(state[1]), GUARD], dtype=torch.int64, device=dev)
    stats = torch.tensor([GUARD] + STATS0.tolist() + [GUARD], dtype=torch.int64, device=dev)
    p_in, p_iq, p_bits = buf.data_ptr() + 4 * in_off, iq.data_ptr() + 4 * iq_off, bits.data_ptr() + 8 * bits_off
    p_soft, p_ph = sv.data_ptr() + 2 * soft_off, ph.data_ptr() + 2 * ph_off
    if aligned:
        assert not (p_in % 16 or p_iq % 16 or p_bits % 16 or p_soft % 16)
    else:
        assert (p_in % 16, p_iq % 16, p_bits % 16, p_soft % 16) == (4, 12, 8, 2)
    ptr = lambda name, p: C.c_void_p(p) if name in outs else None                                          # noqa: E731
    c = _lib.CarrierCfg(L, init, threshold, int(strict), chunk)
    _lib.check(_lib.lib().bbb_carrier_run(C.c_void_p(p_in), len(x), int(final), C.byref(c), C.c_void_p(st.data_ptr() + 8), ptr("iq", p_iq),
                                          ptr("bits", p_bits), ptr("soft", p_soft), ptr("phase", p_ph), C.c_void_p(stats.data_ptr() + 8), 0,
                                          C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "bbb_carrier_run")
    got = {}
    a = iq.cpu().numpy()
    lo, hi = (iq_off, iq_off + n) if "iq" in outs else (0, 0)
    assert (a[:lo] == FILL16).all() and (a[hi:] == FILL16).all(), "a pair next to iq_dev was written"
    got["iq"] = a[lo:hi]
    w = bits.cpu().numpy()
    lo, hi = (bits_off, bits_off + nwords) if "bits" in outs else (0, 0)
    assert (w[:lo] == GUARD).all() and (w[hi:] == GUARD).all(), "a word next to bits_packed_dev was written"
    got["words"] = w[lo:hi].view(np.uint64)
    s = sv.cpu().numpy()
    lo, hi = (soft_off, soft_off + n) if "soft" in outs else (0, 0)
    assert (s[:lo] == FILL16).all() and (s[hi:] == FILL16).all(), "a value next to soft_dev was written"
    got["soft"] = s[lo:hi]
    p = ph.cpu().numpy()
    lo, hi = (ph_off, ph_off + nblocks) if "phase" in outs else (0, 0)
    assert (p[:lo] == FILL16).all() and (p[hi:] == FILL16).all(), "a value next to phase_dev was written"
    got["phases"] = p[lo:hi].view(np.uint16)
    sw = st.cpu().numpy()
    assert sw[0] == GUARD and sw[3] == GUARD, "a word next to state_dev was written"
    tw = stats.cpu().numpy()
    assert tw[0] == GUARD and tw[5] == GUARD, "a word next to stats_dev was written"
    got.update(state=tuple(int(v) for v in sw[1:3].view(np.uint64)), stats=(tw[1:5] - STATS0).tolist())
    return got


def _same(got, want, what="", outs=("iq", "bits", "soft", "phase")):
    for name, key in (("iq", "iq"), ("bits", "words"), ("soft", "soft"), ("phase", "phases")):
        if name in outs:
            g, w = np.asarray(got[key]).reshape(-1), np.asarray(want[key]).reshape(-1)
            assert len(g) == len(w), f"{what}: {key} has {len(g)} elements, not {len(w)}"
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, f"{what}: {key} differs in {len(bad)} places, the first at {bad[0]}: {g[bad[0]]} != {w[bad[0]]}"
    assert got["state"] == want["state"], f"{what}: state {got['state']} != {want['state']}"
    assert got["stats"] == want["stats"], f"{what}: stats {got['stats']} != {want['stats']}"


def _check(x, L=32, init=0, threshold=0, strict=False, chunks=(0,), state=(0, 0), final=True, aligned=(False, True), what=""):
    """The call, once per chunk_blocks and alignment, against the model; returns the model's dict."""
    want = M.run(x, L, init, threshold, strict, state, final)
    for chunk in chunks:
        for al in aligned:
            _same(_call(x, L, init, threshold, strict, chunk, state, final, al), want, f"{what} chunk_blocks {chunk} aligned {al}")
    return want


def _noise(rng, n):
    x = rng.integers(-32768, 32768, (n, 2))
    x[3::61] = (-32768, -32768)
    return x


@pytest.mark.parametrize("L", (8, 24, 32, 1024))
def test_every_block_size_and_length(gpu, L):
    """nin = 1, L - 1, L, L + 1 and the tile of floor(2048 / L) blocks - 1, + 0, + 1, and three tiles and a ragged tail, final
    and not; chunk_blocks 1, 3 and the default; both alignments.  Full-range noise: h is uniform, f_j = 1 in a quarter of the
    blocks (the difference of two uniform values is triangular: a quarter of it lies beyond half the range).  At
    L = 24 a tile holds 85 blocks, 2040 pairs: blocks and tiles do not line up with the threads' 2048."""
    rng = np.random.default_rng(100 + L)
    tile = 2048 // L * L
    flips = blocks = 0
    for i, n in enumerate((1, L - 1, L, L + 1, tile - 1, tile, tile + 1, 3 * tile + 5 * L + 3)):
        x = _noise(rng, n)
        for final in (True, False):
            want = _check(x, L, int(rng.integers(0, 65536)), int(rng.integers(-40, 40)), bool(i & 1), ((1, 0), (3,), (0, 1), (3, 0))[i % 4], final=final,
                          what=f"L {L} n {n} final {final}")
            flips, blocks = flips + want["stats"][1], blocks + want["stats"][0]
    assert blocks > 0 and 0 < flips < blocks


def test_full_scale_zero_blocks_and_saturation(gpu):
    """Blocks of (-32768, -32768): SI = 2^41 at L = 1024, the largest sum there is, and turned onto +I the pair saturates.  Zero
    blocks: h = 0, counted.  A started state goes on from its estimate."""
    x = np.full((2048 + 7, 2), -32768)
    for L in (8, 1024):
        want = _check(x, L, 8192 + 32768, chunks=(1, 0), what=f"full scale L {L}")
        assert (want["iq"][:, 0] == 32767).all() and set(want["phases"].tolist()) == {8192 + 32768}
        assert (_check(x, L, 8192, what=f"full scale the other way L {L}")["iq"][:, 0] == -32768).all()
    z = np.zeros((8 * 50 + 3, 2))
    z[80:88] = (100, 100)
    want = _check(z, 8, 40000, threshold=0, chunks=(3, 0), what="zero blocks")
    assert want["stats"][2] == 50 and want["bits"][:80].all()
    want = _check(z, 8, 40000, threshold=0, strict=True, chunks=(3,), what="zero blocks, strict")
    assert not want["bits"][:80].any()
    rng = np.random.default_rng(7)
    want = _check(rng.integers(-500, 500, (300, 2)), 32, 123, state=(M.STARTED | 54321, 12345), chunks=(2,), what="started")
    assert want["state"][1] == 12345 + 300
    none = _check(rng.integers(-500, 500, (31, 2)), 32, state=(M.STARTED | 6, 5), final=False, what="no block")
    assert none["state"] == (M.STARTED | 6, 5) and none["stats"] == [0, 0, 0, 0]
    assert _check(np.zeros((0, 2)), 32, state=(M.STARTED | 6, 5), what="no pair")["state"] == (M.STARTED | 6, 5)


def test_ties_of_the_unwrap(gpu):
    """Blocks of a constant vector at angles for which h_j - h_(j-1) is 16383, 16384, 49151 and 49152 (and 16385, 49153): the four
    edges of near(), entered from both halves and from a quarter turn away."""
    for L in (8, 24):
        x, hs = H.tie_blocks(L)
        for init in (hs[0], hs[0] + 32768, (hs[0] + 16384) % 65536, (hs[0] + 16383) % 65536, (hs[0] - 16384) % 65536, (hs[0] - 16385) % 65536):
            want = _check(x, L, init, chunks=(1, 3, 0), aligned=(False,), what=f"ties L {L} init {init}")
            assert (want["phases"] & 0x7FFF).tolist() == hs


def test_each_output_alone(gpu):
    """Every output may be NULL: what is not asked for is not written (the guards of _call), phase_dev alone skips the rotation."""
    rng = np.random.default_rng(8)
    x = _noise(rng, 5000)
    want = M.run(x, 24, 99, 3, True)
    for outs in (("iq",), ("bits",), ("soft",), ("phase",), ("bits", "phase")):
        for al in (False, True):
            _same(_call(x, 24, 99, 3, True, 5, aligned=al, outs=outs), want, f"outputs {outs}", outs)


@pytest.fixture(scope="module")
def long_record():
    """2^21 pairs at L = 8: 2^18 blocks.  (pairs, the model's dict)"""
    x = _noise(np.random.default_rng(9), 1 << 21)
    return x, M.run(x, 8, 4242, -9, False)


@pytest.mark.parametrize("chunk", (1, 3, 0, 5000))
def test_more_chunks_than_chain_threads(gpu, long_record, chunk):
    """chunk_blocks 1: 2^18 chunks, a chain thread's share is 1024 of them, and the flag and est kernels take 2^18 / (8 cus)
    turns.  chunk_blocks 3, the default (256 chunks of 1024 blocks, half a turn of the flag kernel's 2048 blocks) and 5000 (three
    turns a chunk, the last ragged inside a thread's 8 blocks)."""
    x, want = long_record
    nchunks = -(-want["nblocks"] // (chunk or 1024))
    assert chunk != 1 or (nchunks > 4 * CHAIN_THREADS and nchunks > 2 * CARRIER_CHUNKS * grid.cus())
    _same(_call(x, 8, 4242, -9, False, chunk, aligned=chunk == 0), want, f"2^21 pairs, chunk_blocks {chunk}")


def test_more_than_two_passes_of_the_grids(gpu):
    """L = 24: 2 * 8 * cus + 5 tiles of 85 blocks and a ragged last one, so that the sum and rotate kernels take a third turn with a
    prefetched tile; chunks of 64 blocks, more than 2 * 8 * cus of them, for the flag and est kernels."""
    L, per = 24, 2048 // 24
    ntiles = grid.passes(CARRIER_TILES)
    nblocks = per * (ntiles - 1) + 7
    n = (nblocks - 1) * L + 11
    assert -(-nblocks // per) == ntiles > 2 * CARRIER_TILES * grid.cus() and -(-nblocks // 64) > 2 * CARRIER_CHUNKS * grid.cus()
    x = _noise(np.random.default_rng(10), n)
    want = M.run(x, L, 31000, 17, True)
    assert want["nblocks"] == nblocks and 0.2 * nblocks < want["stats"][1] < 0.3 * nblocks
    _same(_call(x, L, 31000, 17, True, 64), want, "multipass")
    _same(_call(x, L, 31000, 17, True, 64, aligned=True, outs=("bits",)), want, "multipass, decisions alone", ("bits",))


def _unpack(words, n):
    return np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")[:n]


def test_a_record_cut_at_block_boundaries_equals_one_call(gpu):
    rng = np.random.default_rng(11)
    L = 24
    n = 300 * L + 17
    x = _noise(rng, n)
    want = M.run(x, L, 777, 5, True)
    cr = gpu.CarrierRecovery(L, 777, threshold=5, strict=True, chunk_blocks=7)
    xt = torch.from_numpy(x.astype(np.int16)).to("cuda:0")
    cuts = sorted(set((rng.integers(1, 300, 9) * L).tolist()))
    st = cr.new_state()
    iq, bits, soft, phases = [], [], [], []
    for lo, hi in zip([0] + cuts, cuts + [n]):
        a, b, nb, s, ph = cr.recover(xt[lo:hi], state=st, final=hi == n)
        assert nb == hi - lo
        iq.append(a.cpu().numpy())
        bits.append(_unpack(b, nb))
        soft.append(s.cpu().numpy())
        phases.append(ph.cpu().numpy())
    assert np.array_equal(np.concatenate(iq), want["iq"]) and np.array_equal(np.concatenate(bits), want["bits"])
    assert np.array_equal(np.concatenate(soft), want["soft"]) and np.array_equal(np.concatenate(phases), want["phases"])
    assert tuple(int(v) for v in st.cpu().numpy().view(np.uint64)) == want["state"]
    assert cr.stats() == dict(zip(("blocks", "flips", "zero_blocks", "phase_steps"), want["stats"]))
    assert cr.carrier_offset() == want["stats"][3] / (want["stats"][0] * L * 65536.0)
    cr.reset()
    assert cr.stats()["blocks"] == 0
    # derotate and slice alone are recover's outputs; a call that is not final leaves the ragged tail
    assert np.array_equal(cr.derotate(xt).cpu().numpy(), want["iq"])
    b, nb = cr.slice(xt, final=False)
    assert nb == 300 * L and np.array_equal(_unpack(b, nb), want["bits"][:nb])


def test_a_stream_in_chunks_of_any_size_equals_recover(gpu):
    rng = np.random.default_rng(12)
    L = 40
    n = 150 * L + 31
    x = _noise(rng, n)
    want = M.run(x, L, 50000, -3)
    xt = torch.from_numpy(x.astype(np.int16)).to("cuda:0")
    cr = gpu.CarrierRecovery(L, 50000, threshold=-3, chunk_blocks=5)
    s = cr.stream("all")
    edges = [0] + sorted(rng.integers(0, n, 14).tolist() + [0, 7, 7, 39, 40, 41]) + [n]
    iq, bits, soft = [], [], []
    for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        a, b, nb, z, _ = s.push(xt[lo:hi], final=i == len(edges) - 2)
        iq.append(a.cpu().numpy())
        bits.append(_unpack(b, nb))
        soft.append(z.cpu().numpy())
    assert np.array_equal(np.concatenate(iq), want["iq"]) and np.array_equal(np.concatenate(bits), want["bits"])
    assert np.array_equal(np.concatenate(soft), want["soft"]) and np.array_equal(np.concatenate([p.cpu().numpy() for p in s.phases]), want["phases"])
    assert tuple(int(v) for v in s.state.cpu().numpy().view(np.uint64)) == want["state"]
    s2 = cr.stream()
    assert np.array_equal(torch.cat([s2.push(xt[:1000]), s2.push(xt[1000:], final=True)]).cpu().numpy(), want["iq"])


def test_invalid_arguments_on_the_gpu(gpu):
    """Every BBB_EINVAL of tests/test_carrier_host.py, with a device present: refused before the device is touched (the pointers
    are numbers no device gave out)."""
    from basebandboard_amd import _lib
    for cfg, kw, what in H.INVALID:
        assert H.run_rc(cfg, **kw) == _lib.BBB_EINVAL, what
        assert re.search(what, _lib.lib().bbb_last_error_detail().decode()), what


@pytest.fixture(scope="module")
def loop():
    return M.loop_capture()


@pytest.mark.parametrize("off", M.LOOP["offsets"])
def test_closed_loop(gpu, loop, off):
    """The down-converter's example with its fcw 256 off the transmitter's, through RX.downconvert(..., carrier=...): the GPU's pairs
    and decisions are the model's, the model's decisions are the data, the sign of Q is not, and carrier_offset() is the offset."""
    P = M.LOOP
    capture, data = loop
    pairs = M.loop_pairs(capture, off)
    want = M.run(pairs, P["L"], P["init_phase"])
    fcw = P["fcw"] - off
    ddc = gpu.DDC(fcw, P["taps"], decim=P["decim"], phase=P["decim"] - 1, shift=P["shift"], pa0=(-3 * fcw) % (1 << 24))
    ct = torch.from_numpy(capture).to("cuda:0")
    # phase 66 = 3 + 63: the converter's phase must be below decim, so the record is entered 3 samples late with those 3 as history
    raw = ddc.iq(ct, first_sample=3, nbefore=3)
    assert np.array_equal(raw.cpu().numpy(), pairs), "the down-converter's pairs differ from the model's"
    cr = gpu.CarrierRecovery(P["L"], P["init_phase"])
    iq = gpu.RX(7, P["spb"], 0).downconvert(ct, ddc, carrier=cr, first_sample=3, nbefore=3)
    assert np.array_equal(iq.cpu().numpy(), want["iq"])
    cr2 = gpu.CarrierRecovery(P["L"], P["init_phase"])
    words, nbits = cr2.slice(raw)
    bits = _unpack(words, nbits)
    assert nbits == 4095 and np.array_equal(bits, want["bits"])
    errors = int((want["bits"] != data[:4095]).sum())
    q_errors = int(((pairs[:, 1] > 0) != (data[:4095] == 1)).sum())
    offset = cr2.carrier_offset()
    print("offset", off, "errors", errors, "of 4095, the sign of Q leaves", q_errors, "stats", cr2.stats(), "carrier offset", offset, "ideal", M.loop_ideal_offset(off))
    assert errors < 0.01 * 4095
    assert q_errors > 0.40 * 4095
    assert offset * off > 0 and abs(offset - M.loop_ideal_offset(off)) < 0.02 * abs(M.loop_ideal_offset(off))
    assert cr.stats() == cr2.stats() == dict(zip(("blocks", "flips", "zero_blocks", "phase_steps"), want["stats"]))
