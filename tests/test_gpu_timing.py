"""bbb_timing_run on the GPU against tests/timing_model.py, bit for bit: bits, soft values, the phase of every block, the state
words, the counters of stats_dev and nbits_dev, with guard words around every output and the pointers off 16-byte alignment
where the ABI allows it; and records of more than two passes of every kernel's grid."""
import ctypes as C

import numpy as np
import pytest
import torch

import fir_model
import grid
import timing_model as M
import test_timing_host as H

pytestmark = pytest.mark.gpu

GUARD = -0x0123456789ABCDEF
SOFT_FILL = 0x5A5A
STATS0 = np.array([1000, 2000, 3000, 4000])


def _call(x, nb, P, taps=(1,), L=64, h=4, threshold=0, strict=False, init=M.ACQUIRE, chunk=0, state=(0, 0), final=True, shift=0, soft=np.int16,
          in_off=1, bits_off=1, soft_off=1):
    """One bbb_timing_run through the C ABI.  Every output lies one or more elements behind an aligned address, between guard
    values that must stay as they were; the three big pointers are off 16-byte alignment.  Returns the model's dict."""
    from basebandboard_amd import _lib
    dev = torch.device("cuda", 0)
    x = np.asarray(x, dtype=np.int16)
    nin = len(x) - nb
    nblocks, _, max_bits = M.plan(nin, P, L, final)
    nwords = (max_bits + 63) // 64
    in_off += (in_off + nb) % 8 == 0                                          # never onto a 16-byte boundary
    soft_off += soft_off * np.dtype(soft).itemsize % 16 == 0
    buf = torch.zeros(in_off + len(x) + 8, dtype=torch.int16, device=dev)
    buf[in_off:in_off + len(x)] = torch.from_numpy(x).to(dev)
    bits = torch.full((bits_off + nwords + 1,), GUARD, dtype=torch.int64, device=dev)
    sdt = torch.int16 if soft == np.int16 else torch.int32
    sv = torch.full((soft_off + max_bits + 1,), SOFT_FILL, dtype=sdt, device=dev)
    ph = torch.full((1 + nblocks + 1,), 0xEE, dtype=torch.uint8, device=dev)
    to_i64 = lambda v: int(np.array([v], dtype=np.uint64).view(np.int64)[0])                                # noqa: E731
    st = torch.tensor([GUARD, to_i64(state[0]), to_i64(state[1]), GUARD], dtype=torch.int64, device=dev)
    stats = torch.tensor([GUARD] + STATS0.tolist() + [GUARD], dtype=torch.int64, device=dev)
    cnt = torch.full((3,), GUARD, dtype=torch.int64, device=dev)
    c = _lib.TimingCfg()
    c.ff.ntaps = len(taps)
    for i, v in enumerate(taps):
        c.ff.taps[i] = v
    c.ff.shift, c.ff.decim, c.ff.phase, c.ff.out_bytes = shift, 1, 0, np.dtype(soft).itemsize
    c.spb, c.block_symbols, c.hysteresis_shift, c.threshold, c.strict, c.init_phase, c.chunk_blocks = P, L, h, threshold, int(strict), init, chunk
    p_in, p_bits, p_soft = buf.data_ptr() + 2 * (in_off + nb), bits.data_ptr() + 8 * bits_off, sv.data_ptr() + sv.element_size() * soft_off
    assert p_in % 16 and p_bits % 16 and p_soft % 16, (p_in % 16, p_bits % 16, p_soft % 16)
    _lib.check(_lib.lib().bbb_timing_run(C.c_void_p(p_in), nin, nb, int(final), C.byref(c), C.c_void_p(st.data_ptr() + 8), C.c_void_p(p_bits),
                                         C.c_void_p(p_soft), C.c_void_p(ph.data_ptr() + 1), C.c_void_p(stats.data_ptr() + 8),
                                         C.c_void_p(cnt.data_ptr() + 8), 0, C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "bbb_timing_run")
    n = cnt.cpu().numpy()
    assert n[0] == GUARD and n[2] == GUARD, "a word next to nbits_dev was written"
    nbits = int(n[1])
    assert 0 <= nbits <= max_bits
    w = bits.cpu().numpy()
    assert (w[:bits_off] == GUARD).all() and w[-1] == GUARD, "a word next to bits_packed_dev was written"
    got_bits = np.unpackbits(w[bits_off:-1].view(np.uint64).view(np.uint8), bitorder="little")
    assert not got_bits[nbits:].any(), "the bits from nbits on are not 0"
    s = sv.cpu().numpy()
    assert (s[:soft_off] == SOFT_FILL).all() and (s[soft_off + nbits:] == SOFT_FILL).all(), "a value next to the nbits soft values was written"
    p = ph.cpu().numpy()
    assert p[0] == 0xEE and p[-1] == 0xEE, "a byte next to phase_dev was written"
    sw = st.cpu().numpy()
    assert sw[0] == GUARD and sw[3] == GUARD, "a word next to state_dev was written"
    tw = stats.cpu().numpy()
    assert tw[0] == GUARD and tw[5] == GUARD, "a word next to stats_dev was written"
    return dict(bits=got_bits[:nbits], soft=s[soft_off:soft_off + nbits], phases=p[1:-1], state=tuple(int(v) for v in sw[1:3].view(np.uint64)),
                stats=(tw[1:5] - STATS0).tolist(), nbits=nbits)


def _same(got, want, what=""):
    assert got["nbits"] == want["nbits"], f"{what}: nbits {got['nbits']} != {want['nbits']}"
    assert np.array_equal(got["phases"], want["phases"]), f"{what}: phases differ, the first at block {np.flatnonzero(got['phases'] != want['phases'])[:1]}"
    bad = np.flatnonzero(got["bits"] != want["bits"])
    assert len(bad) == 0, f"{what}: {len(bad)} bits differ, the first at {bad[0]} of {want['nbits']}"
    assert np.array_equal(got["soft"], want["soft"]), f"{what}: soft values differ"
    assert got["state"] == want["state"], f"{what}: state {got['state']} != {want['state']}"
    assert got["stats"] == want["stats"], f"{what}: stats {got['stats']} != {want['stats']}"


def _check(x, nb, P, taps=(1,), L=64, h=4, threshold=0, strict=False, init=M.ACQUIRE, chunks=(0,), state=(0, 0), final=True, shift=0,
           soft=np.int16, what="", **off):
    """The call, once per chunk_blocks, against the model; returns the model's dict."""
    x = np.asarray(x)
    want = M.run(x[nb:], P, taps, L, h, threshold, strict, init, before=x[:nb], state=state, final=final, shift=shift, out_bytes=np.dtype(soft).itemsize)
    for chunk in chunks:
        got = _call(x, nb, P, taps, L, h, threshold, strict, init, chunk, state, final, shift, soft, **off)
        _same(got, want, f"{what} chunk_blocks {chunk}")
    return want


SHAPES = [(P, L) for P in (3, 4, 8, 16, 255, 256) for L in (8, 64, 1024) if L * P <= 65536]


@pytest.mark.parametrize("P,L", SHAPES)
def test_every_shape_and_length(gpu, P, L):
    """Record lengths 1, L P - 1, L P, L P + 1, 37 blocks and a ragged tail, 400 blocks; 1, 7 and 33 taps; chunk_blocks 1, 3 and the
    default, so that chunk boundaries fall everywhere; thresholds off zero, both strict values, both soft forms, history
    shorter than, equal to and beyond the taps.  The data are noise whose loudest phase drifts through both wraps."""
    k = SHAPES.index((P, L))
    rng = np.random.default_rng(100 + k)
    LP = L * P
    for i, n in enumerate((1, LP - 1, LP, LP + 1)):
        ntaps = (1, 7, 33)[(k + i) % 3]
        nb = (0, ntaps - 1, ntaps, ntaps + 5)[i]
        x = np.concatenate([rng.integers(-900, 900, nb), M.drift_record(rng, P, L, n)])
        _check(x, nb, P, M.phase_taps(rng, ntaps, P), L, 3, int(rng.integers(-40, 40)), bool(i & 1), (M.ACQUIRE, 0, P - 1, M.ACQUIRE)[i], (1, 3, 0),
               final=True, shift=i, soft=(np.int16, np.int32)[i & 1], what=f"n {n}", in_off=1 + 2 * i, bits_off=1 + 2 * (i & 1), soft_off=1 + i)
    for nblocks, tail, ntaps in ((37, LP // 3 + 1, (7, 33, 1)[k % 3]), (400, 0, (33, 1, 7)[k % 3])):
        n = nblocks * LP + tail
        nb = ntaps + 3
        x = np.concatenate([rng.integers(-900, 900, nb), M.drift_record(rng, P, L, n)])
        want = _check(x, nb, P, M.phase_taps(rng, ntaps, P), L, 4, int(rng.integers(-40, 40)), bool(k & 1), M.ACQUIRE, (1, 3, 0), shift=2,
                      soft=(np.int32, np.int16)[k & 1], what=f"{nblocks} blocks", in_off=3)
        print(P, L, nblocks, "stats", want["stats"], "nbits", want["nbits"])
        assert want["stats"][0] == nblocks + (tail > 0) and want["stats"][2] >= 1 and want["stats"][3] >= 1, "the record does not wrap both ways"


@pytest.mark.parametrize("P", (4, 255, 256))
def test_ramps_move_in_every_block(gpu, P):
    """The loudest phase advances or retreats one phase per block: a move in every block, a wrap every P blocks; entered with
    init_phase P - 1 / 0, so that the wrap comes in block 1 whatever P is."""
    L = 8
    nblocks = 3 * P // 2 + 4 if P < 16 else 300
    total = [0, 0]
    for d, start in ((1, P - 1), (-1, 0)):
        x = M.ramp(P, L, nblocks, d, start)
        want = _check(np.concatenate([[77], x]), 1, P, [1], L, 4, init=start, chunks=(1, 3, 0), what=f"ramp {d}")
        assert want["moves"].tolist() == [0] + [d] * (nblocks - 1)
        assert want["stats"][2 if d > 0 else 3] == 1 + (nblocks - 2) // P and want["stats"][3 if d > 0 else 2] == 0
        total = [total[0] + want["stats"][2], total[1] + want["stats"][3]]
    assert total[0] >= 1 and total[1] >= 1


def test_all_zero_record_never_moves(gpu):
    """Every comparison ties: the arg-max is phase 0, nothing moves, every bit is 0 >= 0."""
    for P, L, strict in ((8, 8, False), (3, 64, True), (256, 8, False)):
        want = _check(np.zeros(L * P * 50 + 5, dtype=np.int64), 0, P, [3, -2, 1], L, 1, strict=strict, chunks=(1, 3, 0), what=f"zeros P {P}")
        assert want["stats"] == [51, 0, 0, 0] and not want["phases"].any() and want["nbits"] == 50 * L + -(-5 // P)
        assert not want["bits"].any() if strict else want["bits"].all()


def test_ties_in_the_decision_rule(gpu):
    """up == cur + margin exactly: no move.  up == dn > cur + margin: up wins.  up == cur + margin and dn above it: down."""
    P, L, h = 4, 8, 2
    def block(levels):                                                        # noqa: E306
        return np.tile(np.array(levels, dtype=np.int64), L) * np.tile(np.repeat([1, -1], P), L // 2)
    # entered at phase 1; cur 16 L = 128, margin 32
    x = np.concatenate([block([1, 9, 1, 1]), block([5, 16, 20, 1]), block([30, 16, 30, 1]), block([1, 25, 16, 20])])
    want = _check(x, 0, P, [1], L, h, init=1, chunks=(1, 0), what="ties")
    assert want["moves"].tolist() == [0, 0, 1, -1] and want["phases"].tolist() == [1, 1, 2, 1]


def test_threshold_and_strict_at_the_decision(gpu):
    """Samples that sit on the threshold: >= takes them as 1, > as 0; the metric is taken about the threshold."""
    rng = np.random.default_rng(5)
    x = rng.integers(-3, 4, 8 * 16 * 60) + 7
    a = _check(x, 0, 8, [1], 16, 4, threshold=7, strict=False, chunks=(3,), what="at the threshold")
    b = _check(x, 0, 8, [1], 16, 4, threshold=7, strict=True, chunks=(3,), what="strict")
    assert np.array_equal(a["phases"], b["phases"]) and (a["soft"] == 7).sum() > 100 and np.array_equal(a["bits"] != b["bits"], a["soft"] == 7)
    assert a["stats"][1] > 0


def test_full_scale_sums_at_the_int64_bound(gpu):
    """Samples of +-32768 against taps of sum |h| = 65535 and a threshold at the end of int32, L 1024: a term reaches 2^32 - 32769,
    a metric 2^42.  The loud phase is the one whose samples are all -32768; it retreats and advances across the wrap."""
    rng = np.random.default_rng(6)
    P, L, taps = 8, 1024, [0] * 17
    taps[0], taps[8], taps[16] = 32767, 32767, 1
    path = [0, 0, 7, 7, 0, 0, 1]
    x = rng.choice([-32768, 32767], (len(path), L, P))
    for j, p in enumerate(path):
        x[j, :, p] = -32768                                                   # a = -32768 * 65535 at every symbol of the loud phase
    want = _check(x.reshape(-1), 0, P, taps, L, 4, threshold=2 ** 31 - 1, init=0, chunks=(1, 0), soft=np.int32, what="full scale")
    a = fir_model.acc(x.reshape(-1), taps)
    assert np.abs(a - (2 ** 31 - 1)).max() == 2 ** 32 - 32769 and np.abs(a[:L * P] - (2 ** 31 - 1))[0::P].sum() > 2 ** 41
    assert want["phases"].tolist() == path and want["stats"][2:] == [1, 1]


def test_wrap_down_in_block_0_reads_the_sample_in_front_of_the_call(gpu):
    """A call entered locked at phase 0 whose first block moves down: its first instant is a(-1), the history's last sample
    through the filter, or 0 where the call was given no history."""
    P, L = 4, 8
    x = np.concatenate([[5, -6, 7, -3000], M.ramp(P, L, 6, -1, 3)])           # the peak of block 0 is at phase 3: down from 0
    for nb in (4, 2, 1, 0):
        want = _check(x[4 - nb:], nb, P, [2, 1, -1], L, 4, init=0, state=(M.LOCKED | 0, 9), chunks=(1, 0), soft=np.int32, what=f"nbefore {nb}")
        first = 2 * x[3] + x[2] - x[1]
        assert want["wraps"][0] == -1 and want["instants"][0] == -1 and want["nbits"] == 6 * L + 2 and want["state"][1] == 9 + want["nbits"]
        assert want["soft"][0] == (first, 2 * x[3] + x[2], 2 * x[3], 0)[(4, 2, 1, 0).index(nb)]
    # the same through two calls: the first leaves the state, init_phase 0 plays no part in the second
    from basebandboard_amd import TimingRecovery
    tr = TimingRecovery(P, [2, 1, -1], L, init_phase=0)
    st = tr.new_state()
    head = np.concatenate([M.ramp(P, L, 1, 1, 0)[:-4], x[:4]])
    xt = torch.from_numpy(np.concatenate([head, x[4:]]).astype(np.int16)).to("cuda:0")
    b1, n1 = tr.slice(xt[:L * P], state=st, final=False)
    b2, n2, soft, ph = tr.recover(xt[L * P - 3:], nbefore=3, state=st, out_dtype=torch.int32)
    one = M.run(xt.cpu().numpy(), P, [2, 1, -1], L, 4, init_phase=0, out_bytes=4)
    assert n1 == L and n2 == one["nbits"] - L and one["wraps"][1] == -1
    assert np.array_equal(soft[:n2].cpu().numpy(), one["soft"][L:]) and ph.cpu().tolist() == one["phases"][1:].tolist()
    assert tuple(int(v) for v in st.cpu().numpy().view(np.uint64)) == one["state"]


@pytest.mark.parametrize("name", sorted(H.MULTIPASS))
def test_more_than_two_passes_of_the_grids(gpu, name):
    """The drifting-noise records of tests/test_timing_host.py, which holds bbb_timing_model_host, the expected values here, to the
    model on three stretches.  small_blocks (8 symbols of 3 samples, the smallest block there is): 2 * 8 * cus + 5 tiles and more
    chunks than that, so the metric, chunk, walk and gather kernels all take a third turn with a prefetched tile, their last pass
    is ragged, and a chain thread owns several chunks.  long_blocks (1024 symbols of 8 samples): 8 * cus + 3 blocks of four tiles,
    two passes of the metric kernel's sums over a block's tiles and five of the gather kernel's."""
    x, taps, P, L, chunk, want = H.multipass_expected(name, grid.cus())
    assert want["stats"][1] > 8 and want["stats"][2] >= 1 and want["stats"][3] >= 1, "the record does not move and wrap both ways"
    got = _call(x, 0, P, taps, L, H.MULTIPASS_H, H.MULTIPASS_THRESHOLD, True, M.ACQUIRE, chunk, shift=H.MULTIPASS_SHIFT, in_off=3)
    _same(got, want, name)


def _unpack(words, n):
    return np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")[:n]


def test_a_capture_cut_at_block_boundaries_equals_one_call(gpu):
    rng = np.random.default_rng(7)
    P, L, taps = 8, 16, M.phase_taps(rng, 19, 8)
    LP = L * P
    n = 300 * LP + 77
    x = M.drift_record(rng, P, L, n).astype(np.int16)
    want = M.run(x, P, taps, L, 3, 11, True, shift=2)
    assert want["stats"][2] >= 1 and want["stats"][3] >= 1
    tr = gpu.TimingRecovery(P, gpu.FIR(taps, shift=2), L, 3, threshold=11, strict=True, chunk_blocks=7)
    xt = torch.from_numpy(x).to("cuda:0")
    cuts = sorted(set((rng.integers(1, 300, 9) * LP).tolist()))
    st = tr.new_state()
    bits, soft, phases = [], [], []
    for lo, hi in zip([0] + cuts, cuts + [n]):
        nb = min(lo, len(taps))
        b, nbits, s, ph = tr.recover(xt[lo - nb:hi], nbefore=nb, state=st, final=hi == n)
        bits.append(_unpack(b, nbits))
        soft.append(s[:nbits].cpu().numpy())
        phases.append(ph.cpu().numpy())
    assert np.array_equal(np.concatenate(bits), want["bits"]) and np.array_equal(np.concatenate(soft), want["soft"])
    assert np.array_equal(np.concatenate(phases), want["phases"])
    assert tuple(int(v) for v in st.cpu().numpy().view(np.uint64)) == want["state"]
    assert tr.stats() == dict(zip(("blocks", "moves", "wraps_up", "wraps_down"), want["stats"]))
    # a call that is not final leaves the ragged tail alone: the guards of _call hold for the shorter outputs
    part = _check(x[:40 * LP + 99], 0, P, taps, L, 3, 11, True, final=False, chunks=(1, 3, 0), shift=2, what="not final")
    assert part["stats"][0] == 40 and part["nconsumed"] == 40 * LP
    assert np.array_equal(part["bits"], want["bits"][:part["nbits"]])
    none = _check(x[:LP - 1], 0, P, taps, L, 3, 11, True, final=False, state=(M.LOCKED | 5, 3), what="no block")
    assert none["nbits"] == 0 and none["state"] == (M.LOCKED | 5, 3)


def test_a_stream_in_chunks_of_any_size_equals_recover(gpu):
    rng = np.random.default_rng(8)
    P, L, taps = 5, 24, M.phase_taps(rng, 12, 5)
    n = 150 * L * P + 31
    x = M.drift_record(rng, P, L, n).astype(np.int16)
    xt = torch.from_numpy(x).to("cuda:0")
    tr = gpu.TimingRecovery(P, taps, L, 3, chunk_blocks=5)
    bits, nbits, soft, phases = tr.recover(xt, out_dtype=torch.int32)
    want = M.run(x, P, taps, L, 3, out_bytes=4)
    assert want["stats"][2] >= 1 and want["stats"][3] >= 1
    assert nbits == want["nbits"] and np.array_equal(_unpack(bits, nbits), want["bits"]) and np.array_equal(soft[:nbits].cpu().numpy(), want["soft"])
    s = tr.stream(torch.int32)
    cuts = sorted(rng.integers(0, n, 14).tolist() + [0, 7, 7, 119, 120, 121])
    got_b, got_s = [], []
    edges = [0] + cuts + [n]
    for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        b, nb, z = s.push(xt[lo:hi], final=i == len(edges) - 2)
        got_b.append(_unpack(b, nb))
        got_s.append(z[:nb].cpu().numpy())
    assert np.array_equal(np.concatenate(got_b), want["bits"]) and np.array_equal(np.concatenate(got_s), want["soft"])
    assert np.array_equal(torch.cat(s.phases).cpu().numpy(), want["phases"])
    assert tuple(int(v) for v in s.state.cpu().numpy().view(np.uint64)) == want["state"]


@pytest.fixture(scope="module")
def loop(oracle):
    x, ref = M.loop_waveform(oracle)
    return {step: M.resample(x, step, M.LOOP["n"]) for step in M.LOOP["steps"]}, ref


@pytest.mark.parametrize("step", M.LOOP["steps"])
def test_closed_loop_counts_equal_the_cpu(gpu, loop, step):
    """The drifting capture of tests/test_timing_host.py: the GPU leaves the model's bits, so its errors and wraps."""
    L = M.LOOP
    y, ref = loop[0][step], loop[1]
    tr = gpu.TimingRecovery(L["P"], block_symbols=L["L"], hysteresis_shift=L["h"])
    yt = torch.from_numpy(y).to("cuda:0")
    words, nbits, soft, phases = tr.recover(yt)
    want = M.run(y, L["P"], L=L["L"], h=L["h"])
    bits = _unpack(words, nbits)
    assert nbits == want["nbits"] and np.array_equal(bits, want["bits"]) and np.array_equal(phases.cpu().numpy(), want["phases"])
    errors, lag = M.loop_errors(bits, ref, M.loop_compare_bits())
    fixed, _ = M.fixed_phase_errors(y, ref)
    st = tr.stats()
    print("step", step, "emitted", nbits, "stats", st, "errors", errors, "at lag", lag, "best fixed phase leaves", fixed)
    assert errors <= M.LOOP_MAX_ERRORS and fixed > M.LOOP_MIN_FIXED_ERRORS
    assert (st["wraps_down"], st["wraps_up"]) == ((M.LOOP_WRAPS, 0) if step > 65536 else (0, M.LOOP_WRAPS))
    assert abs(tr.clock_offset_ppm(phases) - (65536 - step) / 65536 * 1e6) < 15.0
    # RX.count_errors on it: the record from the sample at which data bit 0 is decided, so that decision m is data bit m
    rx = gpu.RX(L["k"], L["P"], 0)
    first = lag * L["P"]
    m = M.run(y[first:], L["P"], L=L["L"], h=L["h"], before=y[first - 1:first])
    model_errors = int((m["bits"] != ref[:m["nbits"]]).sum())
    tr2 = gpu.TimingRecovery(L["P"], block_symbols=L["L"], hysteresis_shift=L["h"])
    assert rx.count_errors(yt, first_sample=first, timing=tr2) == (model_errors, m["nbits"])
    print("count_errors", model_errors, "of", m["nbits"])
    assert model_errors <= M.LOOP_MAX_ERRORS
    assert rx.detect(yt, first_sample=first, timing=tr2)["errors"] == rx.prbsdet.run_stream(*tr2.slice(yt[first - 1:], nbefore=1))["errors"]
    with pytest.raises(ValueError, match="excludes"):
        rx.slice(yt, stride=8, timing=tr2)
    # the soft values, one per symbol, are what a detector at one sample per symbol takes
    d = gpu.DFE([1], [], 1)
    b2, n2 = d.slice(soft[:nbits].contiguous())
    assert n2 == nbits and np.array_equal(_unpack(b2, n2), bits)
