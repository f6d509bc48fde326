"""One call of every receive-chain family over a record whose indices pass 2^31 and 2^32, compared everywhere and bit for bit.

The record is a unit of tests/periodic.py tiled on the device; the expected output is the CPU model's output over the unit,
tiled the same way, compared chunk by chunk on the device; tests/test_periodic_host.py asserts, without a GPU, the conditions
under which that comparison sees an index that lost a high bit anywhere in the record.  Every record is the smallest that
carries the family's own item index past the power of two named in its test, plus three periods and a ragged tail.  Outputs,
state words and counters are compared exactly; nothing here has a tolerance."""
import time

import numpy as np
import pytest
import torch

import basebandboard_amd as bbb
from basebandboard_amd import _lib
import errstat_model
import nco_model
import periodic as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
P31, P32 = P.P31, P.P32


@pytest.fixture(autouse=True)
def _timed_and_freed():
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f"wall {time.time() - t0:.2f} s, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    torch.cuda.reset_peak_memory_stats()


def _record(unit, K, tail):
    """K periods of the unit and `tail` items more, on the device."""
    return P.tile(P.to_dev(unit), K * len(unit) + tail)


def _u64(t):
    return tuple(int(v) for v in t.cpu().numpy().view(np.uint64))


# ---- carrier recovery -----------------------------------------------------------------------------------------------------------

def test_carrier_all_outputs_past_2_31_pairs(gpu):
    """2^31 + ... pairs at L = 24, every output: the pair index passes 2^31, the int16 element index of the pairs in and out
    2^32, their byte offset 2^33, the soft values' byte offset 2^32.  (2^32 pairs with all four outputs would hold 40 GiB live;
    the decisions alone go there below.)"""
    r = P.carrier()
    u, p = P.UNITS["carrier"], r["p"]
    K = P.periods_past(P31, p, r["tail"])
    x = _record(r["unit"], K, r["tail"])
    n = x.shape[0]
    assert n > P31 + 3 * p and 2 * n > P32
    cr = bbb.CarrierRecovery(u["L"], u["init_phase"], u["threshold"], u["strict"])
    st = cr.new_state()
    iq, bits, nb, soft, phases = cr.recover(x, state=st)
    assert nb == n and phases.numel() == -(-n // u["L"])
    e = r["expect"]
    P.assert_tiled(iq, e["iq"], what="carrier iq")
    P.assert_tiled(soft, e["soft"], what="carrier soft")
    P.assert_tiled(phases, e["phases"], what="carrier phases")
    assert P.assert_tiled_bits(bits, e["bits"], K, "carrier bits") == n
    assert _u64(st) == r["state"](K)
    assert cr.stats() == dict(zip(("blocks", "flips", "zero_blocks", "phase_steps"), r["stats"](K)))
    del x, iq, bits, soft, phases


def test_carrier_decisions_past_2_32_pairs(gpu):
    """2^32 + ... pairs, the decisions alone: the pair index passes 2^32, the bit index of the decisions with it."""
    r = P.carrier()
    u, p = P.UNITS["carrier"], r["p"]
    K = P.periods_past(P32, p, r["tail"])
    x = _record(r["unit"], K, r["tail"])
    n = x.shape[0]
    assert n > P32 + 3 * p
    cr = bbb.CarrierRecovery(u["L"], u["init_phase"], u["threshold"], u["strict"])
    st = cr.new_state()
    bits, nb = cr.slice(x, state=st)
    assert nb == n
    assert P.assert_tiled_bits(bits, r["expect"]["bits"], K, "carrier bits") == n
    assert _u64(st) == r["state"](K)
    assert cr.stats() == dict(zip(("blocks", "flips", "zero_blocks", "phase_steps"), r["stats"](K)))
    del x, bits


# ---- decision-feedback equalizer -------------------------------------------------------------------------------------------------

def test_dfe_past_2_32_decisions(gpu):
    """spb 1, the smallest the call accepts, nfb 4, the default regions: 2^32 + ... samples, as many decisions and int16 soft
    values.  The sample, decision and soft-value index pass 2^32; there are 2^20 regions."""
    from basebandboard_amd import dfe as D
    r = P.dfe()
    u, p = P.UNITS["dfe"], r["p"]
    g = D.geometry(u["spb"])
    assert (g["region_symbols"], g["warmup_symbols"]) == (u["region"], u["warmup"])
    K = P.periods_past(P32, p, r["tail"])
    x = _record(r["unit"], K, r["tail"])
    n = x.numel()
    assert n > P32 + 3 * p
    eq = bbb.DFE(list(u["taps"]), list(u["fb"]), u["spb"], threshold=u["threshold"])
    st = eq.new_state()
    bits, nb, soft = eq.equalize(x, state=st)
    assert nb == n
    P.assert_tiled(soft, r["expect"]["soft"], what="dfe soft")
    assert P.assert_tiled_bits(bits, r["expect"]["bits"], K, "dfe bits") == n
    assert int(st.item()) == r["state"]
    assert eq.stats() == dict(zip(("regions", "not_proven", "repaired", "symbols"), r["stats"](K)))
    del x, bits, soft


# ---- timing recovery -------------------------------------------------------------------------------------------------------------

def _timing(name, want_soft):
    r = getattr(P, name)()
    u, p = P.UNITS[name], r["p"]
    K = P.periods_past(P32, p, r["tail"])
    x = _record(r["unit"], K, r["tail"])
    assert x.numel() > P32 + 3 * p
    tr = bbb.TimingRecovery(u["P"], block_symbols=u["L"])
    st = tr.new_state()
    e = r["expect"]
    if want_soft:
        bits, nb, soft, phases = tr.recover(x, state=st)
        assert nb == r["nbits"](K)
        P.assert_tiled(soft[:nb], e["soft"], what=name + " soft")
        P.assert_tiled(phases, e["phases"], what=name + " phases")
        del soft, phases
    else:
        bits, nb = tr.slice(x, state=st)
        assert nb == r["nbits"](K)
    assert P.assert_tiled_bits(bits, e["bits"], K, name + " bits") == nb
    assert _u64(st) == r["state"](K)
    assert tr.stats() == dict(zip(("blocks", "moves", "wraps_up", "wraps_down"), r["stats"](K)))
    del x, bits


def test_timing_wraps_both_ways_past_2_32_samples(gpu):
    """P = 4, L = 64: 2^32 + ... samples, 15 wraps up and 10 down in every period of 192 blocks, the decisions alone.  The sample
    index passes 2^32, the decisions' bit index 2^30; a period holds 12283 bits, so the words are unpacked on the device."""
    _timing("timing_wraps", False)


def test_timing_no_net_wrap_with_soft_values_past_2_32_samples(gpu):
    """The same size with ten wraps each way in a period: 12288 bits a period, with the soft values and the phases."""
    _timing("timing_level", True)


# ---- down-converter ----------------------------------------------------------------------------------------------------------------

def _ddc(name, limit, modes):
    r = getattr(P, name)()
    u, p = P.UNITS[name], r["p"]
    K = P.periods_past(limit, p, r["tail"])
    x = _record(r["unit"], K, r["tail"])
    n = x.numel()
    assert n > limit + 3 * p
    d = bbb.DDC(u["fcw"], list(u["taps"]), u["decim"], u["phase"], u["shift"], pa0=u["pa0"])
    for key in modes:
        out = d.iq(x) if key == "iq" else d._run(x, 0, 0, _lib.DDC_POLAR, None)
        assert out.shape[0] == r["expect"][key].length(K)
        P.assert_tiled(out, r["expect"][key], what=f"{name} {key}")
        del out
    del x


def test_ddc_decimated_past_2_32_samples(gpu):
    """decim 4, IQ16 and polar: 2^32 + ... samples in (the input sample index passes 2^32, its byte offset 2^33), 2^30 pairs
    out (their byte offset passes 2^32).  fcw * period = 0 mod 2^24: the oscillator has the record's period."""
    _ddc("ddc4", P32, ("iq", "polar"))


def test_ddc_undecimated_past_2_31_samples(gpu):
    """decim 1, IQ16: 2^31 + ... samples in and pairs out, so the int16 element index of the output passes 2^32."""
    _ddc("ddc1", P31, ("iq",))


# ---- convolutional codec -----------------------------------------------------------------------------------------------------------

def _conv(u):
    return bbb.ConvCode(u["K"], u["gens"], u["puncture"])


def test_conv_encode_past_2_32_transmitted_bits(gpu):
    """K = 7 at rate 3/4: 3 * 2^30 + ... input bits, 2^32 + ... transmitted bits, and the state word behind the last step."""
    r = P.conv34()
    u = P.UNITS["conv34"]
    per_out = len(r["encode"].period)
    K = P.periods_past(P32, per_out, r["rx_tail"])
    nbits = K * r["T"] + r["tail"]
    words = P.tile(P.to_dev(P.pack(r["data"])), -(-nbits // 64))
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    tx, ntx = _conv(u).encode(words, nbits, state=st)
    assert int(st.item()) == r["enc_state"] != 0
    assert ntx == r["encode"].length(K) > P32 + 3 * per_out
    assert P.assert_tiled_bits(tx, r["encode"], K, "conv encode") == ntx
    del words, tx


def test_conv_hard_decode_past_2_32_received_bits(gpu):
    """K = 7 at rate 3/4 from packed bits, one in 41 wrong: 2^32 + ... received bits, 3 * 2^30 + ... decisions."""
    r = P.conv34()
    u = P.UNITS["conv34"]
    per_in = len(r["rx_unit"])
    K = P.periods_past(P32, per_in, r["rx_tail"])
    nin = K * per_in + r["rx_tail"]
    assert nin > P32 + 3 * per_in
    words = P.tile(P.to_dev(P.pack(r["rx_unit"])), -(-nin // 64))
    code = _conv(u)
    bits, nd = code.decode(words, hard=True, nbits=nin)
    assert nd == K * r["T"] + r["tail"]
    assert P.assert_tiled_bits(bits, r["decode"], K, "conv hard decode") == nd
    assert code.stats() == dict(zip(("windows", "steps"), r["stats"](K)))
    del words, bits


def test_conv_soft_decode_past_2_32_values(gpu):
    """K = 3 unpunctured from int16 soft values (the only soft format the call takes): 2^32 + ... values, 2^31 + ... decisions."""
    r = P.conv12()
    u = P.UNITS["conv12"]
    per_in = len(r["unit"])
    K = P.periods_past(P32, per_in, r["rx_tail"])
    x = _record(r["unit"], K, r["rx_tail"])
    assert x.numel() > P32 + 3 * per_in
    code = _conv(u)
    bits, nd = code.decode(x)
    assert nd == K * r["T"] + r["tail"] > P31
    assert P.assert_tiled_bits(bits, r["decode"], K, "conv soft decode") == nd
    assert code.stats() == dict(zip(("windows", "steps"), r["stats"](K)))
    del x, bits


# ---- error statistics ----------------------------------------------------------------------------------------------------------------

def test_errstat_one_accumulate_past_2_32_bits(gpu):
    """One accumulate of 2^32 + ... bits with errors in the first and last words, on both sides of 2^31 and of 2^32 and at 600
    places in between, against errstat_model.direct, which takes positions."""
    n = P32 + 3 * 64 * 1000 + 37
    rng = np.random.default_rng(4)
    near = [-4097, -65, -64, -2, -1, 0, 1, 63, 64, 65, 4096]
    pos = [0, 5, 63, 64, 130] + [P31 + d for d in near] + [P32 + d for d in near] + [n - 101, n - 38, n - 37, n - 2, n - 1]
    pos = np.unique(np.concatenate([pos, rng.integers(0, n, 600), P31 + rng.integers(-5000, 5000, 40), P32 + rng.integers(-5000, 5000, 40)]))
    assert pos[0] == 0 and pos[-1] == n - 1 and (pos < P31).sum() > 100 and (pos > P32).sum() > 20
    w, inv = np.unique(pos // 64, return_inverse=True)
    val = np.zeros(len(w), dtype=np.uint64)
    np.bitwise_or.at(val, inv, np.uint64(1) << (pos % 64).astype(np.uint64))
    err = torch.zeros(-(-n // 64), dtype=torch.int64, device=DEV)
    err[P.to_dev(w)] = P.to_dev(val)
    blocks = (1000, 1 << 20, P31, P32)
    es = bbb.ErrorStats(guard=100, block_bits=blocks)
    es.accumulate(err, nbits=n)
    want = errstat_model.direct(pos, n, 100, blocks)
    assert want["errors"] == len(pos) and want["last_error"] == n - 1 and want["max_gap"] > 1 << 24
    assert errstat_model.differences(es.read(), want) == []
    del err


# ---- capture eye ---------------------------------------------------------------------------------------------------------------------

def test_capture_eye_takes_a_second_launch(gpu):
    """RX.eye of 2^31 + ... int16 samples: the launch loop of the capture eye cuts at 2^31 samples and takes a second turn.  A
    histogram of a tiled record is the same wherever a launch reads it, so the record is two: a unit of values below 0 up to
    sample 2^30 + 12345, a unit of values from 0 on behind it.  A launch that read from the wrong half counts in the wrong rows.
    Both units have a prime length, so every period starts in another column.  Once from a 16-byte aligned pointer, once from
    one 2 bytes on."""
    rng = np.random.default_rng(5)
    pa, pb = 4099, 4093
    A, B = rng.integers(-2048, 0, pa).astype(np.int16), rng.integers(0, 2048, pb).astype(np.int16)
    n, cut, first = P31 + 3 * pa + 1500, (1 << 30) + 12345, 5
    base = torch.empty(n + 1, dtype=torch.int16, device=DEV)
    P.tile(P.to_dev(A), cut, out=base[:cut])
    P.tile(P.to_dev(B), n + 1 - cut, out=base[cut:])
    assert base.data_ptr() % 16 == 0
    rx = bbb.RX(7, 8, 0)
    for off in (0, 1):
        want = P.eye_hist_tiled(np.roll(A, -off), first, cut - off) + P.eye_hist_tiled(B, first + cut - off, n - cut + off)
        assert want.sum() == n and want[128:].sum() == cut - off and want[:128].sum() == n - cut + off
        hist = rx.eye(base[off:off + n], first)
        got = hist.cpu().numpy().view(np.int64)
        bad = np.argwhere(got != want)
        assert len(bad) == 0, f"offset {off}: {len(bad)} bins differ, the first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
    del base


# ---- oscillator ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off_aligned"])
def test_nco_constant_call_takes_a_second_launch(gpu, off):
    """A constant-fm call of 2^30 + ... samples: nco_api.hip cuts such calls at 2^30 samples.  The waveform is a closed form in
    the sample number and repeats after 2^24 samples, so every 2^24 samples are compared with the model's [2^24, 2^25) (the
    first with [0, 2^24): the pipeline fills there); windows on both sides of the cut and the end come from a second object
    through seek as well, and the values around the output stay as they were.  int16 is the only output type the oscillator
    has."""
    n, fcw, am, fm, pm = (1 << 30) + 3 * 4093 + 77, 0x5A5A5B, 40000, -12345, 77
    S = 1 << 24
    base = torch.full((n + 8,), 0x5A5A, dtype=torch.int16, device=DEV)
    out = base[off:off + n]
    o = bbb.NCO(fcw, am, fm, pm)
    x = o.generate(n, out=out)
    assert x.data_ptr() == out.data_ptr() and out.data_ptr() % 16 == 2 * off
    first, later = P.to_dev(nco_model.closed_at(0, S, fcw, fm, am, pm)), P.to_dev(nco_model.closed_at(S, S, fcw, fm, am, pm))
    for a in range(0, n, S):
        b = min(n, a + S)
        P.assert_same(x[a:b], (later if a else first)[:b - a], a, "nco")
    assert (base[:off] == 0x5A5A).all() and (base[off + n:] == 0x5A5A).all()
    assert o.state == o.state_after(n)
    for a in ((1 << 30) - 1000, n - 2000):
        o2 = bbb.NCO(fcw, am, fm, pm)
        o2.seek(a)
        assert torch.equal(o2.generate(2000), x[a:a + 2000]), a
        assert np.array_equal(x[a:a + 2000].cpu().numpy(), nco_model.closed_at(a, 2000, fcw, fm, am, pm)), a
    del base, out, x


# ---- sequence detector -------------------------------------------------------------------------------------------------------------------

def test_mlse_past_2_32_symbols(gpu):
    """The 256-thread kernel with four states, blocks of 8 symbols behind 8 of warm-up and in front of 8 of lookahead, one sample a
    symbol: 2^32 + ... samples and decisions, 2^29 windows.  The sample index and the decisions' bit index pass 2^32."""
    r = P.mlse()
    u, p = P.UNITS["mlse"], r["p"]
    K = P.periods_past(P32, p, r["tail"])
    x = _record(r["unit"], K, r["tail"])
    n = x.numel()
    assert n > P32 + 3 * p
    B, W, D = u["geom"]
    ml = bbb.MLSE(bbb.FIR(list(u["taps"]), shift=u["shift"]), list(u["g"]), u["spb"], init_state=u["init_state"], block_symbols=B,
                  warmup_symbols=W, lookahead_symbols=D)
    bits, nb = ml.slice(x)
    assert nb == n
    assert P.assert_tiled_bits(bits, r["expect"], K, "mlse bits") == n
    assert ml.stats() == dict(zip(("windows", "symbols"), r["stats"](K)))
    del x, bits


# ---- Reed-Solomon --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rs1", "rs2"])
def test_rs_past_2_32_bytes(gpu, name):
    """CCSDS (255, 223) frames at depth 1 (and 2), clean, correctable and failed: so many that the DATA bytes pass 2^32, the coded
    bytes with them, through decode and then through encode.  The status byte of every codeword and the counters are held too."""
    r = getattr(P, name)()
    code = r["code"]
    nf, tf = P.UNITS[name]["frames"], r["tail_frames"]
    K = P.periods_past(P32, nf * code.data_bytes, tf * code.data_bytes)
    frames = K * nf + tf
    assert frames * code.data_bytes > P32 + 3 * nf * code.data_bytes
    rs = bbb.ReedSolomon.ccsds(code.depth)
    recv = P.tile(P.to_dev(r["recv"]), frames * code.frame_bytes)
    data, nerr = rs.decode(recv)
    del recv
    tail = tf * code.data_bytes
    P.assert_tiled(data, r["out"][:0], r["out"], r["out"][:tail], what=name + " decoded bytes")
    P.assert_tiled(nerr, r["nerr"][:0], r["nerr"], r["nerr"][:tf * code.depth], what=name + " status bytes")
    assert rs.stats() == dict(zip(("codewords", "clean", "failed", "symbols_corrected", "bits_corrected"), r["stats"](K)))
    del data, nerr
    src = P.tile(P.to_dev(r["data"]), frames * code.data_bytes)
    coded = rs.encode(src)
    P.assert_tiled(coded, r["coded"][:0], r["coded"], r["coded"][:tf * code.frame_bytes], what=name + " coded bytes")
    del src, coded


# ---- frame synchroniser ----------------------------------------------------------------------------------------------------------------------

def _fs():
    u = P.UNITS["framesync"]
    return bbb.FrameSync(bbb.framesync.CCSDS_MARKER, 32, 32 + 8 * u["payload_bytes"], u["tol_search"], u["tol_lock"], u["verify"],
                         u["flywheel"], True, bbb.framesync.CCSDS_RANDOMIZER)


def _framesync(nbits, and_back):
    r = P.framesync(nbits)
    K, F, nframes = r["K"], r["cfg"].F, r["frames"]
    fs = _fs()
    rec = P.tile(P.to_dev(r["words"]), -(-nbits // 64))
    st = fs.new_state()
    pos, meta, count = fs.find(rec, nbits, state=st)
    assert int(count) == nframes and pos.numel() >= nframes
    for a in range(0, nframes, P.CHUNK):
        b = min(nframes, a + P.CHUNK)
        P.assert_same(pos[a:b], torch.arange(a, b, dtype=torch.int64, device=DEV) * F, a, "framesync positions")
    assert int(pos[nframes - 1]) + F <= nbits < int(pos[nframes - 1]) + 2 * F
    e = r["expect"]
    assert nframes == e.length(K)
    P.assert_tiled(meta[:nframes], e, what="framesync meta words")
    assert _u64(st) == tuple(r["state"])
    assert fs.stats() == dict(zip(bbb.framesync.COUNTERS, r["state"][2:]))
    if and_back:
        # the payloads cut out of the inverted stream, and attached again: the stream as it was sent
        pay = fs.extract(rec, nbits, pos, meta, count)[:nframes * fs.payload_bytes]
        P.assert_tiled(pay, r["payload"][:0], r["payload"], r["payload"][:len(e.tail) * fs.payload_bytes], what="framesync payloads")
        back, nback = fs.attach(pay)
        assert nback == nframes * F
        clean = P.Expect(r["clean"][:0], r["clean"], r["clean"][:nback % r["per"]])
        assert P.assert_tiled_bits(back, clean, nback // r["per"] + 1, "framesync attached bits") == nback
        del pay, back
    del rec, pos, meta


def test_framesync_locked_past_2_32_bits(gpu):
    """Frames of 248 bits locked from bit 0, inverted, 61 a period (15128 bits: a period is no whole words), one marker in 61 so
    wrong that lock rides over it: 2^32 + ... bits through find, the positions (j * 248) and meta words of 17 million frames and
    the state words; then extract (complemented, derandomised) gives the payloads and attach the stream as it was sent.  The
    bit index passes 2^32 in all three."""
    u = P.UNITS["framesync"]
    _framesync(P32 + 3 * P.framesync()["per"] + u["tail_bits"], True)


def test_framesync_at_the_largest_record(gpu):
    """Exactly 2^35 bits, the most bbb_framesync_run accepts: 138 547 332 frames."""
    _framesync(1 << 35, False)


def test_framesync_past_the_largest_record_is_einval(gpu):
    """2^35 + 1 bits: BBB_EINVAL, and nothing written to the positions, the meta words, the state or the scratch (the record is
    there in full all the same)."""
    import ctypes as C
    nbits = (1 << 35) + 1
    fs = _fs()
    rec = torch.zeros(-(-nbits // 64), dtype=torch.int64, device=DEV)
    guard = -0x0123456789ABCDEF
    pos = torch.full((1024,), guard, dtype=torch.int64, device=DEV)
    meta = torch.full((1024,), 0x5A5A, dtype=torch.int16, device=DEV)
    st = torch.full((_lib.FRAMESYNC_NSTATE,), guard, dtype=torch.int64, device=DEV)
    scratch = torch.full((max(1, fs.plan(1 << 35)[0] // 8),), guard, dtype=torch.int64, device=DEV)
    rc = _lib.lib().bbb_framesync_run(C.c_void_p(rec.data_ptr()), nbits, 0, 1, C.byref(fs._cfg()), C.c_void_p(st.data_ptr()),
                                      C.c_void_p(pos.data_ptr()), C.c_void_p(meta.data_ptr()), 1024, C.c_void_p(scratch.data_ptr()), 0,
                                      C.c_void_p(torch.cuda.current_stream(0).cuda_stream))
    assert rc == _lib.BBB_EINVAL and b"2^35" in _lib.lib().bbb_last_error_detail()
    torch.cuda.synchronize()
    assert (pos == guard).all() and (meta == 0x5A5A).all() and (st == guard).all() and (scratch == guard).all()
    del rec, scratch
