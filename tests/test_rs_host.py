"""The Reed-Solomon codec without a GPU: pins of the convention that do not come from the model, the model against exhaustive
search, bbb_rs_model_host and bbb_rs_encode_host against the model, the argument checks of bbb_rs_decode and bbb_rs_encode
through the C ABI, the Python argument checks, the stream's cutting in the model, the kernels' per-lane core
(basebandboard_amd/csrc/rs_common.hpp) called from a restatement of the kernels' walk on the CPU under ASan/UBSan, and the closed
loop RS encode -> convolutional encode -> noise -> Viterbi -> RS decode."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from conftest import ROOT

import grid
import rs_model as M

GUARD = 0xA5


def _cfg(code):
    c = _lib.RSCfg()
    c.prim_poly, c.fcr, c.prim, c.nroots, c.n, c.depth = code.prim_poly, code.fcr, code.prim, code.nroots, code.n, code.depth
    return c


# ---- pins that do not come from the model -------------------------------------------------------------------------------

def test_pins_of_the_convention():
    qr = M.Code(26, 16)                                                            # 0x11D, fcr 0, prim 1, nroots 10
    assert [qr.log[v] for v in qr.gen] == [0, 251, 67, 46, 61, 118, 70, 64, 94, 32, 45]
    data = [32, 91, 11, 120, 209, 114, 220, 77, 67, 64, 236, 17, 236, 17, 236, 17]
    parity = [196, 35, 39, 119, 235, 215, 231, 226, 93, 23]
    assert M.encode_word(qr, data) == data + parity
    out = np.zeros(26, dtype=np.uint8)
    src = np.array(data, dtype=np.uint8)
    assert _lib.lib().bbb_rs_encode_host(C.c_void_p(src.ctypes.data), 1, C.byref(_cfg(qr)), C.c_void_p(out.ctypes.data)) == 0
    assert out.tolist() == data + parity
    cc = M.ccsds()
    assert cc.gen == cc.gen[::-1] and cc.gen[:6] == [1, 91, 127, 86, 16, 30] and len(cc.gen) == 33
    assert (bbb.ReedSolomon.ccsds(4).n, bbb.ReedSolomon.ccsds(4).k, bbb.ReedSolomon.ccsds(4).fcr, bbb.ReedSolomon.ccsds(2, 239).fcr) == (255, 223, 112, 120)
    assert (bbb.ReedSolomon.dvb().n, bbb.ReedSolomon.dvb().k, bbb.ReedSolomon.dvb().t) == (204, 188, 8)


def _xtime_mul(poly, a, b):
    """a b by shift and xor, written out here."""
    r = 0
    for i in range(8):
        if b >> i & 1:
            r ^= a
        a = (a << 1) ^ (poly if a & 0x80 else 0)
    return r


def test_every_codeword_is_zero_at_the_roots():
    rng = np.random.default_rng(40)
    lib = _lib.lib()
    for code in (M.ccsds(2), M.dvb(), M.Code(26, 16, depth=3), M.Code(40, 36, 0x12B, 1, 11, 8), M.Code(255, 239, 0x187, 120, 11, 1)):
        data = rng.integers(0, 256, 2 * code.data_bytes).astype(np.uint8)
        out = np.zeros(2 * code.frame_bytes, dtype=np.uint8)
        assert lib.bbb_rs_encode_host(C.c_void_p(data.ctypes.data), 2, C.byref(_cfg(code)), C.c_void_p(out.ctypes.data)) == 0
        assert np.array_equal(out, M.encode(code, data))
        for f in range(2):
            fr = out[f * code.frame_bytes:(f + 1) * code.frame_bytes]
            assert np.array_equal(fr[:code.data_bytes], data[f * code.data_bytes:(f + 1) * code.data_bytes])   # systematic, data first
            for c in range(code.depth):
                word = fr[c::code.depth].tolist()
                for i in range(code.nroots):
                    x = 1
                    for _ in range(code.prim * (code.fcr + i)):
                        x = _xtime_mul(code.prim_poly, x, 2)
                    v = 0
                    for sym in word:                                               # symbol 0 is the coefficient of x^(n-1)
                        v = _xtime_mul(code.prim_poly, v, x) ^ sym
                    assert v == 0, (code.n, f, c, i)


# ---- the model against exhaustive search ------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (1, 2))
def test_model_equals_exhaustive_search(k):
    """nroots = 4, t = 2: every codeword of the (5, 1) and (6, 2) codes in a table; for received words at every distance from
    a codeword the model gives the one codeword within 2 symbols, or a failure, exactly as the search over the table says."""
    code = M.Code(4 + k, k, 0x11D, 1, 1)
    rng = np.random.default_rng(42 + k)
    mul = np.array([[code.mul(a, b) for b in range(256)] for a in range(256)], dtype=np.uint8)
    units = [np.array(M.encode_word(code, [int(i == j) for i in range(k)]), dtype=np.uint8) for j in range(k)]
    msgs = np.stack(np.meshgrid(*[np.arange(256)] * k, indexing="ij"), axis=-1).reshape(-1, k)
    book = np.zeros((256 ** k, code.n), dtype=np.uint8)
    for j in range(k):                                                             # the code is linear ...
        book ^= mul[msgs[:, j]][:, units[j]]
    for i in rng.integers(0, len(book), 50):                                       # ... which the encoder confirms
        assert book[i].tolist() == M.encode_word(code, msgs[i].tolist())
    assert np.array_equal(book[:, :k], msgs)
    seen = {0: 0, 1: 0, 2: 0, M.FAILED: 0}
    for dist in range(code.n + 1):
        for _ in range(60):
            recv = book[rng.integers(0, len(book))].copy()
            for s in rng.choice(code.n, dist, replace=False):
                recv[s] ^= rng.integers(1, 256)
            d = (book != recv).sum(axis=1)
            near = np.flatnonzero(d <= code.t)
            assert len(near) <= 1
            word, nerr = M.decode_word(code, recv.tolist())
            if len(near):
                assert word == book[near[0]].tolist() and nerr == d[near[0]], (dist, recv)
            else:
                assert nerr == M.FAILED and word == recv.tolist(), (dist, recv)
            seen[nerr] += 1
    assert all(seen.values()), seen


# ---- the host entry points against the model ----------------------------------------------------------------------------------

def _model_host(code, recv, nframes, want_nerr=True, want_stats=True, stats0=(0, 0, 0, 0, 0)):
    lib = _lib.lib()
    nd, ne = nframes * code.data_bytes, nframes * code.depth
    src = np.ascontiguousarray(recv, dtype=np.uint8)
    data, nerr = np.full(nd + 32, GUARD, dtype=np.uint8), np.full(ne + 32, GUARD, dtype=np.uint8)
    stats = np.array(list(stats0) + [GUARD], dtype=np.uint64)
    rc = lib.bbb_rs_model_host(C.c_void_p(src.ctypes.data), nframes, C.byref(_cfg(code)), C.c_void_p(data[16:].ctypes.data),
                               C.c_void_p(nerr[16:].ctypes.data) if want_nerr else None, C.c_void_p(stats.ctypes.data) if want_stats else None)
    assert rc == 0, lib.bbb_last_error_detail()
    assert (data[:16] == GUARD).all() and (data[16 + nd:] == GUARD).all() and (nerr[:16] == GUARD).all() and (nerr[16 + ne:] == GUARD).all()
    assert stats[5] == GUARD
    if not want_nerr:
        assert (nerr == GUARD).all()
    return data[16:16 + nd], nerr[16:16 + ne], stats[:5].tolist()


def _encode_host(code, data, nframes):
    lib = _lib.lib()
    out = np.full(nframes * code.frame_bytes + 32, GUARD, dtype=np.uint8)
    src = np.ascontiguousarray(data, dtype=np.uint8)
    assert lib.bbb_rs_encode_host(C.c_void_p(src.ctypes.data), nframes, C.byref(_cfg(code)), C.c_void_p(out[16:].ctypes.data)) == 0
    assert (out[:16] == GUARD).all() and (out[16 + nframes * code.frame_bytes:] == GUARD).all()
    return out[16:16 + nframes * code.frame_bytes]


def test_host_entry_points_equal_the_model_on_the_grid():
    seen = set()
    for i, c in enumerate(M.grid_cases()):
        code = c["code"]
        assert np.array_equal(_encode_host(code, c["data"], c["nframes"]), c["coded"]), i
        data, nerr, stats = _model_host(code, c["recv"], c["nframes"])
        assert np.array_equal(nerr, c["nerr"]), (i, code.n, code.nroots, nerr, c["nerr"])
        assert np.array_equal(data, c["out"]) and stats == c["stats"], (i, stats, c["stats"])
        seen |= set(c["nerr"].tolist())
        # the statistics are added to, and both may be left out
        again = _model_host(code, c["recv"], c["nframes"], want_nerr=False, stats0=(5, 4, 3, 2, 1))[2]
        assert again == [a + b for a, b in zip(c["stats"], (5, 4, 3, 2, 1))]
        assert np.array_equal(_model_host(code, c["recv"], c["nframes"], want_stats=False)[0], c["out"])
    assert {0, 1, 2, 8, 16, M.FAILED} <= seen
    two = M.grid_cases()[-1]                        # nroots 2 at n 255, two errors: most words decode to ANOTHER codeword
    assert two["stats"][3] > 32 and np.count_nonzero(two["out"] != two["data"]) > 0
    lib = _lib.lib()
    g = np.full(8, GUARD, dtype=np.uint8)           # nframes = 0 writes nothing
    st = np.full(5, 7, dtype=np.uint64)
    assert lib.bbb_rs_model_host(None, 0, C.byref(_cfg(M.ccsds())), C.c_void_p(g.ctypes.data), C.c_void_p(g.ctypes.data), C.c_void_p(st.ctypes.data)) == 0
    assert lib.bbb_rs_encode_host(None, 0, C.byref(_cfg(M.ccsds())), C.c_void_p(g.ctypes.data)) == 0
    assert (g == GUARD).all() and (st == 7).all()


def test_invalid_arguments_return_before_the_device_is_touched():
    """Every pointer here is a number no device ever gave out: a call that got as far as the device would fail otherwise
    (BBB_ENODEV on a machine without a GPU), and the last cases show that a valid call does get that far."""
    import torch
    lib = _lib.lib()
    IN, DATA, NERR, STATS = 1 << 20, 1 << 24, 1 << 26, 1 << 28
    NF = 10                                         # of (255, 223) at depth 4: 10200 coded, 8920 data bytes, 40 codewords

    def dec(cfg, in_dev=IN, nframes=NF, data=DATA, nerr=NERR, stats=STATS):
        return lib.bbb_rs_decode(C.c_void_p(in_dev), nframes, C.byref(cfg) if cfg is not None else None, C.c_void_p(data),
                                 C.c_void_p(nerr) if nerr else None, C.c_void_p(stats) if stats else None, 0, None)

    def enc(cfg, data=IN, nframes=NF, out=DATA):
        return lib.bbb_rs_encode(C.c_void_p(data), nframes, C.byref(cfg) if cfg is not None else None, C.c_void_p(out), 0, None)

    def model(cfg):
        return lib.bbb_rs_model_host(None, 0, C.byref(cfg) if cfg is not None else None, None, None, None)

    def changed(**kw):
        c = _cfg(M.ccsds(4))
        for k, v in kw.items():
            if k == "reserved":
                c.reserved[1] = v
            else:
                setattr(c, k, v)
        return c

    good = changed()
    bad_cfg = [(None, "null"), (changed(prim_poly=0x1D), "prim_poly must have 9 bits"), (changed(prim_poly=0x21D), "prim_poly must have 9 bits"),
               (changed(prim_poly=0x11B), "not primitive"),                         # the AES polynomial: irreducible, x of order 51
               (changed(prim_poly=0x11C), "not primitive"), (changed(prim_poly=0x101), "not primitive"),
               (changed(fcr=255), "fcr must"), (changed(prim=0), "prim must"), (changed(prim=255), "prim must"),
               (changed(prim=3), "prim must"), (changed(prim=85), "prim must"),
               (changed(nroots=0), "nroots must"), (changed(nroots=3), "nroots must"), (changed(nroots=34), "nroots must"),
               (changed(n=32), "n must"), (changed(n=256), "n must"), (changed(depth=0), "depth must"), (changed(depth=9), "depth must"),
               (changed(reserved=1), "reserved")]
    for cfg, what in bad_cfg:
        for call in (dec, enc, model):
            assert call(cfg) == _lib.BBB_EINVAL, what
            assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    bad = [(dec, dict(in_dev=0), "in_dev"), (dec, dict(data=0), "data_dev"), (dec, dict(stats=STATS + 4), "misaligned stats_dev"),
           (dec, dict(data=IN + 10199), "data_dev overlaps the input"), (dec, dict(data=IN - 8919), "data_dev overlaps the input"),
           (dec, dict(nerr=IN + 10199), "nerr_dev overlaps the input"), (dec, dict(stats=IN + 10192), "stats_dev overlaps the input"),
           (dec, dict(nerr=DATA + 8919), "nerr_dev overlaps data_dev"), (dec, dict(stats=DATA - 32), "stats_dev overlaps data_dev"),
           (dec, dict(stats=NERR + 32), "stats_dev overlaps nerr_dev"), (dec, dict(nframes=(1 << 40) // 1020 + 1), "2\\^40"),
           (dec, dict(nframes=1 << 63), "2\\^40"),
           (enc, dict(data=0), "data_dev"), (enc, dict(out=0), "out_dev"), (enc, dict(out=IN + 8919), "out_dev overlaps"),
           (enc, dict(out=IN - 10199), "out_dev overlaps"), (enc, dict(nframes=(1 << 40) // 1020 + 1), "2\\^40")]
    for call, kw, what in bad:
        assert call(good, **kw) == _lib.BBB_EINVAL, what
        assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    if not torch.cuda.is_available():
        # exactly at the bounds, and outputs next to the inputs but not in them: valid
        for cfg in (good, changed(prim_poly=0x187), changed(fcr=254), changed(prim=254), changed(nroots=2, n=3), changed(nroots=32, n=33),
                    changed(depth=1), changed(depth=8), changed(prim_poly=0x12B)):
            assert dec(cfg) == _lib.BBB_ENODEV and enc(cfg) == _lib.BBB_ENODEV
        assert dec(good, data=IN + 10200, nerr=IN - 40, stats=IN + 10200 + 8920) == _lib.BBB_ENODEV
        assert dec(good, nerr=0, stats=0) == _lib.BBB_ENODEV and dec(good, stats=DATA - 40, nerr=DATA + 8920) == _lib.BBB_ENODEV
        assert dec(good, nframes=(1 << 40) // 1020, data=1 << 50, nerr=1 << 51, stats=1 << 52) == _lib.BBB_ENODEV
        assert enc(good, out=IN + 8920) == _lib.BBB_ENODEV and enc(good, out=IN - 10200) == _lib.BBB_ENODEV
        assert dec(good, in_dev=0, data=0, nframes=0) == _lib.BBB_ENODEV


def test_python_argument_checks():
    with pytest.raises(ValueError, match="n must"):
        bbb.ReedSolomon(256, 223)
    with pytest.raises(ValueError, match="n must"):
        bbb.ReedSolomon(10, 10)
    with pytest.raises(ValueError, match="nroots must"):
        bbb.ReedSolomon(255, 222)
    with pytest.raises(ValueError, match="nroots must"):
        bbb.ReedSolomon(255, 221)
    with pytest.raises(ValueError, match="not primitive"):
        bbb.ReedSolomon(prim_poly=0x11B)
    with pytest.raises(ValueError, match="prim must"):
        bbb.ReedSolomon(prim=5)
    with pytest.raises(ValueError, match="fcr must"):
        bbb.ReedSolomon(fcr=255)
    with pytest.raises(ValueError, match="depth must"):
        bbb.ReedSolomon(depth=9)
    with pytest.raises(ValueError, match="CCSDS"):
        bbb.ReedSolomon.ccsds(1, 200)
    with pytest.raises(ValueError, match="outer must"):
        bbb.Concatenated(bbb.ConvCode(7, (0o171, 0o133)), bbb.ReedSolomon())
    r = bbb.ReedSolomon.ccsds(5)
    c = r._cfg()
    assert (c.prim_poly, c.fcr, c.prim, c.nroots, c.n, c.depth, list(c.reserved)) == (0x187, 112, 11, 32, 255, 5, [0, 0])
    assert (r.t, r.frame_bytes, r.data_bytes) == (16, 1275, 1115)
    assert r.stats() == dict(codewords=0, clean=0, failed=0, symbols_corrected=0, bits_corrected=0)
    with pytest.raises(ValueError, match="CUDA tensor"):
        r.encode(np.zeros(1115, dtype=np.uint8))
    cat = bbb.Concatenated(r, bbb.ConvCode(7, (0o171, 0o133)))
    assert cat.outer is r and cat.inner.K == 7


def test_stream_equals_one_call_in_the_model():
    rng = np.random.default_rng(44)
    for case in (M.grid_cases()[5], M.grid_cases()[20], M.grid_cases()[-1]):
        code, recv = case["code"], case["recv"]
        for cuts in ([], [0, 1, 1, len(recv) - 1], sorted(rng.integers(0, len(recv) + 1, 7).tolist())):
            data, nerr, left = M.stream(code, recv, cuts)
            assert np.array_equal(data, case["out"]) and np.array_equal(nerr, case["nerr"]) and left == 0
        data, nerr, left = M.stream(code, recv[:-3], [code.frame_bytes + 1])       # a record that ends inside a frame
        assert left == code.frame_bytes - 3 and np.array_equal(data, case["out"][:-code.data_bytes])


# ---- the kernels' core on the CPU, under the sanitizers --------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("rs_host")
    exe = d / "rs_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", str(ROOT / "tests" / "rs_host.cpp"), "-o", str(exe)])
    return exe


def _blob(mode, code, nframes, payload, in_off, out_off):
    head = np.array([mode, code.prim_poly, code.fcr, code.prim, code.nroots, code.n, code.depth, nframes, in_off, out_off], dtype=np.int64)
    body = np.zeros((len(payload) + 7) // 8 * 8, dtype=np.uint8)
    body[:len(payload)] = payload
    return head.tobytes() + body.tobytes()


def test_lane_core_on_the_cpu_equals_the_model(host_exe, tmp_path):
    cases = M.grid_cases()
    offs = (0, 1, 3, 15)
    blobs = [_blob(0, c["code"], c["nframes"], c["recv"], offs[i % 4], offs[(i // 4) % 4]) for i, c in enumerate(cases)]
    blobs += [_blob(1, c["code"], c["nframes"], c["data"], offs[(i + 1) % 4], offs[(i // 4 + 2) % 4]) for i, c in enumerate(cases)]
    # records that end inside a workgroup's four frames, and one frame alone
    short = [(c, nf) for c in (cases[3], cases[10], cases[30]) for nf in (1, 2, 3) if nf <= c["nframes"]]
    blobs += [_blob(0, c["code"], nf, c["recv"][:nf * c["code"].frame_bytes], 5, 2) for c, nf in short]
    (tmp_path / "c.bin").write_bytes(b"".join(blobs))
    r = subprocess.run([str(host_exe), str(tmp_path / "c.bin"), str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"cases {len(blobs)}" in r.stdout, (r.returncode, r.stderr[-3000:])
    lines = (tmp_path / "o.txt").read_text().split("\n")
    for i, c in enumerate(cases):
        assert [int(t) for t in lines[3 * i].split()] == c["stats"], (i, lines[3 * i], c["stats"])
        assert bytes.fromhex(lines[3 * i + 1]) == c["nerr"].tobytes(), i
        assert bytes.fromhex(lines[3 * i + 2]) == c["out"].tobytes(), i
    for i, c in enumerate(cases, len(cases)):
        assert bytes.fromhex(lines[3 * i + 2]) == c["coded"].tobytes(), i
    for i, (c, nf) in enumerate(short, 2 * len(cases)):
        code = c["code"]
        assert bytes.fromhex(lines[3 * i + 1]) == c["nerr"][:nf * code.depth].tobytes(), i
        assert bytes.fromhex(lines[3 * i + 2]) == c["out"][:nf * code.data_bytes].tobytes(), i


# ---- the closed loop on the CPU ------------------------------------------------------------------------------------------------

def test_closed_loop_counts():
    """16 frames of CCSDS (255, 223) at depth 4 through (0171, 0133) and noise (rs_model.LOOP), and the same bytes at depth 1:
    the Viterbi decoder leaves fewer errors than the channel made, in bursts; interleaved to depth 4 every codeword is
    corrected, at depth 1 some burst is longer than one codeword takes."""
    deep, flat = M.loop_counts(4), M.loop_counts(1)
    print(deep, flat)
    assert deep == M.LOOP_COUNTS[4] and flat == M.LOOP_COUNTS[1]
    for r in (deep, flat):
        assert r["channel"] > r["viterbi"] > 0
    assert deep["failed"] == 0 and deep["data_bits"] == 0 and 0 < deep["worst"] <= 16
    assert flat["failed"] >= 1


# ---- past one pass of the decoder's grid ---------------------------------------------------------------------------------------
# The decode kernel's workgroups take four frames a turn, at most 16 workgroups per compute unit at a time (tests/grid.py).
# Frames are independent by definition, so a record of more than two passes is a short record's frames repeated and its
# expected values are the model's, tiled.  tests/test_gpu_rs.py runs such records on the GPU.
# Out of reach at this cost: the encoder's grid is capped at 2^16 workgroups of 256 codewords, 2^24 codewords a pass.

def multipass_frames(ncus):
    """4 * (2 * 16 * ncus + 5) + 1 frames: workgroup 0 takes three turns, the last pass is ragged and its last group holds one
    frame."""
    return 4 * grid.passes(grid.RS_DECODE, ncus=ncus) + 1


def tile_case(c, nframes):
    """The case c (tests/rs_model.py, make_case) with its received frames repeated up to nframes: (recv, out, nerr, stats), the
    statistics those of c times the whole tiles plus the model's for the frames of the remainder."""
    code, nf = c["code"], c["nframes"]
    whole, rest = divmod(nframes, nf)

    def rep(a, per):
        a = np.asarray(a).reshape(nf, per)
        return np.concatenate([np.tile(a, (whole, 1)), a[:rest]]).reshape(-1)
    recv, out, nerr = rep(c["recv"], code.frame_bytes), rep(c["out"], code.data_bytes), rep(c["nerr"], code.depth)
    tail = M.decode(code, c["recv"][:rest * code.frame_bytes])[2] if rest else [0] * 5
    return recv, out, nerr, [whole * a + b for a, b in zip(c["stats"], tail)]


@pytest.mark.parametrize("code,ncus", ((M.Code(40, 36, 0x12B, 1, 11, 3), 256), (M.ccsds(4), 8)), ids=("short", "ccsds"))
def test_tiled_records_equal_the_host_model(code, ncus):
    """The tiling arithmetic of the multi-pass records, against bbb_rs_model_host over the whole tiled record."""
    c = M.make_case(code, np.random.default_rng(45), 7, M.PATTERNS)
    nframes = multipass_frames(ncus)
    assert nframes % 7 and nframes % 4 == 1
    recv, out, nerr, stats = tile_case(c, nframes)
    assert len(recv) == nframes * code.frame_bytes and np.array_equal(recv[-code.frame_bytes:], c["recv"][(nframes - 1) % 7 * code.frame_bytes:][:code.frame_bytes])
    data, ne, st = _model_host(code, recv, nframes)
    assert np.array_equal(data, out) and np.array_equal(ne, nerr) and st == stats
    assert stats[0] == nframes * code.depth and stats[1] == int((nerr == 0).sum()) and stats[2] == int((nerr == M.FAILED).sum())
    assert stats[3] == int(nerr[nerr != M.FAILED].sum())
