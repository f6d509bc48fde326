"""The LDPC codec without a GPU: pins of the convention that do not come from the model (literal base matrices, every encoded word
in the null space of H by a loop written out here, the encoder's image equal to the whole null space of a code small enough to
enumerate), the vectorised model against the literal serial loop, bbb_ldpc_model_host and bbb_ldpc_encode_host against the model
on the grid, the argument checks of bbb_ldpc_decode and bbb_ldpc_encode through the C ABI, the Python argument checks, the stream's
cutting in the model, the kernels' per-check core (basebandboard_amd/csrc/ldpc_common.hpp) called from a restatement of the
kernels' walk on the CPU under ASan/UBSan, the closed loop encode -> noise -> decode, and the arithmetic of the tiled records that
tests/test_gpu_ldpc.py runs on the GPU (more than two passes of the grid; value indices past 2^32)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib
from conftest import ROOT

import ldpc_model as M
import periodic as P

GUARD = 0xA5A5A5A5A5A5A5A5


def _cfg(code):
    c = _lib.LDPCCfg()
    c.Z, c.J, c.K, c.max_iter, c.norm, c.hard_mag = code.Z, code.J, code.K, code.max_iter, code.norm, code.hard_mag
    for j, row in enumerate(code.base):
        for i, v in enumerate(row):
            c.base[j * code.K + i] = v
    return c


def in_buffer(c):
    """The case's buffer as the C ABI takes it: int16 values, or bits packed into u64 words."""
    return M.pack(c["buf"]) if c["hard"] else np.ascontiguousarray(c["buf"], dtype=np.int16)


# ---- pins that do not come from the model -------------------------------------------------------------------------------

def test_pins_of_the_convention():
    assert M.array_base(5, 2, 4) == [[0, 0, 0, 0], [1, 2, -1, 0]]
    assert M.array_base(7, 3, 5) == [[0, 0, 0, 0, 0], [2, 3, -1, 0, 1], [2, 4, -1, -1, 0]]
    assert bbb.LDPC.array(5, 2, 4).base == M.array_base(5, 2, 4) and bbb.LDPC.array(7, 3, 5).base == M.array_base(7, 3, 5)
    c = bbb.LDPC.array(127, 4, 16)
    assert (c.n, c.k, c.m, c.rate, c.Z) == (2032, 1524, 508, bbb.fec.Fraction(3, 4), 127)
    c = bbb.LDPC.array(31, 3, 6)
    assert (c.n, c.k, c.m) == (186, 93, 93)
    # one check by hand: array(5, 2, 4), check 5 + 3 (row 1, r = 3) involves variables 0 * 5 + (3 + 1) % 5, 5 + (3 + 2) % 5, 15 + 3
    code = M.array(5, 2, 4)
    assert code.var[1][:, 3].tolist() == [4, 5, 18]


def _encode_host(code, data, ncw):
    lib = _lib.lib()
    nw = (ncw * code.n + 63) // 64
    out = np.full(nw + 4, GUARD, dtype=np.uint64)
    src = M.pack(data)
    assert lib.bbb_ldpc_encode_host(C.c_void_p(src.ctypes.data), ncw, C.byref(_cfg(code)), C.c_void_p(out[2:].ctypes.data)) == 0, lib.bbb_last_error_detail()
    assert (out[:2] == GUARD).all() and (out[2 + nw:] == GUARD).all()
    return out[2:2 + nw]


def test_every_encoded_word_satisfies_every_check():
    rng = np.random.default_rng(50)
    for code in (M.array(5, 2, 4), M.array(7, 3, 5), M.array(31, 3, 6), M.array(127, 4, 16), M.grid_cases()[15]["code"], M.grid_cases()[26]["code"]):
        assert code.triangular
        data = rng.integers(0, 2, 3 * code.k).astype(np.uint8)
        words = _encode_host(code, data, 3)
        x = M.unpack(words, 3 * code.n)
        assert np.array_equal(words, M.pack(M.encode(code, data)))
        assert not M.unpack(words, 64 * len(words))[3 * code.n:].any()               # the unused bits of the last word
        for w in range(3):
            cw = x[w * code.n:(w + 1) * code.n].tolist()
            assert cw[:code.k] == data[w * code.k:(w + 1) * code.k].tolist()        # systematic, data first
            for j in range(code.J):
                for r in range(code.Z):
                    s = 0
                    for c in range(code.K):
                        if code.base[j][c] >= 0:
                            s ^= cw[c * code.Z + (r + code.base[j][c]) % code.Z]
                    assert s == 0, (code.Z, w, j, r)


def test_the_encoders_image_is_the_null_space():
    """array(5, 2, 4): k = 10, n = 20.  All 2^20 words against H written out; the 2^10 encoded words are exactly those in its
    null space."""
    code = M.array(5, 2, 4)
    H = np.zeros((code.m, code.n), dtype=np.uint8)
    for j in range(code.J):
        for r in range(code.Z):
            for c in range(code.K):
                if code.base[j][c] >= 0:
                    H[j * code.Z + r, c * code.Z + (r + code.base[j][c]) % code.Z] ^= 1
    allw = ((np.arange(1 << code.n)[:, None] >> np.arange(code.n)) & 1).astype(np.uint8)
    null = np.flatnonzero(((allw @ H.T) & 1).sum(axis=1) == 0)
    data = ((np.arange(1 << code.k)[:, None] >> np.arange(code.k)) & 1).astype(np.uint8).reshape(-1)
    coded = M.unpack(_encode_host(code, data, 1 << code.k), (1 << code.k) * code.n).reshape(-1, code.n)
    image = np.sort((coded.astype(np.int64) << np.arange(code.n)).sum(axis=1))
    assert len(null) == 1 << code.k and np.array_equal(image, null)


# ---- the vectorised model against the literal loop ------------------------------------------------------------------------

def test_vectorised_model_equals_the_serial_loop():
    small = [c for c in M.grid_cases() if c["code"].n <= 1024]
    assert len(small) >= 15
    for i, c in enumerate(small):
        out, iters, stats = M.decode_serial(c["code"], c["values"], c["hard"])
        assert np.array_equal(out, c["out"]) and np.array_equal(iters, c["iters"]) and stats == c["stats"], i


def test_the_grid_covers_its_list():
    cs = M.grid_cases()
    assert 24 <= len(cs) <= 48 and all(3 <= c["ncw"] <= 9 for c in cs)
    codes = [c["code"] for c in cs]
    assert {2, 31, 63, 64, 65, 127, 511, 512} <= {c.Z for c in codes}
    assert 1 in {c.J for c in codes} and 64 in {c.K for c in codes} and 16384 in {c.n for c in codes} and 8192 in {c.m for c in codes}
    degs = {len(e) for c in codes for e in c.edges}
    assert {2, 32} <= degs
    assert any(0 in [s for e in c.edges for _, s in e] and c.Z - 1 in [s for e in c.edges for _, s in e] for c in codes)
    assert any(c["in_first"] % 2 == 1 for c in cs) and any(c["in_first"] % 8 for c in cs if not c["hard"])
    assert any(c["hard"] and c["in_first"] % 64 and (c["in_first"] % 64 + c["code"].n) > 64 for c in cs)
    assert {1, 64} <= {c.max_iter for c in codes} and {1, 16} <= {c.norm for c in codes}
    assert any(not c.triangular for c in codes)
    seen = set()
    for c in cs:
        seen |= set(c["iters"].tolist())
        for kind, it, w in zip(c["kinds"], c["iters"].tolist(), range(c["ncw"])):
            if kind == "zero":
                assert it == 0 and not c["out"][w * c["code"].k:(w + 1) * c["code"].k].any()
            if kind == "clean":
                assert it == 0
    assert {0, 1, 2, 3, M.FAILED} <= seen
    # a group in which one codeword converges at once and its neighbour fails: array(31, 3, 6) takes eight at a time
    assert cs[8]["iters"].tolist()[:4] == [0, 255, 0, 255]
    assert any(c["values"].max() == 32767 and c["values"].min() == -32768 for c in cs if not c["hard"])


# ---- the host entry points against the model ----------------------------------------------------------------------------------

def _model_host(code, buf, in_first, ncw, hard, want_iters=True, want_stats=True, stats0=(0, 0, 0, 0, 0)):
    lib = _lib.lib()
    nw = (ncw * code.k + 63) // 64
    src = np.ascontiguousarray(buf)
    bits = np.full(nw + 4, GUARD, dtype=np.uint64)
    iters = np.full(ncw + 32, 0xA5, dtype=np.uint8)
    stats = np.array(list(stats0) + [GUARD], dtype=np.uint64)
    rc = lib.bbb_ldpc_model_host(C.c_void_p(src.ctypes.data), in_first, ncw, M.HARD if hard else M.SOFT16, C.byref(_cfg(code)),
                                 C.c_void_p(bits[2:].ctypes.data), C.c_void_p(iters[16:].ctypes.data) if want_iters else None,
                                 C.c_void_p(stats.ctypes.data) if want_stats else None)
    assert rc == 0, lib.bbb_last_error_detail()
    assert (bits[:2] == GUARD).all() and (bits[2 + nw:] == GUARD).all() and (iters[:16] == 0xA5).all() and (iters[16 + ncw:] == 0xA5).all()
    assert stats[5] == GUARD
    if not want_iters:
        assert (iters == 0xA5).all()
    return bits[2:2 + nw], iters[16:16 + ncw], stats[:5].tolist()


def test_host_entry_points_equal_the_model_on_the_grid():
    for i, c in enumerate(M.grid_cases()):
        code = c["code"]
        if code.triangular:
            assert np.array_equal(_encode_host(code, c["data"], c["ncw"]), M.pack(c["coded"])), i
        bits, iters, stats = _model_host(code, in_buffer(c), c["in_first"], c["ncw"], c["hard"])
        assert np.array_equal(iters, c["iters"]), (i, iters, c["iters"])
        assert np.array_equal(bits, M.pack(c["out"])) and stats == c["stats"], (i, stats, c["stats"])
        # the statistics are added to, and both may be left out
        again = _model_host(code, in_buffer(c), c["in_first"], c["ncw"], c["hard"], want_iters=False, stats0=(5, 4, 3, 2, 1))[2]
        assert again == [a + b for a, b in zip(c["stats"], (5, 4, 3, 2, 1))]
        assert np.array_equal(_model_host(code, in_buffer(c), c["in_first"], c["ncw"], c["hard"], want_stats=False)[0], M.pack(c["out"]))
    lib = _lib.lib()
    g = np.full(8, GUARD, dtype=np.uint64)           # ncodewords = 0 writes nothing
    st = np.full(5, 7, dtype=np.uint64)
    cfg = _cfg(M.array(31, 3, 6))
    assert lib.bbb_ldpc_model_host(None, 0, 0, 0, C.byref(cfg), C.c_void_p(g.ctypes.data), C.c_void_p(g.ctypes.data), C.c_void_p(st.ctypes.data)) == 0
    assert lib.bbb_ldpc_encode_host(None, 0, C.byref(cfg), C.c_void_p(g.ctypes.data)) == 0
    assert (g == GUARD).all() and (st == 7).all()
    nt = [c["code"] for c in M.grid_cases() if not c["code"].triangular][0]
    assert lib.bbb_ldpc_encode_host(None, 0, C.byref(_cfg(nt)), None) == _lib.BBB_EINVAL
    assert b"parity part not triangular" in lib.bbb_last_error_detail()


def test_invalid_arguments_return_before_the_device_is_touched():
    """Every pointer here is a number no device ever gave out: a call that got as far as the device would fail otherwise
    (BBB_ENODEV on a machine without a GPU), and the last cases show that a valid call does get that far."""
    import torch
    lib = _lib.lib()
    IN, BITS, ITERS, STATS = 1 << 20, 1 << 24, 1 << 26, 1 << 28
    NCW = 100                                       # of array(31, 3, 6): 18600 values = 37200 bytes in, 9300 bits = 146 words out

    def dec(cfg, in_dev=IN, in_first=0, ncw=NCW, fmt=0, bits=BITS, iters=ITERS, stats=STATS):
        return lib.bbb_ldpc_decode(C.c_void_p(in_dev), in_first, ncw, fmt, C.byref(cfg) if cfg is not None else None, C.c_void_p(bits),
                                   C.c_void_p(iters) if iters else None, C.c_void_p(stats) if stats else None, 0, None)

    def enc(cfg, data=IN, ncw=NCW, out=BITS):
        return lib.bbb_ldpc_encode(C.c_void_p(data), ncw, C.byref(cfg) if cfg is not None else None, C.c_void_p(out), 0, None)

    def model(cfg):
        return lib.bbb_ldpc_model_host(None, 0, 0, 0, C.byref(cfg) if cfg is not None else None, None, None, None)

    def changed(code=None, base_at=None, **kw):
        c = _cfg(code or M.array(31, 3, 6))
        for k, v in kw.items():
            if k == "reserved":
                c.reserved[1] = v
            else:
                setattr(c, k, v)
        for at, v in (base_at or {}).items():
            c.base[at] = v
        return c

    def flat(Z, J, K, fill=0):
        c = _lib.LDPCCfg()
        c.Z, c.J, c.K, c.max_iter = Z, J, K, 20
        for i in range(J * K):
            c.base[i] = fill
        return c

    good = changed()
    wide = flat(16, 2, 64)                          # 64 entries in a block row
    lone = flat(31, 2, 4)
    for i in (0, 1, 2):                             # row 0 keeps one entry
        lone.base[i] = -1
    nocol = flat(31, 2, 4)
    nocol.base[1] = nocol.base[5] = -1              # column 1 holds nothing
    bad_cfg = [(None, "null"), (changed(Z=1), "Z must"), (changed(Z=513), "Z must"), (flat(31, 0, 4), "J must"), (flat(2, 33, 40), "J must"),
               (flat(31, 3, 3), "K must"), (flat(2, 3, 65), "K must"), (flat(512, 3, 33), "n = K Z"), (flat(512, 17, 20), "m = J Z"),
               (changed(max_iter=0), "max_iter must"), (changed(max_iter=65), "max_iter must"), (changed(norm=17), "norm must"),
               (changed(hard_mag=32768), "hard_mag must"), (changed(reserved=1), "reserved"),
               (changed(base_at={2: 31}), "base entries"), (changed(base_at={7: -2}), "base entries"),
               (wide, "every block row"), (lone, "every block row"), (nocol, "every block column")]
    for cfg, what in bad_cfg:
        for call in (dec, enc, model):
            assert call(cfg) == _lib.BBB_EINVAL, what
            assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    nt = changed(base_at={10: -1})                  # base[1][4]: the diagonal block of row 1 is empty
    assert enc(nt) == _lib.BBB_EINVAL and b"parity part not triangular" in lib.bbb_last_error_detail()
    low = changed(base_at={3 + 12: 5})              # base[2][3]: an entry below the diagonal
    assert enc(low) == _lib.BBB_EINVAL and b"parity part not triangular" in lib.bbb_last_error_detail()
    NB, WB = 2 * 18600, 8 * 146
    bad = [(dec, dict(in_dev=0), "in_dev"), (dec, dict(bits=0), "bits_packed_dev"), (dec, dict(fmt=2), "unknown format"),
           (dec, dict(in_dev=IN + 1), "misaligned input"), (dec, dict(in_dev=IN + 4, fmt=1), "misaligned input"),
           (dec, dict(bits=BITS + 4), "misaligned bits_packed_dev"), (dec, dict(stats=STATS + 4), "misaligned stats_dev"),
           (dec, dict(in_first=(1 << 62) + 1), "in_first"),
           (dec, dict(bits=IN + NB - 8), "bits_packed_dev overlaps the input"), (dec, dict(bits=IN - WB + 8), "bits_packed_dev overlaps the input"),
           (dec, dict(bits=IN + 2 * 7 + NB - 6, in_first=7), "bits_packed_dev overlaps the input"),
           (dec, dict(bits=IN + 8 * 3, in_first=64 * 3 + 63, fmt=1), "bits_packed_dev overlaps the input"),
           (dec, dict(iters=IN + NB - 1), "iters_dev overlaps the input"), (dec, dict(stats=IN + NB - 8), "stats_dev overlaps the input"),
           (dec, dict(iters=BITS + WB - 1), "iters_dev overlaps bits_packed_dev"), (dec, dict(stats=BITS - 32), "stats_dev overlaps bits_packed_dev"),
           (dec, dict(stats=ITERS + 96), "stats_dev overlaps iters_dev"), (dec, dict(ncw=(1 << 40) // 186 + 1), "2\\^40"),
           (dec, dict(ncw=1 << 63), "2\\^40"),
           (enc, dict(data=0), "bits_dev"), (enc, dict(out=0), "out_dev"), (enc, dict(data=IN + 4), "misaligned bits_dev"),
           (enc, dict(out=BITS + 4), "misaligned out_dev"), (enc, dict(out=IN + WB - 8), "out_dev overlaps"),
           (enc, dict(out=IN - 8 * 291 + 8), "out_dev overlaps"), (enc, dict(ncw=(1 << 40) // 186 + 1), "2\\^40")]
    for call, kw, what in bad:
        assert call(good, **kw) == _lib.BBB_EINVAL, what
        assert re.search(what, lib.bbb_last_error_detail().decode()), (what, lib.bbb_last_error_detail())
    if not torch.cuda.is_available():
        # exactly at the bounds, and outputs next to the inputs but not in them: valid
        tri = [c["code"] for c in M.grid_cases() if c["code"].triangular]
        at_bounds = [c for c in tri if c.Z in (2, 512) or c.J in (1, 32) or c.K == 64 or c.n == 16384 or c.m == 8192 or 32 in [len(e) for e in c.edges]]
        assert len(at_bounds) >= 7
        for cfg in [good, changed(max_iter=1), changed(max_iter=64), changed(norm=0), changed(norm=16), changed(hard_mag=0), changed(hard_mag=32767)] \
                + [_cfg(c) for c in at_bounds]:
            assert dec(cfg, ncw=3) == _lib.BBB_ENODEV and enc(cfg, ncw=3) == _lib.BBB_ENODEV
        assert dec(nt) == _lib.BBB_ENODEV                                             # the decoder takes any base matrix
        assert dec(good, bits=IN + NB, iters=IN - 100, stats=IN + NB + WB) == _lib.BBB_ENODEV
        assert dec(good, iters=0, stats=0) == _lib.BBB_ENODEV and dec(good, stats=BITS - 40, iters=BITS + WB) == _lib.BBB_ENODEV
        assert dec(good, in_first=7, bits=IN + 14 + NB + 2) == _lib.BBB_ENODEV and dec(good, in_first=1 << 62, ncw=1) == _lib.BBB_ENODEV
        assert dec(good, ncw=(1 << 40) // 186, bits=1 << 50, iters=1 << 51, stats=1 << 52) == _lib.BBB_ENODEV
        assert enc(good, out=IN + WB) == _lib.BBB_ENODEV and enc(good, out=IN - 8 * 291) == _lib.BBB_ENODEV
        assert dec(good, in_dev=0, bits=0, ncw=0) == _lib.BBB_ENODEV


def test_python_argument_checks():
    with pytest.raises(ValueError, match="odd prime"):
        bbb.LDPC.array(9, 2, 4)
    with pytest.raises(ValueError, match="J < K <= p"):
        bbb.LDPC.array(5, 2, 6)
    with pytest.raises(ValueError, match="Z must"):
        bbb.LDPC([[0, 0]], 1)
    with pytest.raises(ValueError, match="Z must"):
        bbb.LDPC([[0, 0]], 513)
    with pytest.raises(ValueError, match="K must"):
        bbb.LDPC([[0, 0], [0, 0]], 5)
    with pytest.raises(ValueError, match="J x K"):
        bbb.LDPC([[0, 0], [0]], 5)
    with pytest.raises(ValueError, match="base entries"):
        bbb.LDPC([[0, 5]], 5)
    with pytest.raises(ValueError, match="every block row"):
        bbb.LDPC([[0, -1, 1], [-1, -1, 1]], 5)
    with pytest.raises(ValueError, match="every block column"):
        bbb.LDPC([[0, -1, 1], [2, -1, 1]], 5)
    with pytest.raises(ValueError, match="max_iter must"):
        bbb.LDPC.array(5, 2, 4, max_iter=65)
    with pytest.raises(ValueError, match="norm must"):
        bbb.LDPC.array(5, 2, 4, norm=0)
    with pytest.raises(ValueError, match="hard_mag must"):
        bbb.LDPC.array(5, 2, 4, hard_mag=0)
    with pytest.raises(ValueError, match="n = K Z"):
        bbb.LDPC([[0] * 33] * 2, 512)
    c = bbb.LDPC.array(31, 3, 6, max_iter=7, norm=9, hard_mag=5)
    f = c._cfg()
    assert (f.Z, f.J, f.K, f.max_iter, f.norm, f.hard_mag, list(f.reserved)) == (31, 3, 6, 7, 9, 5, [0, 0])
    assert list(f.base[:18]) == sum(M.array_base(31, 3, 6), [])
    assert c.stats() == dict(codewords=0, clean=0, failed=0, iterations=0, bits_corrected=0)
    with pytest.raises(ValueError, match="CUDA tensor"):
        c.decode(np.zeros(186, dtype=np.int16))
    with pytest.raises(ValueError, match="no decode call"):
        c.iterations()
    assert isinstance(c.stream(), bbb.LDPCStream)


def test_stream_equals_one_call_in_the_model():
    rng = np.random.default_rng(54)
    for case in (M.grid_cases()[0], M.grid_cases()[3], M.grid_cases()[15]):
        code, vals = case["code"], case["values"]
        for cuts in ([], [0, 1, 1, len(vals) - 1], sorted(rng.integers(0, len(vals) + 1, 7).tolist())):
            out, iters, left = M.stream(code, vals, cuts)
            assert np.array_equal(out, case["out"]) and np.array_equal(iters, case["iters"]) and left == 0
        out, iters, left = M.stream(code, vals[:-3], [code.n + 1])                  # a record that ends inside a codeword
        assert left == code.n - 3 and np.array_equal(out, case["out"][:-code.k])


# ---- the kernels' core on the CPU, under the sanitizers --------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("ldpc_host")
    exe = d / "ldpc_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", str(ROOT / "tests" / "ldpc_host.cpp"), "-o", str(exe)])
    return exe


def _blob(mode, code, ncw, in_first, fmt, payload, in_off, out_off):
    head = np.array([mode, code.Z, code.J, code.K, code.max_iter, code.norm, code.hard_mag, ncw, in_first, fmt, in_off, out_off], dtype=np.int64)
    base = np.zeros((code.J * code.K + 3) // 4 * 4, dtype=np.int16)
    base[:code.J * code.K] = np.array(code.base, dtype=np.int16).reshape(-1)
    raw = np.ascontiguousarray(payload).tobytes()
    return head.tobytes() + base.tobytes() + raw + bytes(-len(raw) % 8)


def test_check_core_on_the_cpu_equals_the_model(host_exe, tmp_path):
    cases = M.grid_cases()
    offs = (0, 1, 3, 7)
    blobs = [_blob(0, c["code"], c["ncw"], c["in_first"], int(c["hard"]), in_buffer(c), offs[i % 4], offs[(i // 4) % 4]) for i, c in enumerate(cases)]
    enc = [c for c in cases if c["code"].triangular]
    blobs += [_blob(1, c["code"], c["ncw"], 0, 0, M.pack(c["data"]), offs[(i + 1) % 4], offs[(i // 4 + 2) % 4]) for i, c in enumerate(enc)]
    (tmp_path / "c.bin").write_bytes(b"".join(blobs))
    r = subprocess.run([str(host_exe), str(tmp_path / "c.bin"), str(tmp_path / "o.txt")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"cases {len(blobs)}" in r.stdout, (r.returncode, r.stderr[-3000:])
    lines = (tmp_path / "o.txt").read_text().split("\n")
    for i, c in enumerate(cases):
        assert [int(t) for t in lines[3 * i].split()] == c["stats"], (i, lines[3 * i], c["stats"])
        assert bytes.fromhex(lines[3 * i + 1]) == c["iters"].tobytes(), i
        assert bytes.fromhex(lines[3 * i + 2]) == M.pack(c["out"]).tobytes(), i
    for i, c in enumerate(enc, len(cases)):
        assert bytes.fromhex(lines[3 * i + 2]) == M.pack(c["coded"]).tobytes(), i


# ---- the closed loop on the CPU ------------------------------------------------------------------------------------------------

def test_closed_loop_counts():
    """40 codewords of array(127, 4, 16) at +-64 through Gaussian noise (ldpc_model.LOOP): at sigma 32 the decoder takes more than a
    thousand channel errors to none; at sigma 40 it fails on some words and converges on others; from hard decisions at sigma 32
    it leaves more errors than from soft ones."""
    soft, worse, hard = M.loop_counts(32), M.loop_counts(40), M.loop_counts(32, hard=True)
    print(soft, worse, hard)
    assert soft == M.LOOP_COUNTS[(32, False)] and worse == M.LOOP_COUNTS[(40, False)] and hard == M.LOOP_COUNTS[(32, True)]
    assert soft["channel"] > 1000 and soft["failed"] == 0 and soft["data"] == 0
    assert 1 <= worse["failed"] < M.LOOP["ncw"]                                     # the others have iters below 255
    assert hard["data"] > soft["data"]
    # the same through bbb_ldpc_model_host
    code, data, coded, vals = M.loop_record(40)
    bits, iters, stats = _model_host(code, vals, 0, M.LOOP["ncw"], False)
    assert int((M.unpack(bits, len(data)) != data).sum()) == worse["data"] and stats[2] == worse["failed"] and stats[3] == worse["iters"]
    assert (iters == M.FAILED).any() and (iters < M.FAILED).any()


# ---- past one pass of the decoder's grid ---------------------------------------------------------------------------------------
# The decode kernel's workgroups take a group of codewords a turn (eight of array(31, 3, 6)), and the grid is capped at a multiple
# of the compute-unit count (tests/test_gpu_ldpc.py names the factor).  Codewords are independent by definition, so a record of
# more than two passes is a short record's codewords repeated and its expected values are the model's, tiled.

UNIT_KINDS = ("clean", "light", "clean", "clean", "tie", "clean", "clean")


@pytest.fixture(scope="module")
def unit7():
    return M.make_case(M.array(31, 3, 6), np.random.default_rng(55), UNIT_KINDS)


def multipass_codewords(factor, ncus):
    """8 * (2 * factor * ncus + 5) + 3 codewords of array(31, 3, 6): workgroup 0 takes three turns, the last pass is ragged and
    its last group holds three codewords."""
    return 8 * (2 * factor * ncus + 5) + 3


def tile_case(c, ncw):
    """The case c with its codewords repeated up to ncw: (values, out bits, iters, stats), the statistics those of c times the
    whole tiles plus the model's for the codewords of the remainder."""
    code, nu = c["code"], c["ncw"]
    whole, rest = divmod(ncw, nu)

    def rep(a, per):
        a = np.asarray(a).reshape(nu, per)
        return np.concatenate([np.tile(a, (whole, 1)), a[:rest]]).reshape(-1)
    tail = M.decode(code, c["values"][:rest * code.n], c["hard"])[2] if rest else [0] * 5
    return rep(c["values"], code.n), rep(c["out"], code.k), rep(c["iters"], 1), [whole * a + b for a, b in zip(c["stats"], tail)]


def test_tiled_records_equal_the_host_model(unit7):
    """The tiling arithmetic of the multi-pass record, against bbb_ldpc_model_host over the whole tiled record."""
    ncw = multipass_codewords(8, 16)
    assert ncw % 7 and ncw % 8 == 3
    vals, out, iters, stats = tile_case(unit7, ncw)
    bits, its, st = _model_host(unit7["code"], vals, 0, ncw, False)
    assert np.array_equal(bits, M.pack(out)) and np.array_equal(its, iters) and st == stats
    assert stats[0] == ncw and stats[1] == int((iters == 0).sum()) and stats[2] == 0


# ---- the unit of the record whose value indices pass 2^32 ---------------------------------------------------------------------

def wide_unit():
    """Seven codewords of array(31, 3, 6) with different data: five clean, two that need iterations; 1302 values.  The clean
    words' magnitudes are random (a clean word is one whose SIGNS satisfy the checks), so that a shifted read meets different
    values."""
    code = M.array(31, 3, 6)
    rng = np.random.default_rng(56)
    c = M.make_case(code, rng, UNIT_KINDS)
    vals = c["values"].astype(np.int64)
    mags = rng.integers(40, 2000, len(vals))
    vals = np.where(np.repeat(np.array(UNIT_KINDS) == "clean", code.n), np.sign(vals) * mags, vals).astype(np.int16)
    out, iters, stats = M.decode(code, vals)
    return dict(code=code, values=vals, data=c["data"], out=out, iters=iters, stats=stats)


def test_the_wide_unit_meets_the_three_conditions():
    u = wide_unit()
    code = u["code"]
    assert len(u["values"]) == 1302 and P.odd_factor(1302) > 1 and P.odd_factor(7 * code.k) > 1 and P.odd_factor(7) > 1
    assert sorted(u["iters"].tolist())[:5] == [0] * 5 and all(0 < v < M.FAILED for v in sorted(u["iters"].tolist())[5:])
    assert np.array_equal(u["out"], u["data"])
    # 1. codewords are independent: any run of the unit's codewords decodes to the same outputs, the counters are linear
    two = M.decode(code, np.concatenate([u["values"], u["values"], u["values"][:3 * code.n]]))
    assert np.array_equal(two[0], np.concatenate([u["out"], u["out"], u["out"][:3 * code.k]]))
    assert np.array_equal(two[1], np.concatenate([u["iters"], u["iters"], u["iters"][:3]]))
    tail = M.decode(code, u["values"][:3 * code.n])[2]
    assert two[2] == [2 * a + b for a, b in zip(u["stats"], tail)]
    # 2. and 3. no power of two is a multiple of a period, and a shifted read meets different data
    P.assert_shift_shows(u["values"], "ldpc values")
    P.assert_shift_shows(u["out"], "ldpc data bits", group=64)
    P.assert_shift_shows(u["iters"], "ldpc iters", group=8)
