"""The error statistics without a GPU: the numpy model's two forms against each other and against brute force, the binning,
the argument checks of the bbb_errstat_* entry points, and the host arithmetic of ErrorStats.result."""
import ctypes as C

import numpy as np
import pytest

import basebandboard_amd as bbb
from basebandboard_amd import _lib, errstat
from conftest import ROOT
import errstat_model as M

GUARDS = (0, 1, 7, 64, 1000)
BLOCKS = (1, 64, 100, 12000)


def random_stream(rng, n, p):
    if p >= 1:
        return np.arange(n)
    return np.flatnonzero(rng.random(n) < p)


@pytest.mark.parametrize("p", (0, 1e-3, 0.05, 0.5, 1))
def test_model_direct_equals_call_by_call(p):
    rng = np.random.default_rng(int(p * 1e6) + 1)
    n = 20_000 if p < 0.5 else 6_000
    e = random_stream(rng, n, p)
    for guard in GUARDS:
        want = M.direct(e, n, guard, BLOCKS)
        cuts = np.sort(rng.integers(0, n + 1, size=rng.integers(0, 9)))
        w = M.Walk(guard, BLOCKS)
        lo = 0
        for hi in list(cuts) + [n]:
            w.accumulate(e[(e >= lo) & (e < hi)] - lo, hi - lo)
            lo = hi
        assert M.differences(w.result(), want) == [], (p, guard)


def test_model_skip_is_error_free_positions():
    w = M.Walk(3, (100,))
    w.accumulate([5], 64)
    w.skip(1 << 33)
    w.accumulate([0, 2, 7], 64)
    e = [5, 64 + (1 << 33), 66 + (1 << 33), 71 + (1 << 33)]
    assert M.differences(w.result(), M.direct(e, 128 + (1 << 33), 3, (100,))) == []


def test_bin():
    for v, b in ((1, 1), (255, 255), (256, 256), (511, 256), (512, 257), (1 << 63, 311), ((1 << 64) - 1, 311)):
        assert M.vbin(v) == b and errstat.vbin(v) == b
    assert errstat.NBINS == M.NBINS == _lib.ERRSTAT_NBINS == 312
    v = np.array([1, 255, 256, 511, 512, 1023, 1024, (1 << 40) - 1, 1 << 40, (1 << 62) + 5])
    assert M.vbin_np(v).tolist() == [M.vbin(int(x)) for x in v]
    edges = errstat.bin_edges()
    assert len(edges) == 312 and edges.dtype == np.uint64
    for b in range(1, 312):
        assert M.vbin(int(edges[b])) == b and M.vbin(int(edges[b]) - 1) == b - 1
    assert "#define BBB_ERRSTAT_NBINS 312" in (ROOT / "include" / "bbb.h").read_text()


def test_errored_blocks_equal_a_set_count():
    rng = np.random.default_rng(5)
    for p in (1e-3, 0.05, 0.5):
        e = random_stream(rng, 30_000, p) + 77_777
        r = M.direct(e, 200_000, 0, BLOCKS)
        w = M.Walk(0, BLOCKS)
        w.accumulate(e, 200_000)
        for j, B in enumerate(BLOCKS):
            assert r["errored_blocks"][j] == w.result()["errored_blocks"][j] == len({int(t) // B for t in e})


def test_argument_checks():
    lib = _lib.lib()
    o = C.c_void_p()
    good = _lib.ErrstatCfg(7, 2, (C.c_uint64 * 4)(64, 12000, 0, 0))

    def einval(rc, text):
        assert rc == _lib.BBB_EINVAL
        assert text in lib.bbb_last_error_detail().decode(), lib.bbb_last_error_detail()

    einval(lib.bbb_errstat_open(None, 0, None, C.byref(o)), "null cfg")
    einval(lib.bbb_errstat_open(C.byref(good), 0, None, None), "null out")
    einval(lib.bbb_errstat_open(C.byref(_lib.ErrstatCfg(0, 5, (C.c_uint64 * 4)(1, 1, 1, 1))), 0, None, C.byref(o)), "nblock")
    einval(lib.bbb_errstat_open(C.byref(_lib.ErrstatCfg(0, 2, (C.c_uint64 * 4)(1, 1 << 40, 0, 0))), 0, None, C.byref(o)),
           "block_bits[1]")
    einval(lib.bbb_errstat_accumulate(None, C.c_void_p(16), None, 64), "null errstat object")
    einval(lib.bbb_errstat_skip(None, 64), "null errstat object")
    einval(lib.bbb_errstat_read(None, C.byref(_lib.ErrstatResult())), "null errstat object")
    einval(lib.bbb_errstat_reset(None), "null errstat object")
    einval(lib.bbb_errstat_set_stream(None, None), "null errstat object")
    einval(lib.bbb_errstat_close(None), "null errstat object")
    t = C.c_uint64()
    einval(lib.bbb_errstat_geometry(None, C.byref(t)), "null")
    einval(lib.bbb_errstat_geometry(C.byref(t), None), "null")
    assert not o.value
    # an entry beyond nblock is not looked at; the largest block size is 2^40 - 1
    ok = _lib.ErrstatCfg((1 << 32) - 1, 1, (C.c_uint64 * 4)((1 << 40) - 1, 1 << 50, 0, 0))
    import torch
    if not torch.cuda.is_available():
        assert lib.bbb_errstat_open(C.byref(ok), 0, None, C.byref(o)) == _lib.BBB_ENODEV
        assert lib.bbb_errstat_open(C.byref(good), 0, None, C.byref(o)) == _lib.BBB_ENODEV
        with pytest.raises(_lib.BbbError) as e:
            bbb.ErrorStats(guard=3, block_bits=(64,))
        assert e.value.code == _lib.BBB_ENODEV
    with pytest.raises(ValueError, match="block_bits"):
        bbb.ErrorStats(block_bits=(1 << 40,))
    with pytest.raises(ValueError):
        bbb.ErrorStats(block_bits=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError):
        bbb.ErrorStats(guard=1 << 32)


def test_geometry():
    tile, wave = errstat.geometry()
    assert tile % 64 == 0 and wave % 64 == 0 and 0 < wave <= tile and tile % wave == 0


def test_result_arithmetic():
    r = _lib.ErrstatResult()
    r.bits, r.errors, r.first_error, r.last_error, r.max_gap = 1000, 6, 10, 900, 500
    r.bursts, r.burst_len_sum, r.max_burst_len, r.max_burst_weight = 2, 7, 5, 3
    r.open_first, r.open_last, r.open_weight = 600, 900, 2
    r.errored_blocks[0], r.errored_blocks[1] = 5, 4
    r.gap_hist[1], r.gap_hist[3], r.gap_hist[256 + 0] = 1, 2, 2
    r.burst_len_hist[2], r.burst_len_hist[5] = 1, 1
    r.burst_weight_hist[1], r.burst_weight_hist[3] = 1, 1
    d = errstat.summarise(r, (64, 300), close=False)
    assert (d["bursts"], d["burst_len_sum"], d["max_burst_len"], d["max_burst_weight"], d["closed"]) == (2, 7, 5, 3, False)
    assert d["ber"] == 6 / 1000 and d["nblocks"] == [16, 4] and d["errored_blocks"] == [5, 4]
    assert d["errored_block_rate"] == [5 / 16, 1.0]
    assert d["mean_burst_len"] == 3.5 and d["mean_burst_weight"] == 2.0      # 4 of the 6 errors lie in closed bursts
    assert d["gap_hist"].dtype == np.uint64 and int(d["gap_hist"].sum()) == 5
    c = errstat.summarise(r, (64, 300), close=True)
    assert (c["bursts"], c["burst_len_sum"], c["max_burst_len"], c["max_burst_weight"], c["closed"]) == (3, 308, 301, 3, True)
    assert c["burst_len_hist"][M.vbin(301)] == 1 and c["burst_weight_hist"][2] == 1 and int(c["burst_len_hist"].sum()) == 3
    assert c["mean_burst_len"] == 308 / 3 and c["mean_burst_weight"] == 2.0
    assert (c["open_first"], c["open_last"], c["open_weight"]) == (600, 900, 2)
    assert int(d["burst_len_hist"].sum()) == 2                              # the first dict is not touched by the second
    z = errstat.summarise(_lib.ErrstatResult(), (64,), close=True)
    assert z["ber"] == 0.0 and z["nblocks"] == [0] and z["errored_block_rate"] == [0.0] and z["mean_burst_len"] == 0.0
    assert not z["closed"] and z["bursts"] == 0
