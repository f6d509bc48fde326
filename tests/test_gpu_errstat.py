"""The error statistics on the GPU, compared exactly with the numpy model (tests/errstat_model.py): every field of
bbb_errstat_result, at every density, around every boundary of the kernel's geometry, in one call and in pieces, with skips,
masks, ragged ends, two handles and a change of stream."""
import json
import subprocess

import numpy as np
import pytest
import torch

import basebandboard_amd as bbb
from basebandboard_amd import errstat
from conftest import ROOT
import errstat_model as M

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
T, W = errstat.geometry()                          # bits per workgroup (tile) and per wavefront
BLOCKS = (1, 64, 100, 12000)
GUARDS = (0, 1, 7, 64, 1000, T + 1)
NSPARSE = (1 << 22) - 37                           # 16 tiles, the last one ragged
NDENSE = 4 * T + W + 129


def dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).to(DEV)


def gpu_result(words, nbits, guard, blocks=BLOCKS, pieces=None, mask=None):
    """bbb_errstat_result of the stream, fed in one call or in `pieces` (bit counts that add up to nbits)."""
    d, m = dev(words), None if mask is None else dev(mask)
    with bbb.ErrorStats(guard, blocks) as es:
        off = 0
        for n in pieces or [nbits]:
            assert off % 64 == 0
            es.accumulate(d[off // 64:], None if m is None else m[off // 64:], n)
            off += n
        assert off == nbits
        return es.read()


def expect_equal(words, nbits, guard, blocks=BLOCKS, **kw):
    want = M.direct(M.positions(words, nbits, kw.get("mask")), nbits, guard, blocks)
    assert M.differences(gpu_result(words, nbits, guard, blocks, **kw), want) == [], (nbits, guard)


def stream(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("0", "1e-4", "1e-3", "0.05"):
        return M.pack(NSPARSE, np.flatnonzero(rng.random(NSPARSE) < float(name))), NSPARSE
    if name == "0.5":
        return rng.integers(0, 1 << 64, size=(NDENSE + 63) // 64, dtype=np.uint64), NDENSE
    if name == "ones":
        return np.full((NDENSE + 63) // 64, ~np.uint64(0)), NDENSE
    if name == "single":
        return M.pack(NSPARSE, [2 * T + 12345]), NSPARSE
    assert name == "pair"                          # two errors 3 T + 5 apart with nothing between
    return M.pack(NSPARSE, [T - 2, 4 * T + 3]), NSPARSE


@pytest.mark.parametrize("name", ("0", "1e-4", "1e-3", "0.05", "0.5", "ones", "single", "pair"))
def test_streams(name):
    words, nbits = stream(name)
    pos = M.positions(words, nbits)
    d = dev(words)
    for guard in GUARDS:
        with bbb.ErrorStats(guard, BLOCKS) as es:
            es.accumulate(d, None, nbits)
            assert M.differences(es.read(), M.direct(pos, nbits, guard, BLOCKS)) == [], (name, guard)


LANDMARKS = (63, 64, W - 1, W, T - 1, T, 2 * T - 1, 2 * T)


def test_landmark_errors():
    n = 3 * T + 64
    words = M.pack(n, LANDMARKS)
    for guard in GUARDS:
        expect_equal(words, n, guard)
    for k in range(len(LANDMARKS)):                # ... and each on its own, and with a neighbour a guard away
        expect_equal(M.pack(n, [LANDMARKS[k]]), n, 7)
        expect_equal(M.pack(n, [LANDMARKS[k], LANDMARKS[k] + 7]), n, 7)
        expect_equal(M.pack(n, [LANDMARKS[k], LANDMARKS[k] + 8]), n, 7)


@pytest.mark.parametrize("guard", GUARDS)
def test_pairs_straddling_landmarks(guard):
    """Two errors exactly guard and guard + 1 apart on either side of a boundary, an earlier error so that the pair closes a
    burst or continues one, and a later one that closes whatever the pair left open."""
    n = 5 * T
    for edge in (64, W, T, 2 * T):
        for d in (guard, guard + 1):
            if d == 0:
                continue
            a = max(edge - (d + 1) // 2, 0)
            b = a + d
            assert a < edge <= b or a == 0
            for before in ((), (a - guard - 1,), (a - max(guard, 1),)):
                if before and before[0] < 0:
                    continue
                pos = sorted(set(before) | {a, b, b + guard + 5})
                expect_equal(M.pack(n, pos), n, guard, blocks=(64, T))


def test_bursts_through_tiles():
    n = 6 * T
    # unbroken through three tiles, densely and with one error per wavefront or less
    for guard, step in ((64, 64), (64, 1), (1000, 1000), (T + 1, W + 1), (T + 1, T)):
        pos = list(range(T - 5, 4 * T + 6, step)) + [5 * T + 2 * guard, 5 * T + 2 * guard + 1]
        pos = [p for p in pos if p < n]
        expect_equal(M.pack(n, [3] + pos), n, guard)
    # a tile that holds only the last error of a burst, empty tiles behind it
    expect_equal(M.pack(n, [T - 10, T - 3, T + 2, 5 * T + 9]), n, 7)
    expect_equal(M.pack(n, [T - 10, T - 3, T + 2]), n, 7)
    expect_equal(M.pack(n, [T - 3, T + 2, 5 * T + 9, 5 * T + 10]), n, 7)
    # ... and a wavefront that does
    expect_equal(M.pack(n, [W - 10, W - 3, W + 2, 3 * W + 9]), n, 7)


def test_pieces_equal_one_call():
    sizes = [64, 0, T, 0, 3 * T + 64, 0, T + W + 64 * 5 + 21]
    cuts = np.cumsum(sizes)
    n = int(cuts[-1])
    rng = np.random.default_rng(11)
    pos = set(np.flatnonzero(rng.random(n) < 1e-3).tolist())
    for c in cuts[:-1]:                            # an open burst across every boundary between calls
        pos |= {int(c) - 2, int(c) - 1, int(c), int(c) + 3}
    words = M.pack(n, sorted(pos))
    for guard in (0, 7, 1000):                     # (100 and 12000 divide none of the boundaries: blocks cross them)
        want = M.direct(M.positions(words, n), n, guard, BLOCKS)
        assert M.differences(gpu_result(words, n, guard), want) == []
        assert M.differences(gpu_result(words, n, guard, pieces=sizes), want) == []
        walk = M.Walk(guard, BLOCKS)               # the model's own call-by-call form
        e = M.positions(words, n)
        lo = 0
        for s in sizes:
            walk.accumulate(e[(e >= lo) & (e < lo + s)] - lo, s)
            lo += s
        assert M.differences(walk.result(), want) == []


def test_ragged_end_and_reset():
    n = T + 3 * 64 + 17
    rng = np.random.default_rng(12)
    pos = np.flatnonzero(rng.random(n) < 2e-3)
    pos = np.union1d(pos, [n - 1, n - 18, T + 3 * 64])
    words = M.pack(n, pos)
    words[-1] |= ~np.uint64(0) << np.uint64(17)    # beyond nbits: ones, ignored
    mask = np.zeros_like(words)
    d, m = dev(words), dev(mask)
    want = M.direct(pos, n, 7, BLOCKS)
    with bbb.ErrorStats(7, BLOCKS) as es:
        es.accumulate(d, None, n)
        assert M.differences(es.read(), want) == []
        with pytest.raises(ValueError, match="reset"):
            es.accumulate(d, None, 64)
        with pytest.raises(ValueError, match="reset"):
            es.skip(64)
        assert M.differences(es.read(), want) == []
        es.reset()
        es.accumulate(d, m, n)                     # as new, and the same with a mask of zeros
        assert M.differences(es.read(), want) == []
        es.reset()
        es.skip(5)                                 # a ragged skip ends the record too
        with pytest.raises(ValueError, match="reset"):
            es.accumulate(d, None, 64)
        es.reset()
        es.accumulate(d, None, 0)                  # nothing
        assert M.differences(es.read(), M.direct([], 0, 7, BLOCKS)) == []


def test_skip():
    a, b = dev(M.pack(64, [5])), dev(M.pack(128, [9, 70]))
    big = 1 << 33
    with bbb.ErrorStats(7, (64, 1 << 20)) as es:
        es.accumulate(a, None, 64)
        es.skip(big)
        es.accumulate(b, None, 128)
        r = es.read()
        want = M.direct([5, 64 + big + 9, 64 + big + 70], 192 + big, 7, (64, 1 << 20))
        assert M.differences(r, want) == []
        assert r.max_gap == big + 68 and r.gap_hist[M.vbin(big + 68)] == 1 and r.last_error == big + 134
    # inside an open burst: a small guard closes it at the next error, a large one keeps it open
    for guard in (7, 1000):
        with bbb.ErrorStats(guard, BLOCKS) as es:
            es.accumulate(dev(M.pack(64, [50, 60])), None, 64)
            es.skip(64)
            es.accumulate(dev(M.pack(64, [1])), None, 64)
            es.skip(T + 64)
            es.accumulate(dev(M.pack(64, [2])), None, 64)
            e = [50, 60, 129, 192 + T + 64 + 2]
            assert M.differences(es.read(), M.direct(e, 5 * 64 + T, guard, BLOCKS)) == [], guard
    blocks = (1 << 39, (1 << 40) - 1, 3)
    with bbb.ErrorStats(0, blocks) as es:
        es.accumulate(dev(M.pack(64, [63])), None, 64)
        es.skip((1 << 39) - 64)
        es.accumulate(dev(M.pack(64, [0])), None, 64)
        es.skip(1 << 40)
        es.accumulate(dev(M.pack(64, [0, 1])), None, 64)
        e = [63, 1 << 39, (1 << 39) + 64 + (1 << 40), (1 << 39) + 64 + (1 << 40) + 1]
        want = M.direct(e, (1 << 39) + (1 << 40) + 128, 0, blocks)
        assert want["errored_blocks"] == [3, 2, 3]
        assert M.differences(es.read(), want) == []


@pytest.mark.parametrize("k", (7, 31))
def test_detector_stream_with_reload_mask(k):
    n = (1 << 20) + 4 * 64 + 13
    buf = bbb.PRBS(k, device=0).generate(n).cpu().numpy().view(np.uint64).copy()
    rng = np.random.default_rng(k)
    flips = set(rng.integers(3000, n, size=40).tolist())
    flips |= set(range(T + 500, T + 500 + 3 * k))                # a burst long enough to force a resync (prbs.py:136)
    for f in flips:
        buf[f // 64] ^= np.uint64(1) << np.uint64(f % 64)
    det = bbb.PRBSErrorDetector(k, device=0)
    d = dev(buf)
    with bbb.ErrorStats(2 * k, BLOCKS) as es, bbb.ErrorStats(2 * k, BLOCKS) as raw:
        st = det.run_stream(d, n, want_err=True, want_reload=True, error_stats=es)
        assert st["resyncs"] >= 2 and st["reload_clocks"] > 0
        r = es.read()
        assert r.errors == st["errors"] and r.bits == n
        err, rl = st["err"].cpu().numpy(), st["reload"].cpu().numpy()
        assert M.differences(r, M.direct(M.positions(err, n, rl), n, 2 * k, BLOCKS)) == []
        raw.accumulate(st["err"], None, n)
        rr = raw.read()
        assert rr.errors == st["errors_raw"]
        assert M.differences(rr, M.direct(M.positions(err, n), n, 2 * k, BLOCKS)) == []
        # the keyword alone: the streams are made internally and not returned; the handle goes on counting
        es.reset()
        plain = det.run_stream(d, n - 13)          # a multiple of 64 bits: the record goes on behind it
        st2 = det.run_stream(d, n - 13, error_stats=es)
        assert st2 == plain and "err" not in st2 and "reload" not in st2
        st3 = det.run_stream(d, n, want_err=True, error_stats=es)
        assert "err" in st3 and "reload" not in st3
        assert es.read().errors == st2["errors"] + st3["errors"] and es.result()["bits"] == 2 * n - 13


def test_every_alignment_and_mask_form():
    n = 2 * T + W + 64 * 3 + 5
    rng = np.random.default_rng(13)
    words = M.pack(n + 64, np.flatnonzero(rng.random(n + 64) < 3e-3))
    mask = M.pack(n + 64, np.flatnonzero(rng.random(n + 64) < 0.3))
    d, m = dev(words), dev(mask)
    assert d.data_ptr() % 16 == 0 and m.data_ptr() % 16 == 0
    nw = (n + 63) // 64
    for eo in (0, 1):                              # word offsets: 8 bytes off 16-byte alignment and on it
        for mo in (None, 0, 1):
            with bbb.ErrorStats(64, BLOCKS) as es:
                es.accumulate(d[eo:], None if mo is None else m[mo:], n)
                mw = None if mo is None else mask[mo:mo + nw]
                want = M.direct(M.positions(words[eo:eo + nw], n, mw), n, 64, BLOCKS)
                assert M.differences(es.read(), want) == [], (eo, mo)


def test_two_handles_and_a_change_of_stream():
    n = 3 * T + 64
    rng = np.random.default_rng(14)
    wa = M.pack(n, np.flatnonzero(rng.random(n) < 1e-3))
    wb = M.pack(n, np.flatnonzero(rng.random(n) < 2e-2))
    da, db = dev(wa), dev(wb)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    cut = T + 64
    with bbb.ErrorStats(7, BLOCKS) as ea, bbb.ErrorStats(1000, (100,)) as eb:
        with torch.cuda.stream(s1):
            ea.accumulate(da, None, cut)
        with torch.cuda.stream(s2):
            eb.accumulate(db, None, cut)
            ea.accumulate(da[cut // 64:], None, n - cut)       # the handle moves to another stream between its calls
        with torch.cuda.stream(s1):
            eb.accumulate(db[cut // 64:], None, n - cut)
            rb = eb.read()
        ra = ea.read()
        torch.cuda.synchronize()
        assert M.differences(ra, M.direct(M.positions(wa, n), n, 7, BLOCKS)) == []
        assert M.differences(rb, M.direct(M.positions(wb, n), n, 1000, (100,))) == []


def test_result_closes_the_open_burst_on_the_host():
    n = 512
    with bbb.ErrorStats(7, (100,)) as es:
        es.accumulate(dev(M.pack(n, [10, 12, 500, 505, 509])), None, n)
        o, c = es.result(close=False), es.result()
        assert (o["bursts"], o["open_first"], o["open_last"], o["open_weight"]) == (1, 500, 509, 3)
        assert (c["bursts"], c["burst_len_sum"], c["max_burst_len"], c["max_burst_weight"]) == (2, 13, 10, 3)
        assert c["mean_burst_weight"] == 2.5 and c["nblocks"] == [6] and c["errored_blocks"] == [2] and c["ber"] == 5 / 512
        es.accumulate(dev(M.pack(64, [0])), None, 64)           # the device state was not touched: the burst goes on
        assert es.result(close=False)["open_weight"] == 4


def test_example_prints_the_summary():
    n, k, guard = 1_000_000, 31, 64
    r = subprocess.run([str(ROOT / "examples" / "bbb_mc"), "--errstat", "1", "--bits", str(n), "--prbs", str(k), "--guard", str(guard)],
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    out, = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    flips = sorted(set(range(4096, n, 99991)) | set(range(n // 2, n // 2 + 3 * k)))
    buf = bbb.PRBS(k, device=0).generate(n).cpu().numpy().view(np.uint64).copy()
    for f in flips:
        buf[f // 64] ^= np.uint64(1) << np.uint64(f % 64)
    st = bbb.PRBSErrorDetector(k, device=0).run_stream(dev(buf), n, want_err=True, want_reload=True)
    want = M.direct(M.positions(st["err"].cpu().numpy(), n, st["reload"].cpu().numpy()), n, guard, (1000, 10000, 100000, 1000000))
    assert out["mode"] == "errstat" and out["bits"] == n and out["flipped"] == len(flips)
    assert out["errors"] == want["errors"] == st["errors"] and out["errors_raw"] == st["errors_raw"]
    assert (out["first_error"], out["last_error"], out["max_gap"]) == (want["first_error"], want["last_error"], want["max_gap"])
    assert out["bursts"] == want["bursts"] + 1 and out["errored_blocks"] == want["errored_blocks"]
