"""PRBSErrorDetector over one long packed stream, executed in parallel chunks with state hand-off
(bbb_prbs_detector_stream), against the serial restatement of gateware/bbb/prbs.py:61-99.  Every
err / reload bit and every total must be identical, whatever the chunking and however bad the
speculative starts are."""
import time

import numpy as np
import pytest
import torch

from detector_geometry import default_chunk_words, form_of

pytestmark = pytest.mark.gpu

KS = (7, 9, 11, 15, 20, 23, 31)
TOTALS = ("errors", "errors_raw", "reload_clocks", "resyncs")


def corrupt(words, nbits, ber, seed, bursts=()):
    """XOR Bernoulli(ber) errors and the given (start, length) bursts into a packed numpy stream."""
    rng = np.random.default_rng(seed)
    w = words.copy()
    n = int(rng.binomial(nbits, ber))
    pos = np.unique(rng.integers(0, nbits, size=n))
    for a, l in bursts:
        pos = np.union1d(pos, np.arange(a, min(nbits, a + l)))
    pos = pos.astype(np.uint64)
    np.bitwise_xor.at(w, (pos // 64).astype(np.int64), np.uint64(1) << (pos % np.uint64(64)))
    return w


def run_both(gpu, oracle, k, words, nbits, **kw):
    det = gpu.PRBSErrorDetector(k)
    t = torch.from_numpy(words.view(np.int64)).cuda()
    got = det.run_stream(t, nbits, want_err=True, want_reload=True, **kw)
    e, r, st = oracle.prbs_detector_packed(k, words, nbits)
    assert np.array_equal(got["err"].cpu().numpy().view(np.uint64), e)
    assert np.array_equal(got["reload"].cpu().numpy().view(np.uint64), r)
    for name in TOTALS:
        assert got[name] == st[name], name
    assert got["bits"] == nbits
    return got


@pytest.mark.parametrize("k", KS)
def test_clean_stream(gpu, oracle, k):
    """The reference's preamble: after the reload out of reset (k + k//2 clocks; the junk that the half-loaded
    LFSR leaves in the error history can trigger a second one) nothing is flagged."""
    nbits = 300_001
    words = gpu.PRBS(k).generate(nbits, first_bit=5).cpu().numpy().view(np.uint64)
    got = run_both(gpu, oracle, k, words, nbits)
    assert got["errors"] == 0 and 1 <= got["resyncs"] <= 3 and got["chunks_rerun"] == 0


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ber", (1e-4, 2e-2))
def test_reference_test_protocol_at_scale(gpu, oracle, k, ber):
    """prbs.py:124-163 on 2e6 clocks: Bernoulli errors, a 3k burst in the middle (forces a resync), then
    clean; `errors` (err while reload == 0) is what the reference asserts equal to the injected errors."""
    nbits = 2_000_000
    words = gpu.PRBS(k).generate(nbits).cpu().numpy().view(np.uint64)
    bad = corrupt(words, nbits, ber, seed=k, bursts=[(nbits // 2, 3 * k)])
    got = run_both(gpu, oracle, k, bad, nbits)
    assert got["resyncs"] >= 2


@pytest.mark.parametrize("chunk_bits,warm_bits", [(64, 64), (128, 64), (640, 128), (4096, 64), (4096, 1024), (65536, 256),
                                                  (40960, 1024), (57344, 1024), (65536, 1024)])      # (round 5: the fused kernel's longer chunks)
def test_chunking_never_changes_the_result(gpu, oracle, chunk_bits, warm_bits):
    """Short warm-ups make many speculative starts wrong: the verify / re-run passes must repair all of them."""
    k, nbits = 31, 700_003
    words = gpu.PRBS(k).generate(nbits).cpu().numpy().view(np.uint64)
    bad = corrupt(words, nbits, 1e-2, seed=chunk_bits + warm_bits, bursts=[(1000, 200), (350_000, 93), (699_000, 2000)])
    got = run_both(gpu, oracle, k, bad, nbits, chunk_bits=chunk_bits, warm_bits=warm_bits)
    if warm_bits <= 64:
        assert got["chunks_rerun"] > 0


@pytest.mark.parametrize("nbits", (1, 2, 63, 64, 65, 127, 128, 4095, 4096, 4097, 12_345))
def test_ragged_lengths(gpu, oracle, nbits):
    k = 9
    words = gpu.PRBS(k).generate(nbits + 64).cpu().numpy().view(np.uint64)[: (nbits + 63) // 64].copy()
    run_both(gpu, oracle, k, corrupt(words, nbits, 0.01, seed=nbits), nbits, chunk_bits=128, warm_bits=64)


@pytest.mark.parametrize("k", (7, 31))
def test_noise_input_still_exact(gpu, oracle, k):
    """Random bits: the detector resynchronises for ever; the chunked run must still be the serial one."""
    nbits = 400_000
    rng = np.random.default_rng(99 + k)
    words = rng.integers(0, 2**64, size=(nbits + 63) // 64, dtype=np.uint64)
    got = run_both(gpu, oracle, k, words, nbits, chunk_bits=1024, warm_bits=128)
    assert got["resyncs"] > 100


def test_serial_guard_path(gpu, oracle):
    """All-zero input after a PRBS prefix with a one-word warm-up: the result must be exact.  (The name is history: this
    stream never reaches the serial guard, nor even a repair pass -- an all-zero LFSR predicts zeros, so every chunk of the
    zero stretch is flagged clean and starts consistent; chunks_rerun and serial_fallback are 0, asserted here so that the
    docstring cannot drift again.  test_serial_guard_is_reached below is the one that gets there.)"""
    k, nbits = 15, 200_000
    words = gpu.PRBS(k).generate(nbits).cpu().numpy().view(np.uint64).copy()
    words[100:] = 0
    got = run_both(gpu, oracle, k, words, nbits, chunk_bits=64, warm_bits=64)
    print(f"\nzeros after a prefix: chunks={got['chunks']} rerun={got['chunks_rerun']} serial_fallback={got['serial_fallback']}", end="")
    assert got["serial_fallback"] == 0 and got["chunks_rerun"] == 0


@pytest.mark.parametrize("k", (7, 20))
def test_serial_guard_is_reached(gpu, oracle, k):
    """The cheapest stream on which the speculation never settles: a clean prefix (the serial machine locks), then one
    flipped bit every k clocks for ever.  The true machine stays locked -- one error per k clocks is far below the
    threshold -- but every reload of k + k // 2 clocks takes a flipped bit into the LFSR, so no machine started from reset
    inside that stretch ever locks: every speculative start is wrong, every end state computed from one is wrong, a repair
    pass puts right exactly one more chunk, and after 32 passes det_serial_kernel takes over (sparse form for k = 7, dense
    for k = 20)."""
    nbits = 64 * 64 * 40 + 11
    words = gpu.PRBS(k).generate(nbits).cpu().numpy().view(np.uint64).copy()
    pos = np.arange(4096, nbits, k, dtype=np.uint64)
    np.bitwise_xor.at(words, (pos // np.uint64(64)).astype(np.int64), np.uint64(1) << (pos % np.uint64(64)))
    clean = oracle.prbs_detector_packed(k, gpu.PRBS(k).generate(nbits).cpu().numpy().view(np.uint64), nbits)[2]
    st = oracle.prbs_detector_packed(k, words, nbits)[2]
    assert st["resyncs"] == clean["resyncs"] and st["errors"] == len(pos)      # (on the oracle alone: the true machine stays locked)
    got = run_both(gpu, oracle, k, words, nbits, chunk_bits=4096, warm_bits=64)
    print(f"\nk={k}: chunks={got['chunks']} rerun={got['chunks_rerun']} serial_fallback={got['serial_fallback']}", end="")
    assert got["chunks"] == 41 and got["serial_fallback"] == 1


def test_empty_and_errors(gpu):
    det = gpu.PRBSErrorDetector(7)
    t = torch.zeros(4, dtype=torch.int64, device="cuda")
    assert det.run_stream(t, 0)["bits"] == 0
    with pytest.raises(ValueError):
        det.run_stream(t, 10, chunk_bits=100)
    with pytest.raises(ValueError):
        det.run_stream(t, 1000)


def test_full_size_loopback(gpu):
    """1e9 bits of PRBS-31 through generator -> detector: one reload out of reset, no error, all chunks consistent."""
    nbits = 1_000_000_000
    buf = gpu.PRBS(31).generate(nbits)
    got = gpu.PRBSErrorDetector(31).run_stream(buf, nbits)
    assert got["errors"] == 0 and 1 <= got["resyncs"] <= 3 and got["reload_clocks"] >= 31 + 15 and got["chunks_rerun"] == 0
    base = got["resyncs"]
    # one flipped bit far inside: the detector's LFSR runs on its own feedback, so exactly ONE flagged clock
    buf[5_000_000] ^= 1 << 17
    got = gpu.PRBSErrorDetector(31).run_stream(buf, nbits)
    assert got["errors"] == 1 and got["resyncs"] == base


MID_NBITS = 2_120_000_000                 # the shortest round length whose DEFAULT chunk (128 words) takes the fused kernel


# (k = 7, 9, 23: the oracle passes of all six k != 20 together -- 15-19 s each on one core -- cost more than the pass over
# 1e10 bits in test_gpu_prbs.py, which is this check for k = 31; k = 11 and 15 share NH = 2 with 23 and go through the
# fused kernel in test_gpu_detector_forms.py)
@pytest.mark.parametrize("k", (7, 9, 23))
def test_default_geometry_takes_the_fused_kernel_exactly(gpu, oracle, k):
    """One default call (chunk_bits = 0, warm_bits = 0) per k at a length whose default chunk is a fused one -- what a user
    gets at scale: isolated flips around chunk starts and wave regions; totals and err words exact.  The same call on the
    clean stream is timed and printed (not asserted): a k whose classification never set a flag would still be exact, and
    an order of magnitude slower than k = 31."""
    nbits, nw = MID_NBITS, (MID_NBITS + 63) // 64
    cw = default_chunk_words(nbits, torch.cuda.get_device_properties(0).multi_processor_count)
    assert cw == 128 and form_of(k, cw, 1024) == "fused"
    det = gpu.PRBSErrorDetector(k)
    buf = gpu.PRBS(k).generate(nbits)
    clean = det.run_stream(buf, nbits)
    assert clean["errors"] == 0 and clean["chunks_rerun"] == 0 and clean["chunks"] == -(-nw // cw) and clean["serial_fallback"] == 0
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        det.run_stream(buf, nbits)
        ms.append((time.perf_counter() - t0) * 1e3)
    rng = np.random.default_rng(77 + k)
    lm = np.unique(np.concatenate([rng.integers(2, nw // 128 - 1, size=2000) * 128, rng.integers(1, nw // 8192, size=2000) * 8192]))
    wd = lm + rng.integers(-4, 5, size=len(lm))                            # distinct words, more than 100 words apart
    bit = np.where(rng.random(len(lm)) < 0.3, 63, rng.choice((0, 1, 31, 32, 62), size=len(lm)))
    dv = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int64)).cuda()  # noqa: E731
    buf[dv(wd)] ^= torch.ones(len(lm), dtype=torch.int64, device="cuda") << dv(bit)
    words = buf.cpu().numpy().view(np.uint64)
    t0 = time.perf_counter()
    e, r, st = oracle.prbs_detector_packed(k, words, nbits)
    t_oracle = time.perf_counter() - t0
    assert st["errors"] == len(lm) and st["resyncs"] == clean["resyncs"]   # (the oracle alone: every flip flagged once, still locked)
    got = det.run_stream(buf, nbits, want_err=True)
    print(f"\nk={k}: clean default call {min(ms):.3f} ms (host wall, best of 3), chunks={got['chunks']} rerun={got['chunks_rerun']}, "
          f"oracle pass {t_oracle:.1f} s", end="")
    for name in TOTALS:
        assert got[name] == st[name], (name, got[name], st[name])
    assert got["bits"] == nbits and got["chunks"] == -(-nw // cw) and got["serial_fallback"] == 0
    del r
    diff = np.flatnonzero(got["err"].cpu().numpy().view(np.uint64) != e)
    assert len(diff) == 0, f"err differs from the oracle in {len(diff)} words, first word {diff[0]} = chunk {diff[0] // cw} + {diff[0] % cw}"
