"""Every execution form of bbb_prbs_detector_stream, for every k, bit for bit against the oracle's serial machine.

Which form a call takes is decided by its geometry alone (detector_geometry.form_of restates the rule; the host test
test_detector_geometry_host.py holds that restatement to the kernel file): the fused kernel, classification + sparse
kernel, the dense pass in tiles or lane by lane.  One stream per (k, pattern) -- long enough for several blocks of 256
chunks at 1024 words per chunk, with a partial last wave and a partial last word -- goes through every geometry; the
oracle, whose result does not depend on chunking, runs once per stream.

The patterns put their flips where the machinery hands over: bit 63 of a word (the `last` term of the clean predicate),
the words on either side of a chunk start, of a wave's 64-chunk region and of a block of 256 chunks, the first words
of the stream (the `n >= NH + 1` rule), its last 300, and the resync threshold itself across a word boundary.

A flag that is wrongly unset only costs time; a flag that is wrongly set, or read at the wrong index, makes a lane jump
over a word it had to visit.  So every cell also asserts the path it took (chunks, serial_fallback, chunks_rerun), and
prints its re-run count (run with -s)."""
import bisect
import ctypes as C

import numpy as np
import pytest
import torch

from detector_geometry import KS, form_of

pytestmark = pytest.mark.gpu

TOTALS = ("errors", "errors_raw", "reload_clocks", "resyncs")
NBITS = 337 * 1024 * 64 + 37             # 329 full chunks of 1024 words + 8 (> 256 + 64, partial last wave), 37 bits in the last word
NWORDS = (NBITS + 63) // 64
PATTERNS = ("clean", "isolated", "threshold", "storm")
BITS = (0, 1, 31, 32, 62, 63)
GUARD = 0x5AA55AA5C33CC33C

# (chunk words, warm bits)
FUSED = [(128, 1024), (256, 1024), (512, 1024), (640, 1024), (1024, 1024), (128, 64), (1024, 64), (128, 8192), (1024, 8192)]
TWO_KERNEL = [(64, 1024), (192, 1024), (2048, 1024), (512, 16384), (64, 64)]
K20_ONLY = [(24, 1024)]                   # tiles refused by % 16  ((64, 64): tiles refused by the warm-up, in TWO_KERNEL)
# (k, chunk words, warm bits, offset in words of the input view)
CELLS = [(k, cw, wb, 0) for k in KS for cw, wb in FUSED + TWO_KERNEL + (K20_ONLY if k == 20 else [])] + [(k, 64, 1024, 1) for k in KS]


def expected_form(k, cw, wb, off):
    form = form_of(k, cw, wb, aligned16=off % 2 == 0)
    if off == 0 and k != 20:
        assert form == ("fused" if (cw, wb) in FUSED else "two-kernel")
    elif off:
        assert form == "dense-lane"
    else:
        assert form == ("dense-lane" if (cw, wb) in ((24, 1024), (64, 64), (128, 64), (1024, 64)) else "dense-tiled")
    return form


# ---------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------
def landmark_words(rng):
    """Word indices where something hands over, for every geometry of the matrix at once."""
    lm = set(range(9))                                                     # the n >= NH + 1 rule, the reload out of reset
    lm.update(int(x) * 64 for x in rng.choice(np.arange(1, NWORDS // 64), size=300, replace=False))      # chunk starts
    for cw in (128, 640, 1024):
        for step in (64 * cw, 256 * cw):                                   # wave regions, blocks
            for b in range(step, NWORDS, step):
                lm.update((b, b - 128))                                    # ... and where a wave's region starts
    lm.update(range(NWORDS - 300, NWORDS))
    return sorted(lm)


def xor_bits(words, pos):
    pos = np.asarray(sorted(pos), dtype=np.uint64)
    assert len(np.unique(pos)) == len(pos)
    np.bitwise_xor.at(words, (pos // np.uint64(64)).astype(np.int64), np.uint64(1) << (pos % np.uint64(64)))


def lock_clock(ref_clean):
    """The last clock of the clean stream with reload == 1: where the reload out of reset ends."""
    r = ref_clean[1]
    nz = np.flatnonzero(r)
    assert len(nz) and nz[-1] < 4, "the clean stream reloads out of reset and never again"
    return int(nz[-1]) * 64 + int(r[nz[-1]]).bit_length() - 1


def make_isolated(k, words, rng, t_lock):
    """Single flips at landmark words L + d, d = -4 .. 4, at least 4 k clocks apart (the detector stays locked)."""
    cand = [(L + d) for L in landmark_words(rng) for d in range(-4, 5) if 0 <= L + d < NWORDS]
    cand = [cand[i] for i in rng.permutation(len(cand))]
    taken = []
    for wd in cand:
        bit = 63 if rng.random() < 0.3 else int(rng.choice(BITS[:-1]))
        t = wd * 64 + bit
        if t >= NBITS or t <= t_lock + 4 * k:
            continue
        i = bisect.bisect_left(taken, t)
        if (i > 0 and t - taken[i - 1] < 4 * k) or (i < len(taken) and taken[i] - t < 4 * k):
            continue
        taken.insert(i, t)
    assert sum(t % 64 == 63 for t in taken) * 4 >= len(taken) > 1000
    xor_bits(words, taken)
    return dict(flips=len(taken))


def make_threshold(k, words, rng, t_lock):
    """Clusters of k // 2 (no resync) and k // 2 + 1 flips (exactly one) inside one window of k clocks that lies across a
    landmark word boundary at every offset 0 .. k; packed from the window's first clock, or spread to its first and last."""
    bounds, prev = [], -10 ** 9
    for L in landmark_words(rng):
        if L * 64 - k > t_lock + 8 * k and (L - prev) * 64 >= 8 * k and L * 64 + k < NBITS:
            bounds.append(L)
            prev = L
    combos = [(off, m, style) for off in range(k + 1) for m in (k // 2, k // 2 + 1) for style in ("packed", "spread")]
    assert len(bounds) >= 2 * len(combos)
    order = rng.permutation(len(bounds))
    flips, big = [], 0
    for i, bi in enumerate(order):
        off, m, style = combos[i % len(combos)]
        t0 = bounds[bi] * 64 - off                                         # the window: clocks t0 .. t0 + k - 1
        if style == "packed":
            cl = list(range(t0, t0 + m))
        else:
            cl = [t0, t0 + k - 1] + [int(t0 + 1 + x) for x in rng.choice(k - 2, size=m - 2, replace=False)]
        flips += cl
        big += m == k // 2 + 1
    xor_bits(words, flips)
    return dict(flips=len(flips), big=big, clusters=len(bounds))


ZERO_AT = 327680                          # a wave-region boundary at 128, 640 and 1024 words per chunk (40, 8 and 5 regions)


def make_storm(k, words, rng, t_lock):
    """Bernoulli 1e-3; random bursts that start up to a reload's length before a landmark (reload_ctr != 0 at a chunk's
    end); 300 all-zero words across a wave-region boundary; the last 100 bits random."""
    pos = np.unique(rng.integers(0, NBITS, size=int(rng.binomial(NBITS, 1e-3))))
    xor_bits(words, pos)
    lms = [L for L in landmark_words(rng) if L >= 9]
    lms = [L for L in lms if L < NWORDS - 300] + [L for L in lms if L >= NWORDS - 300][::16]
    for L in lms:
        a = L * 64 - int(rng.integers(0, k + k // 2 + 1))
        n = int(rng.integers(3 * k, 201))
        b = min(NBITS, a + n)
        xor_bits(words, [t for t in range(a, b) if rng.random() < 0.5])
    words[ZERO_AT - 150: ZERO_AT + 150] = 0
    xor_bits(words, [t for t in range(NBITS - 100, NBITS) if rng.random() < 0.5])
    return dict(bursts=len(lms))


_host, _streams = {}, {}


def host_stream(gpu, oracle, k, pattern):
    """The (k, pattern) stream and its oracle result (computed once)."""
    key = (k, pattern)
    if key in _host:
        return _host[key]
    clean = gpu.PRBS(k).generate(NBITS).cpu().numpy().view(np.uint64).copy()
    assert len(clean) == NWORDS
    if pattern == "clean":
        words, info = clean, {}
        ref = oracle.prbs_detector_packed(k, words, NBITS)
        assert ref[2]["errors"] == 0
    else:
        ref_clean = host_stream(gpu, oracle, k, "clean")["ref"]
        t_lock = lock_clock(ref_clean)
        rng = np.random.default_rng(1000 * k + PATTERNS.index(pattern))
        words = clean.copy()
        info = {"isolated": make_isolated, "threshold": make_threshold, "storm": make_storm}[pattern](k, words, rng, t_lock)
        ref = oracle.prbs_detector_packed(k, words, NBITS)
        c, s = ref_clean[2], ref[2]
        # the pattern does to the serial machine what it was built to do: checked on the oracle alone, before any comparison
        if pattern == "isolated":
            assert s["resyncs"] == c["resyncs"] and s["reload_clocks"] == c["reload_clocks"]
            assert s["errors_raw"] == c["errors_raw"] + info["flips"] and s["errors"] == c["errors"] + info["flips"]
        elif pattern == "threshold":
            assert s["resyncs"] == c["resyncs"] + info["big"]
            assert s["reload_clocks"] == c["reload_clocks"] + info["big"] * (k + k // 2)
        else:
            assert s["resyncs"] > c["resyncs"] + info["bursts"] // 2
    _host[key] = dict(words=words, ref=ref, info=info)
    return _host[key]


def stream(gpu, oracle, k, pattern):
    """... and both on the device, the input also one word into a larger buffer (8 mod 16 bytes)."""
    key = (k, pattern)
    if key in _streams:
        return _streams[key]
    h = host_stream(gpu, oracle, k, pattern)
    words, ref = h["words"], h["ref"]
    dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()          # noqa: E731
    shifted = torch.zeros(NWORDS + 1, dtype=torch.int64, device="cuda")
    shifted[1:] = dev(words)
    out = dict(words=words, ref=ref, info=h["info"], t=dev(words), t_shifted=shifted, err=dev(ref[0]), reload=dev(ref[1]))
    _streams[key] = out
    return out


def where(i, cw):
    c = i // cw
    return f"word {i} = chunk {c} + {i % cw} (block {c // 256}, wave {c % 256 // 64}, lane {c % 64})"


def same_words(got, want, what, cw):
    if torch.equal(got, want):
        return
    i = int(torch.nonzero(got != want)[0])
    raise AssertionError(f"{what} differs first at {where(i, cw)}: got {int(got[i]) & (2 ** 64 - 1):#018x}, oracle "
                         f"{int(want[i]) & (2 ** 64 - 1):#018x}; {int((got != want).sum())} words differ")


def check_totals(got, ref, nbits, cw):
    for name in TOTALS:
        assert got[name] == ref[2][name], (name, got[name], ref[2][name])
    assert got["bits"] == nbits
    assert got["chunks"] == -(-((nbits + 63) // 64) // cw)
    assert got["serial_fallback"] == 0


# ---------------------------------------------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("k,cw,wb,off", CELLS, ids=[f"k{k}-cw{cw}-warm{wb}" + ("-shifted" if off else "") for k, cw, wb, off in CELLS])
def test_form_matrix(gpu, oracle, k, cw, wb, off, pattern):
    form = expected_form(k, cw, wb, off)
    s = stream(gpu, oracle, k, pattern)
    src = s["t_shifted"][off:] if off else s["t"]
    assert src.data_ptr() % 16 == 8 * off and src.is_contiguous()
    got = gpu.PRBSErrorDetector(k).run_stream(src, NBITS, want_err=True, want_reload=True, chunk_bits=cw * 64, warm_bits=wb)
    print(f"\nk={k} {pattern} chunk_words={cw} warm_bits={wb} {form}: chunks={got['chunks']} rerun={got['chunks_rerun']} "
          f"serial={got['serial_fallback']}", end="")
    same_words(got["err"], s["err"], "err", cw)
    same_words(got["reload"], s["reload"], "reload", cw)
    check_totals(got, s["ref"], NBITS, cw)
    sparse = form in ("fused", "two-kernel")
    if pattern == "clean":
        # a sparse form starts a chunk from the state its flags imply, which on a clean stream is the true one.  The dense form
        # starts from reset `warm` bits earlier: the all-ones history triggers at once, the LFSR holds k true bits k clocks later
        # and no error arises after that; the junk errors of those k clocks either trigger ONE more reload (over by clock
        # 1 + k + k + k // 2, history zeroed) or have left the history by clock 1 + 2 k: the true state from there on
        assert sparse or wb >= 2 * k + k // 2 + 2
        assert got["chunks_rerun"] == 0
    if pattern == "storm" and wb == 64 and sparse:
        assert got["chunks_rerun"] > 0


def one_cell_per_form(k):
    if k == 20:
        return [(128, 1024, 0), (24, 1024, 0)]                             # dense in tiles, dense lane by lane
    return [(128, 1024, 0), (64, 1024, 0), (64, 1024, 1)]                  # fused, two-kernel, dense lane by lane


@pytest.mark.parametrize("want_err,want_reload", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("k", KS)
def test_every_output_combination(gpu, oracle, k, want_err, want_reload):
    """Both / err only / reload only / totals only (det_chunk_kernel<K, false>, det_span_tiled without outputs): the
    totals are the oracle's in all four, the streams where asked for."""
    s = stream(gpu, oracle, k, "storm")
    for cw, wb, off in one_cell_per_form(k):
        src = s["t_shifted"][off:] if off else s["t"]
        got = gpu.PRBSErrorDetector(k).run_stream(src, NBITS, want_err=want_err, want_reload=want_reload, chunk_bits=cw * 64, warm_bits=wb)
        check_totals(got, s["ref"], NBITS, cw)
        assert ("err" in got) == want_err and ("reload" in got) == want_reload
        if want_err:
            same_words(got["err"], s["err"], "err", cw)
        if want_reload:
            same_words(got["reload"], s["reload"], "reload", cw)


@pytest.mark.parametrize("k,cw,wb,off", [(31, 128, 1024, 0), (31, 64, 1024, 0), (31, 64, 1024, 1), (9, 1024, 64, 0), (20, 128, 1024, 0),
                                         (20, 24, 1024, 0)])
def test_outputs_at_8_byte_alignment_stay_inside(gpu, oracle, k, cw, wb, off):
    """err / reload given as views one word (8 bytes) into larger buffers -- the interface asks for no more than a
    uint64_t * -- filled with a guard value: exact streams, and the guard words in front and behind untouched."""
    from basebandboard_amd import _lib
    s = stream(gpu, oracle, k, "storm")
    src = s["t_shifted"][off:] if off else s["t"]
    pad = 32
    guard = GUARD                          # (positive as an int64)
    bufs = [torch.full((NWORDS + 1 + pad,), guard, dtype=torch.int64, device="cuda") for _ in range(2)]
    views = [b[1: 1 + NWORDS] for b in bufs]
    assert all(v.data_ptr() % 16 == 8 for v in views)
    st = _lib.DetectorStats()
    _lib.check(_lib.lib().bbb_prbs_detector_stream(k, C.c_void_p(src.data_ptr()), NBITS, C.c_void_p(views[0].data_ptr()),
                                                   C.c_void_p(views[1].data_ptr()), C.byref(st), cw * 64, wb, 0,
                                                   C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "bbb_prbs_detector_stream")
    got = {n: int(getattr(st, n)) for n, _ in _lib.DetectorStats._fields_}
    check_totals(got, s["ref"], NBITS, cw)
    same_words(views[0], s["err"], "err", cw)
    same_words(views[1], s["reload"], "reload", cw)
    for b in bufs:
        assert int(b[0]) == guard and bool((b[1 + NWORDS:] == guard).all())


@pytest.mark.parametrize("k", (9, 31))
@pytest.mark.parametrize("nbits", (128 * 64 - 1, 128 * 64, 128 * 64 + 1, 255 * 64 + 5, 256 * 64, 257 * 64 + 63, 64 * 128 * 64 + 1,
                                   65 * 128 * 64 - 1))
def test_ragged_lengths_fused(gpu, oracle, k, nbits):
    """Short streams through the fused kernel: one chunk, a partial second chunk, one wave and one word, two waves less one bit."""
    assert form_of(k, 128, 1024) == "fused"
    nw = (nbits + 63) // 64
    words = gpu.PRBS(k).generate(nbits + 64).cpu().numpy().view(np.uint64)[:nw].copy()
    rng = np.random.default_rng(nbits + k)
    pos = set(int(x) for x in rng.integers(0, nbits, size=nbits // 1000))
    pos.update((nbits - 1, (nbits // 64) * 64 - 1, 127 * 64 + 63))         # the last bit, bit 63 of the last full word and of the first chunk
    xor_bits(words, [t for t in pos if t < nbits])
    e, r, st = oracle.prbs_detector_packed(k, words, nbits)
    got = gpu.PRBSErrorDetector(k).run_stream(torch.from_numpy(words.view(np.int64)).cuda(), nbits, want_err=True, want_reload=True,
                                              chunk_bits=128 * 64, warm_bits=1024)
    same_words(got["err"], torch.from_numpy(e.view(np.int64)).cuda(), "err", 128)
    same_words(got["reload"], torch.from_numpy(r.view(np.int64)).cuda(), "reload", 128)
    check_totals(got, (e, r, st), nbits, 128)

