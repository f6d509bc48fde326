"""bbb_dfe_run on the GPU against tests/dfe_model.py: bits, soft values, the final state word and the counters of stats_dev, with
regions and warm-ups set small through the call so that a short record has many regions, the speculation and the repair, and more regions than two passes of
the region and repair kernels' grids."""
import ctypes as C

import numpy as np
import pytest
import torch

import fir_model
import grid
import dfe_model as M
import test_dfe_host as H

pytestmark = pytest.mark.gpu

BOUND = 2 ** 31 - 1
GUARD = -0x0123456789ABCDEF


def _call(gpu, x, nb, taps, fb, spb, phase=0, threshold=0, strict=False, region=0, warmup=0, state=0, shift=0, soft=np.int16,
          in_off=0, bits_off=0, soft_off=0, unaligned=False):
    """One bbb_dfe_run through the C ABI on tensors placed `*_off` elements behind an aligned address; the words and values
    next to the outputs must stay as they were.  unaligned: the offsets must put the three pointers off 16-byte alignment.
    Returns (bits uint8, soft or None, state, stats dict)."""
    from basebandboard_amd import _lib
    dev = torch.device("cuda", 0)
    x = np.asarray(x, dtype=np.int16)
    nin = len(x) - nb
    nsym = fir_model.nout(nin, spb, phase)
    nwords = (nsym + 63) // 64
    buf = torch.zeros(in_off + len(x) + 8, dtype=torch.int16, device=dev)
    buf[in_off:in_off + len(x)] = torch.from_numpy(x).to(dev)
    bits = torch.full((bits_off + nwords + 2,), GUARD, dtype=torch.int64, device=dev)
    st = torch.tensor([state - (1 << 32) if state >= 1 << 31 else state], dtype=torch.int32, device=dev)
    stats = torch.tensor([1000, 2000, 3000, 4000], dtype=torch.int64, device=dev)
    c = _lib.DfeCfg()
    c.ff.ntaps = len(taps)
    for i, v in enumerate(taps):
        c.ff.taps[i] = v
    c.ff.shift, c.ff.decim, c.ff.phase, c.ff.out_bytes = shift, spb, phase, 2 if soft is None else np.dtype(soft).itemsize
    c.nfb = len(fb)
    for i, v in enumerate(fb):
        c.fb[i] = v
    c.threshold, c.strict, c.region_symbols, c.warmup_symbols = threshold, int(strict), region, warmup
    sv = None
    if soft is not None:
        sv = torch.full((soft_off + nsym + 2,), 0x5A5A, dtype=torch.int16 if soft == np.int16 else torch.int32, device=dev)
    got = C.c_uint64()
    p_in, p_bits = buf.data_ptr() + 2 * (in_off + nb), bits.data_ptr() + 8 * (bits_off + 1)
    p_soft = None if sv is None else sv.data_ptr() + sv.element_size() * (soft_off + 1)
    if unaligned:
        assert p_in % 16 and p_bits % 16 and (p_soft is None or p_soft % 16), (p_in % 16, p_bits % 16, p_soft)
    _lib.check(_lib.lib().bbb_dfe_run(C.c_void_p(p_in), nin, nb, C.byref(c), C.c_void_p(st.data_ptr()), C.c_void_p(p_bits),
                                      None if p_soft is None else C.c_void_p(p_soft),
                                      C.c_void_p(stats.data_ptr()), C.byref(got), 0,
                                      C.c_void_p(torch.cuda.current_stream(0).cuda_stream)), "bbb_dfe_run")
    assert got.value == nsym
    w = bits.cpu().numpy()
    assert (w[:bits_off + 1] == GUARD).all() and w[-1] == GUARD, "a word next to bits_packed_dev was written"
    out_soft = None
    if sv is not None:
        s = sv.cpu().numpy()
        assert (s[:soft_off + 1] == 0x5A5A).all() and s[-1] == 0x5A5A, "a value next to soft_dev was written"
        out_soft = s[soft_off + 1:-1]
    words = w[bits_off + 1:-1].view(np.uint64)
    got_bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    assert not got_bits[nsym:].any(), "the unused bits of the last word are not 0"
    stv = (stats.cpu().numpy() - np.array([1000, 2000, 3000, 4000])).tolist()
    return got_bits[:nsym], out_soft, int(st.cpu().numpy().view(np.uint32)[0]), dict(zip(("regions", "not_proven", "repaired", "symbols"), stv))


def _check(gpu, x, nb, taps, fb, spb, phase=0, threshold=0, strict=False, region=0, warmup=0, state=0, shift=0, soft=np.int16, **off):
    """The call against the model; returns the counters."""
    x = np.asarray(x)
    bits, sv, st, stats = _call(gpu, x, nb, taps, fb, spb, phase, threshold, strict, region, warmup, state, shift, soft, **off)
    a = fir_model.acc(x[nb:], taps, x[:nb])[phase::spb]
    wb, v, ws, _ = M.decide(a, fb, threshold, strict, state)
    want = M.replay(a, fb, threshold, strict, state, region or 4096, warmup or 64)
    print("stats", stats, "model", want)
    bad = np.flatnonzero(bits != wb)
    assert len(bad) == 0, f"{len(bad)} bits differ, the first at symbol {bad[0]} of {len(wb)}"
    if soft is not None:
        assert np.array_equal(sv, M.soft(v, shift, np.dtype(soft).itemsize)), "soft values differ"
    assert st == ws, "final state differs"
    assert stats == want
    return stats


def _taps(rng, ntaps, total):
    """ntaps int16 taps with sum |h| == total."""
    mag = rng.multinomial(total, [1 / ntaps] * ntaps)
    assert mag.max() <= 32767
    return (mag * rng.choice([-1, 1], ntaps)).tolist()


def _fb(rng, nfb, total):
    if nfb == 0:
        return []
    return [int(v) for v in rng.multinomial(total, [1 / nfb] * nfb) * rng.choice([-1, 1], nfb)]


@pytest.mark.parametrize("spb", (1, 2, 3, 8, 256))
def test_every_nfb_at_the_bound_and_inside(gpu, spb):
    """nfb 0..4, taps at the int32 bound (32768 sum |h| + sum |fb| = 2^31 - 1) and far inside it, both strict values, nonzero
    thresholds, ragged nin, nbefore 0 and beyond ntaps, every pointer off 16-byte alignment.  The samples are scaled so that
    the feed-forward sums are of the feedback's size: starts get proven, speculated and repaired."""
    rng = np.random.default_rng(100 + spb)
    nsym = 2500 if spb < 256 else 255
    repaired = unproven = 0
    for nfb in range(5):
        for at_bound in (True, False):
            ntaps = int(rng.choice([7, 8, 9, 33] if at_bound else [1, 7, 8, 9, 33]))
            sum_h = 60000 if at_bound else 500
            taps = _taps(rng, ntaps, sum_h)
            fb = _fb(rng, nfb, BOUND - 32768 * sum_h if at_bound else 3000)
            assert M.valid(taps, fb) and (not at_bound or nfb == 0 or 32768 * sum_h + sum(abs(v) for v in fb) == BOUND)
            nb = 0 if at_bound else ntaps + 5
            phase = int(rng.integers(0, spb))
            n = min(1 << 16, nsym * spb + int(rng.integers(0, spb + 3))) - nb
            amp = max(2, int(sum(abs(v) for v in fb) / sum_h * 2)) if nfb else 2000
            x = rng.integers(-amp, amp + 1, n + nb)
            if at_bound:
                x[rng.integers(0, n, 40)] = rng.choice([-32768, 32767], 40)          # full-scale samples among them
            st = _check(gpu, x, nb, taps, fb, spb, phase, int(rng.integers(-50, 50)), bool((nfb + at_bound) & 1), region=37 + 2 * nfb,
                        warmup=3 + nfb, state=int(rng.integers(0, 1 << 32)), shift=int(rng.integers(0, 12)),
                        soft=np.int32 if at_bound else np.int16, in_off=1 + 2 * nfb + (nb & 1), bits_off=2 * (nfb & 1),
                        soft_off=2 * nfb, unaligned=True)
            repaired += st["repaired"]
            unproven += st["not_proven"]
    assert spb == 256 or (unproven > 0 and repaired > 0)             # (256: 255 symbols, a handful of regions)


def test_full_scale_sums_at_the_bound(gpu):
    """Every sample -32768 or 32767 against taps of sum |h| = 65535 and fb at what the bound leaves: v reaches both ends of int32."""
    rng = np.random.default_rng(7)
    taps = _taps(rng, 16, 65535)
    # blocks of 16 samples that meet the taps sign for sign, or sign against sign, at every fourth symbol
    x = np.where(np.repeat(rng.integers(0, 2, 375), 16), 32767, -32767) * np.sign(np.tile(taps[::-1], 375))
    x[x == -32767] = -32768
    _check(gpu, x, 0, taps, _fb(rng, 3, BOUND - 32768 * 65535), 4, 3, soft=np.int32, region=50, warmup=2)


def test_empty_and_tiny_records(gpu):
    for nin, state, nfb in ((0, 0xFFFFFFFF, 2), (0, 5, 4), (1, 0xF, 4), (63, 1, 1), (64, 0, 1), (65, 3, 3)):
        st = _check(gpu, np.arange(nin) * 7 - 100, 0, [1, 1], [9, 4, 2, 1][:nfb], 1, state=state, region=16, warmup=4)
        assert st["symbols"] == nin
    _check(gpu, np.arange(5), 0, [1], [3], 8, phase=7)                               # a record that ends in front of its first symbol


def test_nfb_0_is_fir_slice(gpu):
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.integers(-3000, 3000, 50_001).astype(np.int16)).to("cuda:0")
    for spb, phase in ((1, 0), (8, 5), (3, 2)):
        fir = gpu.FIR(rng.integers(-100, 100, 21).tolist())
        for strict in (False, True):
            want, nbits = fir.slice(x, stride=spb, phase=phase, threshold=77, strict=strict, nbefore=30)
            d = gpu.DFE(fir, [], spb, phase, threshold=77, strict=strict, region_symbols=301, warmup_symbols=8)
            got, n2, soft = d.equalize(x, nbefore=30, out_dtype=torch.int32)
            assert n2 == nbits and torch.equal(got, want)
            assert torch.equal(soft, fir.filter(x, decim=spb, phase=phase, nbefore=30, out_dtype=torch.int32))
            assert d.stats() == dict(regions=(nbits + 300) // 301, not_proven=0, repaired=0, symbols=nbits)


@pytest.mark.parametrize("spb,phase,region", ((1, 0, 37), (8, 3, 101), (2, 1, 64)))
def test_all_ambiguous_record_is_repaired(gpu, spb, phase, region):
    """Zero samples, fb = {5}, threshold 0: every decision is the inverse of the last, so no warm-up map is constant and the
    true start alternates with the parity of the region's first symbol.  With an odd region length (or, at 64, an odd warm-up)
    the speculation from state 0 fails for half of the regions: the repair pass is what makes the bits right."""
    x = np.zeros(1 << 15 if spb > 1 else 1 << 13, dtype=np.int16)
    warmup = 7 if region == 64 else 64
    st = _check(gpu, x, 0, [3, -2, 1], [5], spb, phase, region=region, warmup=warmup)
    assert st["not_proven"] == st["regions"] - 1 and st["repaired"] > 0
    assert st["repaired"] >= (st["regions"] - 3) // 2
    bits = _call(gpu, x, 0, [3, -2, 1], [5], spb, phase, region=region, warmup=warmup)[0]
    assert np.array_equal(bits, (np.arange(len(bits)) + 1) & 1)


@pytest.mark.parametrize("spb", (1, 8))
def test_ambiguous_stretch_across_every_boundary(gpu, spb):
    """A stretch of zero samples longer than the warm-up, among strongly decided symbols, placed across a region boundary, a
    step boundary (2048 samples) and wave boundaries inside a step (bbb_dfe_geometry: 64 symbols, 512 in the block form of
    decim 1, where a lane owns eight), with the region chosen so that the three do not coincide."""
    rng = np.random.default_rng(9)
    from basebandboard_amd import dfe
    g = dfe.geometry(spb)
    wave = g["wave_symbols"]
    assert (g["step_samples"], wave) == (2048, 512 if spb == 1 else 64)
    taps, fb, warmup, region, phase = [40, 30, 20], [50, -20], 16, 1000, spb - 1
    nsym = 4 * region + 17
    step_sym = (g["step_samples"] - phase + spb - 1) // spb                      # the first symbol of step 1
    places = [2 * region, step_sym] + [wave * j for j in (3, 5, 11) if wave * j + 40 < nsym]
    assert len(places) >= 4 and all(p % region and p % step_sym for p in places[2:])
    for at in places:
        x = rng.choice([-500, 500], nsym * spb)
        lo, hi = (at - 40) * spb + phase, (at + 40) * spb + phase
        x[max(0, lo - 2):hi] = 0
        st = _check(gpu, x, 0, taps, fb, spb, phase, region=region, warmup=warmup)
        assert st["regions"] == 5
    # the stretch over the region boundary leaves that region's start unproven
    x = rng.choice([-500, 500], nsym * spb)
    x[(2 * region - 40) * spb:(2 * region + 40) * spb] = 0
    assert _check(gpu, x, 0, taps, [50], spb, phase, region=region, warmup=warmup)["not_proven"] == 1


@pytest.mark.parametrize("spb", (1, 2))
def test_more_than_two_passes_of_the_grids(gpu, spb):
    """Regions of 16 symbols (tests/test_dfe_host.py builds the records), in the block form of one sample a symbol and in the
    point form.  Noisy data over 2 * 8 * cus + 5 regions: a workgroup of the region kernel takes three regions, re-using the
    image, the waves' totals and the gathered ends behind its loop's last barrier.  The all-zero record over twice as many:
    the model repairs more regions than two passes of the repair kernel's grid, which then loops as well."""
    x, taps, fb, phase = H.multipass_noisy(spb, grid.cus())
    st = _check(gpu, x, 0, taps, fb, spb, phase, region=H.MULTIPASS_REGION, warmup=H.MULTIPASS_NOISY["warmup"], state=5, shift=1,
                in_off=3, bits_off=1, soft_off=1)
    assert st["regions"] == grid.passes(grid.DFE) and 0 < st["repaired"] <= st["not_proven"]
    z, Z = H.multipass_zero(spb, grid.cus()), H.MULTIPASS_ZERO
    want = M.replay(np.zeros(len(z) // spb, dtype=np.int64), Z["fb"], 0, False, 0, H.MULTIPASS_REGION, Z["warmup"])
    assert want["repaired"] > 2 * grid.DFE * grid.cus(), "the model does not repair more than two passes of regions"
    st = _check(gpu, z, 0, Z["taps"], Z["fb"], spb, spb - 1, region=H.MULTIPASS_REGION, warmup=Z["warmup"], soft=np.int32, in_off=1)
    assert st == want


def test_noisy_data_with_the_default_geometry(gpu):
    """Random noisy data under the default region and warm-up: most regions prove their start, and the counters are those of
    the model's own replay of the speculation rule."""
    rng = np.random.default_rng(10)
    data = np.repeat(rng.choice([-400, 400], 1 << 14), 4)
    x = data + np.concatenate([np.zeros(4, dtype=np.int64), (data * 0.7).astype(np.int64)[:-4]]) + rng.normal(0, 150, len(data)).astype(np.int64)
    st = _check(gpu, x, 0, [1, 1, 1, 1], [1120], 4, 3)
    assert st["regions"] == 4 and st["not_proven"] == 0 and st["repaired"] == 0
    st = _check(gpu, x, 0, [1, 1, 1, 1], [1120, 100, -50, 20], 4, 3, region=50, warmup=2)
    assert st["regions"] == 328 and 0 < st["not_proven"] < 328


def test_a_capture_cut_at_random_points_equals_one_call(gpu):
    rng = np.random.default_rng(11)
    n, spb, phase = 40_000, 8, 5
    x = rng.integers(-300, 300, n).astype(np.int16)
    taps, fb = rng.integers(-20, 20, 19).tolist(), [900, -400, 200]
    wb, ws, wst = M.run(x, taps, fb, spb, phase, 11, True, shift=2)
    d = gpu.DFE(gpu.FIR(taps, shift=2), fb, spb, phase, threshold=11, strict=True, region_symbols=61, warmup_symbols=5)
    xt = torch.from_numpy(x).to("cuda:0")
    bits, nbits, soft = d.equalize(xt)
    assert nbits == len(wb) and np.array_equal(np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")[:nbits], wb)
    assert np.array_equal(soft.cpu().numpy(), ws)
    s = d.stream(torch.int16)
    cuts = sorted(rng.integers(0, n, 12).tolist() + [0, 7, 7, n])
    got_b, got_s = [], []
    for lo, hi in zip([0] + cuts, cuts + [n]):
        b, nb, z = s.push(xt[lo:hi])
        got_b.append(np.unpackbits(b.cpu().numpy().view(np.uint8), bitorder="little")[:nb])
        got_s.append(z.cpu().numpy())
    assert np.array_equal(np.concatenate(got_b), wb) and np.array_equal(np.concatenate(got_s), ws)
    assert int(s.state.item()) == wst
    assert d.stats()["symbols"] == 2 * len(wb)
    # slice() with a caller's state word continues where the word says
    st = d.new_state(5)
    b2, n2 = d.slice(xt, state=st)
    w2 = M.run(x, taps, fb, spb, phase, 11, True, state=5)
    assert np.array_equal(np.unpackbits(b2.cpu().numpy().view(np.uint8), bitorder="little")[:n2], w2[0]) and int(st.item()) == w2[2]


def test_closed_loop_counts_equal_the_cpu(gpu, oracle):
    """The echo channel's record through RX.count_errors: the linear receiver and the DFE leave what tests/test_dfe_host.py
    found on the CPU."""
    L = M.LOOP
    y, h, sigma2, _ = M.loop_record(oracle)
    yt = torch.from_numpy(y).to("cuda:0")
    d = gpu.DFE.mmse(h, 8, L["cursor"], L["nff"], L["nfb"], sigma2)
    assert d.ff.taps == M.LOOP_FF and d.fb == M.LOOP_FB
    rx = gpu.RX(L["k"], 8, (17 + L["cursor"]) % 8)
    first = (17 + L["cursor"]) // 8 * 8
    assert rx.count_errors(yt, first_sample=first, dfe=d) == (M.LOOP_DFE_ERRORS, M.LOOP_BITS)
    assert rx.count_errors(yt, first_sample=first, rx_filter=gpu.FIR(M.LOOP_LINEAR_TAPS)) == (M.LOOP_LINEAR_ERRORS, M.LOOP_BITS)
    same = rx.prbsdet.run_stream(*d.slice(yt[first - 11:], nbefore=11, phase=(17 + L["cursor"]) % 8))
    assert rx.detect(yt, first_sample=first, dfe=d)["errors"] == same["errors"]
    with pytest.raises(ValueError, match="not both"):
        rx.slice(yt, rx_filter=gpu.FIR([1]), dfe=d)
    with pytest.raises(ValueError, match="spb"):
        rx.slice(yt, stride=4, dfe=d)
