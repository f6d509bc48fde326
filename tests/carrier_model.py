"""numpy int64 model of the carrier recovery of include/bbb.h (bbb_carrier_*), written from the header's formulas alone.

  block j = the pairs [j L, (j + 1) L) below nin        nblocks = final ? ceil(nin / L) : floor(nin / L)
  SR_j = sum(I I - Q Q)    SI_j = 2 sum(I Q)             m = max(|SR|, |SI|)    s = max(0, bitlength(m) - 15)
  h_j  = (cordic phase of (SR >> s, SI >> s) mod 2^16) >> 1
  d = (h_j - est_(j-1)) mod 2^16;  est_j = h_j if d < 16384 or d >= 49152 else (h_j + 32768) mod 2^16
  adr = est_j >> 6   c = ROM[(adr + 256) mod 1024]   s = ROM[adr]
  I' = sat16((I c + Q s) >> 15)    Q' = sat16((Q c - I s) >> 15)    bit = I' >= threshold (> with strict)

The CORDIC is tests/ddc_model.py's and the ROM tests/nco_model.py's.  The block sums and the derotation are vectorised; the
unwrap is the serial rule, one block at a time.  Nothing here is shared with basebandboard_amd/csrc/carrier_common.hpp.
"""
import numpy as np

import ddc_model
import nco_model
from nco_model import ROM

STARTED = 1 << 63


def plan(nin, L=32, final=True):
    nblocks = -(-nin // L) if final else nin // L
    return nblocks, min(nin, nblocks * L)


def bitlength(m):
    """Of non-negative int64 values below 2^62, exactly (no floating point)."""
    m = np.asarray(m, dtype=np.int64)
    n = np.zeros(m.shape, dtype=np.int64)
    for k in range(62):
        n = np.where(m >> k != 0, k + 1, n)
    return n


def block_h(pairs, L, nblocks):
    """(h, zero) of every block; the last block may be partial (the missing pairs add nothing)."""
    x = np.zeros((nblocks * L, 2), dtype=np.int64)
    x[:len(pairs)] = pairs
    i, q = x[:, 0].reshape(nblocks, L), x[:, 1].reshape(nblocks, L)
    sr, si = (i * i - q * q).sum(axis=1), 2 * (i * q).sum(axis=1)
    assert max(np.abs(sr).max(initial=0), np.abs(si).max(initial=0)) <= 2 ** 41
    s = np.maximum(0, bitlength(np.maximum(np.abs(sr), np.abs(si))) - 15)
    a, b = sr >> s, si >> s
    assert a.min(initial=0) >= -32768 and a.max(initial=0) <= 32767 and b.min(initial=0) >= -32768 and b.max(initial=0) <= 32767
    th = ddc_model.cordic(a, b)[1].astype(np.int64) if nblocks else np.zeros(0, dtype=np.int64)
    return (th & 0xFFFF) >> 1, (sr == 0) & (si == 0)


def unwrap(h, est):
    """The serial rule from est_(-1) = est: (est_j, flips, sum of the wrapped steps)."""
    out, flips, steps = np.zeros(len(h), dtype=np.int64), 0, 0
    for j, hj in enumerate(h.tolist()):
        d = (hj - est) & 0xFFFF
        nxt = hj if d < 16384 or d >= 49152 else (hj + 32768) & 0xFFFF
        flips += (nxt >> 15) != (est >> 15)
        w = (nxt - est) & 0xFFFF
        steps += w - 65536 if w >= 32768 else w
        est = out[j] = nxt
    return out, flips, steps


def pack(bits, nwords):
    b = np.zeros(nwords * 64, dtype=np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint64)


def run(pairs, L=32, init_phase=0, threshold=0, strict=False, state=(0, 0), final=True):
    """One call: a dict of iq [n, 2] int16, bits (uint8, n of them), words (uint64, ceil(nblocks L / 64)), soft int16 [n],
    phases uint16 [nblocks], state (two ints), stats (four ints, the last signed), nblocks, nconsumed."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    nblocks, n = plan(len(pairs), L, final)
    x = pairs[:n]
    h, zero = block_h(x, L, nblocks)
    est0 = state[0] & 0xFFFF if state[0] >> 63 else init_phase
    est, flips, steps = unwrap(h, est0)
    adr = np.repeat(est >> 6, L)[:n]
    c, s = ROM[(adr + 256) & 1023], ROM[adr]
    io = np.clip((x[:, 0] * c + x[:, 1] * s) >> 15, -32768, 32767)
    qo = np.clip((x[:, 1] * c - x[:, 0] * s) >> 15, -32768, 32767)
    bits = (io > threshold if strict else io >= threshold).astype(np.uint8)
    st0 = (STARTED | int(est[-1])) if nblocks else state[0]
    return dict(iq=np.stack([io, qo], axis=1).astype(np.int16), bits=bits, words=pack(bits, (nblocks * L + 63) // 64), soft=io.astype(np.int16),
                phases=est.astype(np.uint16), state=(st0, state[1] + n), stats=[nblocks, int(flips), int(zero.sum()), int(steps)],
                nblocks=nblocks, nconsumed=n)


def stream(pairs, cuts, L=32, **kw):
    """The record piece by piece at `cuts` (multiples of L), the state carried, only the last piece final: run()'s dict."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    state, stats, parts = (0, 0), [0, 0, 0, 0], []
    edges = [0] + list(cuts) + [len(pairs)]
    for k, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        r = run(pairs[a:b], L, state=state, final=k == len(edges) - 2, **kw)
        assert r["nconsumed"] == b - a
        state, stats = r["state"], [u + v for u, v in zip(stats, r["stats"])]
        parts.append(r)
    out = {key: np.concatenate([p[key] for p in parts]) for key in ("iq", "bits", "soft", "phases")}
    out.update(state=state, stats=stats)
    return out


# ---- the closed loop: the down-converter's own example with the two oscillators apart ------------------------------------------
LOOP = dict(fcw=1 << 20, spb=64, nbits=4096, pm=-512, sigma=12000.0, taps=[1] * 64, shift=6, decim=64, phase=66, L=32, init_phase=16384,
            offsets=(256, -256), data_seed=5, noise_seed=11)


def loop_capture():
    """(int16 capture, data bits): a carrier at fcw phase-modulated by half a turn per bit 1, 64 samples a bit, plus Gaussian
    noise of sigma 12000, rounded and clipped to int16."""
    p = LOOP
    data = np.random.default_rng(p["data_seed"]).integers(0, 2, p["nbits"])
    pm = np.repeat(np.where(data == 1, p["pm"], 0), p["spb"]).astype(np.int64)
    x, _ = nco_model.closed(len(pm), p["fcw"], pm=pm)
    noise = np.random.default_rng(p["noise_seed"]).normal(0.0, p["sigma"], len(pm))
    return np.clip(np.round(x.astype(np.float64) + noise), -32768, 32767).astype(np.int16), data


def loop_pairs(capture, off):
    """The capture through the down-converter whose fcw lies `off` below the transmitter's: [4095, 2] int16; pair q is data
    bit q."""
    p = LOOP
    fcw = p["fcw"] - off
    return ddc_model.ddc(capture, fcw, p["taps"], p["shift"], p["decim"], p["phase"], pa0=(-3 * fcw) % (1 << 24))


def loop_ideal_offset(off):
    """Turns per pair."""
    return off * LOOP["decim"] / 2 ** 24
