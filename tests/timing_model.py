"""Serial restatement of the symbol timing recovery of include/bbb.h (bbb_timing_*), on fir_model's acc:

  a(n) = acc(n), n in [-1, nin)        block j = samples [j L P, (j + 1) L P)        E_j[p] = sum_i |a(j L P + i P + p) - threshold|

The tracker's state is (locked, phi).  A first block after reset takes init_phase, or the arg-max of its metric; every other
block moves phi by at most one, towards the larger neighbour where that beats the current phase by more than cur >> h.  A move
across phase 0 is a wrap: the block then emits L - 1 (up) or L + 1 (down) instants instead of L, the extra one a sample in front
of the block.  Written from the header's definition alone; the device's core (csrc/timing_common.hpp) is not consulted.
"""
import numpy as np

import fir_model

ACQUIRE = 0xFFFFFFFF
LOCKED = 1 << 63


def plan(nin, P, L, final=True):
    """(nblocks, nconsumed, max_bits)."""
    nblocks = -(-nin // (L * P)) if final else nin // (L * P)
    return nblocks, min(nin, nblocks * L * P), nblocks * (L + 1)


def soft(v, shift=0, out_bytes=2):
    v = np.asarray(v, dtype=np.int64)
    if out_bytes == 2:
        return np.clip(v >> shift, -32768, 32767).astype(np.int16)
    return v.astype(np.int32)


def run(x, P, taps=(1,), L=64, h=4, threshold=0, strict=False, init_phase=ACQUIRE, before=(), state=(0, 0), final=True, shift=0,
        out_bytes=2):
    """One call: a dict of bits (uint8), soft, phases (uint8 per block), instants (sample index of every bit), moves and wraps
    per block, state (two ints), stats [blocks, moves, wraps up, wraps down], nbits, nconsumed."""
    x = np.asarray(x, dtype=np.int64)
    before = np.asarray(before, dtype=np.int64)[-len(taps):] if len(before) else np.zeros(0, dtype=np.int64)
    nblocks, nin, _ = plan(len(x), P, L, final)
    # a(-1) .. a(nin - 1): the last history sample becomes a record sample of its own
    hist = np.concatenate([np.zeros(1, dtype=np.int64), before])
    a = fir_model.acc(np.concatenate([hist[-1:], x[:nin]]), taps, hist[:-1])
    mag = np.abs(a[1:] - threshold)
    locked, phi = bool(state[0] >> 63), (state[0] & 0xFFFFFFFF) % P
    phases, moves, wraps, instants = [], [], [], [np.zeros(0, dtype=np.int64)]
    for j in range(nblocks):
        blk = mag[j * L * P:(j + 1) * L * P]
        E = [int(blk[p::P].sum()) for p in range(P)]
        m = w = 0
        if not locked:
            phi = init_phase if init_phase < P else max(range(P), key=lambda p: (E[p], -p))
            locked = True
        else:
            cur, up, dn = E[phi], E[(phi + 1) % P], E[(phi + P - 1) % P]
            margin = cur >> h
            if up > cur + margin and up >= dn:
                m = 1
            elif dn > cur + margin:
                m = -1
            phi = (phi + m) % P
            if m == 1 and phi == 0:
                w = 1
            if m == -1 and phi == P - 1:
                w = -1
        phases.append(phi)
        moves.append(m)
        wraps.append(w)
        t = j * L * P + phi + P * np.arange(w, L, dtype=np.int64)
        instants.append(t[t < nin])
    instants = np.concatenate(instants)
    v = a[instants + 1]
    bits = (v > threshold if strict else v >= threshold).astype(np.uint8)
    st0 = (LOCKED | phi) if nblocks else state[0]
    wr = np.array(wraps, dtype=np.int64)
    return dict(bits=bits, soft=soft(v, shift, out_bytes), phases=np.array(phases, dtype=np.uint8), instants=instants,
                moves=np.array(moves, dtype=np.int64), wraps=wr, state=(st0, state[1] + len(bits)), nbits=len(bits), nconsumed=nin,
                stats=[nblocks, int(np.count_nonzero(moves)), int((wr > 0).sum()), int((wr < 0).sum())])


def stream(x, P, cuts, taps=(1,), **kw):
    """The record cut at `cuts` (multiples of L P), each piece with len(taps) samples of history and the state words, final on
    the last piece only: the same dict (without instants)."""
    x = np.asarray(x, dtype=np.int64)
    state, stats = (0, 0), np.zeros(4, dtype=np.int64)
    bits, softs, phases = [], [], []
    edges = [0] + list(cuts) + [len(x)]
    for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        r = run(x[lo:hi], P, taps, before=x[max(0, lo - len(taps)):lo], state=state, final=k == len(edges) - 2, **kw)
        assert r["nconsumed"] == hi - lo or k == len(edges) - 2
        state = r["state"]
        stats += r["stats"]
        bits.append(r["bits"])
        softs.append(r["soft"])
        phases.append(r["phases"])
    return dict(bits=np.concatenate(bits), soft=np.concatenate(softs), phases=np.concatenate(phases), state=state, stats=stats.tolist())


# ---- records that exercise the tracker -------------------------------------------------------------------------------------

def ramp(P, L, nblocks, direction, start=0, amp=1000, low=10):
    """A record whose per-phase amplitude peak advances (direction +1) or retreats (-1) one phase per block: block j has
    `amp` at phase (start + direction * j) mod P and `low` elsewhere, signs alternating from symbol to symbol.  With the
    tracker entered at `start` it moves in every block and wraps every P blocks."""
    x = np.full((nblocks, L, P), low, dtype=np.int64)
    for j in range(nblocks):
        x[j, :, (start + direction * j) % P] = amp
    x *= np.where(np.arange(L) & 1, -1, 1)[None, :, None]
    return x.reshape(-1)


def drift_path(rng, P, nblocks, hold=2):
    """The peak phase of every block of a drifting record: from phase 1 three phases down (across the wrap), five up (across it
    again), then a random walk; every phase is held for `hold` blocks."""
    steps = [-1] * 3 + [1] * 5
    nsteps = -(-nblocks // hold)
    steps = (steps + rng.choice([-1, 0, 1], max(0, nsteps - len(steps))).tolist())[:nsteps]
    peak = (1 + np.concatenate([[0], np.cumsum(steps)])) % P
    return np.repeat(peak, hold)[:nblocks]


def drift_record(rng, P, L, n, amp=2000, hold=2):
    """Uniform noise of `n` samples whose amplitude depends on the sampling phase, largest at a peak phase that drifts along
    drift_path and falling off by a quarter per phase of circular distance (never below a fifth): the tracker acquires the peak
    and follows it through wraps in both directions."""
    nblocks = -(-n // (L * P))
    peak = drift_path(rng, P, nblocks, hold)
    d = np.abs(np.arange(P)[None, :] - peak[:, None])
    d = np.minimum(d, P - d)
    gain = np.maximum(0.2, 1.0 - 0.25 * d)                                # [nblocks, P]
    x = rng.integers(-amp, amp + 1, (nblocks, L, P)) * gain[:, None, :]
    return x.astype(np.int64).reshape(-1)[:n]


def phase_taps(rng, ntaps, P, total=300):
    """`ntaps` taps that keep a sample's phase: weight only at the delays that are multiples of P (and 1 at the last tap, so that
    the filter does reach ntaps samples), sum |h| <= total + 1."""
    h = np.zeros(ntaps, dtype=np.int64)
    at = np.arange(0, ntaps, P)
    h[at] = rng.multinomial(total, [1 / len(at)] * len(at)) * rng.choice([-1, 1], len(at))
    if h[0] == 0:
        h[0] = 1
    if ntaps > 1 and h[-1] == 0:
        h[-1] = 1
    return h.tolist()


# ---- the closed loop: a capture from an ADC with its own clock -----------------------------------------------------------------
# The CPU waveform of dfe_model.loop_record's kind (PRBS-7, roll-off 0.5, noise_var 8, 2^18 samples) resampled in integers
# with a clock offset of +-20 / 65536 (305 ppm), recovered with P 8, L 64, h 4, acquire, no filter.
LOOP = dict(k=7, beta=0.5, noise_var=8, n=1 << 18, P=8, L=64, h=4, steps=(65536 + 20, 65536 - 20), lags=range(-14, 15))
LOOP_MAX_ERRORS = 10           # recovered
LOOP_MIN_FIXED_ERRORS = 10000  # the best fixed phase
LOOP_WRAPS = 10                # in the drift's direction, none in the other


def loop_waveform(oracle):
    """(the shaper's waveform with the spare samples the slower clock reaches, the data bits)."""
    from basebandboard_amd.bitshaper import rcf_coefficients
    n = LOOP["n"]
    lut = oracle.Lutopt(path=oracle.data_path(256))
    x = oracle.tx(lut, 1, rcf_coefficients(LOOP["beta"]), LOOP["k"], n + 128, noise_var=LOOP["noise_var"], warmup=16)
    return np.asarray(x, dtype=np.int64), np.array(oracle.prbs_bits(LOOP["k"], n // 8 + 64)[0])


def resample(x, step, n):
    """y[m] = (x[i] (65536 - f) + x[i + 1] f) >> 16 with pos = m step, i = pos >> 16, f = pos & 65535, for m < n."""
    x = np.asarray(x, dtype=np.int64)
    pos = np.arange(n, dtype=np.int64) * step
    i, f = pos >> 16, pos & 65535
    assert i[-1] + 1 < len(x)
    return ((x[i] * (65536 - f) + x[i + 1] * f) >> 16).astype(np.int16)


def loop_errors(bits, ref, ncompare):
    """The fewest errors of the first `ncompare` usable decisions against the data bits over the lags of LOOP (decision m is
    data bit m - lag), and that lag."""
    best = None
    for lag in LOOP["lags"]:
        m = np.arange(len(bits))
        k = m - lag
        ok = (k >= 0) & (k < len(ref))
        mm, kk = m[ok][:ncompare], k[ok][:ncompare]
        e = int((bits[mm] != ref[kk]).sum())
        if best is None or e < best[0]:
            best = (e, lag)
    return best


def loop_compare_bits():
    return LOOP["n"] // LOOP["P"] - 46


def fixed_phase_errors(y, ref):
    """The fewest errors any fixed phase leaves: (errors, phase)."""
    P = LOOP["P"]
    out = []
    for p in range(P):
        bits = (y[p::P] >= 0).astype(np.uint8)
        out.append((loop_errors(bits, ref, loop_compare_bits())[0], p))
    return min(out)
