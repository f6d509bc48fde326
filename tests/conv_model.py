"""Serial restatement of the convolutional codec of include/bbb.h (bbb_conv_*), in numpy integers:

  state h : K-1 bits, bit i = the input bit i + 1 steps back          r = (h << 1) | b
  c_i     = parity of the bits j of r for which bit K-1-j of gen[i] is set     h' = r & (NS - 1)
  gain    = sum_i r_i d(c_i)                                          d(1) = +1, d(0) = -1

Coded bit i of absolute step t is transmitted iff bit t mod p of keep[i] is set, in order of i; idx(t) counts the transmitted
bits in front of step t.  Block j, the steps [j B, (j + 1) B), is decided by one Viterbi run over [max(0, j B - W), min(Nend,
(j + 1) B + D)): a window that starts at step 0 gives init_state 0 and every other state -2^30, any other starts all states at
0; the survivor of h' is the larger m[h] + gain over h = (h' >> 1) | (c << (K-2)), a tie goes to c = 0; the end state is the
largest metric, the lowest index on a tie, or state 0 where a terminated record ends; the decision of step t is bit 0 of the
traced-back path's state behind t.  A call that is not final decides the steps below the largest block boundary E with
E + D <= first_step + nsteps.  decide() walks all windows of a call side by side, one numpy row per window.
"""
import numpy as np

DEFAULTS = (192, 64, 64)
BARRED = -(1 << 30)
PRESETS = {"2/3": (2, (0b01, 0b11)), "3/4": (3, (0b101, 0b011)), "5/6": (5, (0b10101, 0b01011)), "7/8": (7, (0b1010001, 0b0101111))}


class Code:
    def __init__(self, K, gens, period=1, keep=None, init_state=0, terminated=False):
        self.K, self.gens, self.n, self.ns = K, list(gens), len(gens), 1 << (K - 1)
        self.period = period
        self.keep = list(keep) if keep is not None else [(1 << period) - 1] * self.n
        self.init_state, self.terminated = init_state & (self.ns - 1), terminated
        # kept[r]: the coded bits a step at place r of the period transmits; cum[r]: the bits of the places below r
        self.kept = [[i for i in range(self.n) if self.keep[i] >> r & 1] for r in range(period)]
        assert all(self.kept), "a step transmits nothing"
        self.cum = np.concatenate([[0], np.cumsum([len(k) for k in self.kept])]).astype(np.int64)
        self.ptot = int(self.cum[-1])
        # sign[c][h'][i] = d(c_i) of the transition into h' from its predecessor c
        self.pred = np.array([[(hp >> 1) | (c << (K - 2)) for hp in range(self.ns)] for c in (0, 1)])
        self.sign = np.array([[[2 * b - 1 for b in self.code_bits(int(self.pred[c][hp]), hp & 1)] for hp in range(self.ns)] for c in (0, 1)],
                             dtype=np.int64)

    def code_bits(self, h, b):
        r = (h << 1) | b
        return [sum((r >> j & 1) & (g >> (self.K - 1 - j) & 1) for j in range(self.K)) & 1 for g in self.gens]

    @property
    def rate(self):
        return self.period / self.ptot


def geometry(B=0, W=0, D=0):
    return (B or DEFAULTS[0], W or DEFAULTS[1], D or DEFAULTS[2])


def valid_geometry(B, W, D):
    return 1 <= B and 1 <= W <= 128 and D <= 128 and B + W + D <= 512


def idx(code, t):
    return t // code.period * code.ptot + int(code.cum[t % code.period])


def encode(code, bits, first=0, state=None):
    """(transmitted bits uint8, state behind the last step) of the input bits of the steps [first, first + len(bits))."""
    h = code.init_state if state is None else state & (code.ns - 1)
    out = []
    for k, b in enumerate(bits):
        c = code.code_bits(h, int(b))
        out += [c[i] for i in code.kept[(first + k) % code.period]]
        h = ((h << 1) | int(b)) & (code.ns - 1)
    return np.array(out, dtype=np.uint8), h


def nsteps_of(code, nin, first=0):
    """The largest T with idx(first + T) - idx(first) <= nin."""
    x = idx(code, first) + nin
    t = x // code.ptot * code.period
    while idx(code, t + 1) <= x:
        t += 1
    return t - first


def ndecided(nsteps, first=0, final=True, B=0, W=0, D=0):
    B, W, D = geometry(B, W, D)
    if final:
        return nsteps
    end = first + nsteps
    if end < D:
        return 0
    return max(0, (end - D) // B * B - first)


def nbefore_wanted(code, first, B=0, W=0, D=0):
    B, W, D = geometry(B, W, D)
    return idx(code, first) - idx(code, max(0, first // B * B - W))


def plan(code, nin, first=0, final=True, B=0, W=0, D=0):
    """(nsteps, ndecided, nbefore_wanted) of bbb_conv_plan."""
    ns = nsteps_of(code, nin, first)
    return ns, ndecided(ns, first, final, B, W, D), nbefore_wanted(code, first, B, W, D)


def step_values(code, vals, nbefore, first, t_lo, t_hi):
    """r[T - t_lo][i] for the steps T in [t_lo, t_hi): vals[nbefore] is received value idx(first); a punctured position and a
    value outside vals are 0."""
    vals = np.asarray(vals, dtype=np.int64)
    r = np.zeros((max(0, t_hi - t_lo), code.n), dtype=np.int64)
    base = idx(code, first) - nbefore
    for T in range(t_lo, t_hi):
        x = idx(code, T) - base
        for i in code.kept[T % code.period]:
            if 0 <= x < len(vals):
                r[T - t_lo, i] = vals[x]
            x += 1
    return r


def _walk(code, R, length, start_barred, forced):
    """R [nwin, L, n], length [nwin] the steps each window walks, start_barred [nwin]: the window starts at step 0, forced
    [nwin]: it ends in state 0.  (decisions [nwin, L], end metric [nwin])."""
    nwin, L, _ = R.shape
    rows = np.arange(nwin)
    m = np.zeros((nwin, code.ns), dtype=np.int64)
    barred = np.full(code.ns, BARRED, dtype=np.int64)
    barred[code.init_state] = 0
    m[start_barred] = barred
    surv = np.zeros((L, nwin, code.ns), dtype=np.int64)
    for s in range(L):
        c0 = m[:, code.pred[0]] + R[:, s, :] @ code.sign[0].T
        c1 = m[:, code.pred[1]] + R[:, s, :] @ code.sign[1].T
        c = c1 > c0
        m = np.where((s < length)[:, None], np.where(c, c1, c0), m)
        surv[s] = c
    state = np.argmax(m, axis=1)                     # the first of the largest: the lowest index
    state[forced] = 0
    total = m[rows, state]
    bits = np.zeros((nwin, L), dtype=np.uint8)
    for s in range(L - 1, -1, -1):
        act = s < length
        bits[:, s] = state & 1
        state = np.where(act, (state >> 1) | (surv[s, rows, state] << (code.K - 2)), state)
    return bits, total


def viterbi(code, r, start=True):
    """One window over the values r [steps, n]: (decisions, total gain of the path).  start: the window starts at step 0."""
    r = np.asarray(r, dtype=np.int64).reshape(1, -1, code.n)
    bits, total = _walk(code, r, np.array([r.shape[1]]), np.array([bool(start)]), np.array([False]))
    return bits[0].tolist(), int(total[0])


def path_gain(code, r, bits, start=None):
    h, total = code.init_state if start is None else start, 0
    for rv, b in zip(r, bits):
        total += sum(int(v) * (2 * c - 1) for v, c in zip(rv, code.code_bits(h, b)))
        h = ((h << 1) | b) & (code.ns - 1)
    return total


def decide(code, r, t_lo, first, nsteps, final=True, B=0, W=0, D=0):
    """(bits uint8, windows walked) of a call over the steps [first, first + nsteps) whose values r[T - t_lo], T >= t_lo, are given
    (t_lo <= first: its history)."""
    B, W, D = geometry(B, W, D)
    assert valid_geometry(B, W, D)
    nd = ndecided(nsteps, first, final, B, W, D)
    bits = np.zeros(nd, dtype=np.uint8)
    if not nd:
        return bits, 0
    end = first + nsteps
    js = range(first // B, (first + nd - 1) // B + 1)
    wins = [(max(0, j * B - W), min(end, (j + 1) * B + D)) for j in js]
    assert wins[0][0] >= t_lo, "the history does not reach the window's first step"
    L = max(hi - lo for lo, hi in wins)
    R = np.zeros((len(wins), L, code.n), dtype=np.int64)
    for k, (lo, hi) in enumerate(wins):
        R[k, :hi - lo] = r[lo - t_lo:hi - t_lo]
    d, _ = _walk(code, R, np.array([hi - lo for lo, hi in wins]), np.array([lo == 0 for lo, _ in wins]),
                 np.array([bool(code.terminated and final and hi == end) for _, hi in wins]))
    for k, j in enumerate(js):
        lo = wins[k][0]
        e_lo, e_hi = max(j * B, first), min((j + 1) * B, first + nd)
        bits[e_lo - first:e_hi - first] = d[k, e_lo - lo:e_hi - lo]
    return bits, len(wins)


def run(code, vals, nbefore=0, first=0, final=True, B=0, W=0, D=0, hard=False):
    """(bits uint8, windows walked) of one call: vals[nbefore:] are the call's received values (int16 values, or bits 0 / 1 with
    hard), vals[:nbefore] the history in front of them."""
    vals = np.asarray(vals, dtype=np.int64)
    if hard:
        vals = 2 * vals - 1
    Bq, Wq, _ = geometry(B, W, D)
    nsteps = nsteps_of(code, len(vals) - nbefore, first)
    t_lo = max(0, first // Bq * Bq - Wq)
    r = step_values(code, vals[:nbefore + idx(code, first + nsteps) - idx(code, first)], nbefore, first, t_lo, first + nsteps)
    return decide(code, r, t_lo, first, nsteps, final, B, W, D)


def stream(code, vals, cuts, B=0, W=0, D=0, hard=False):
    """The record handed over piece by piece as ConvStream does: every push is a call that is not final over the values not
    yet decided, behind nbefore_wanted values of history; finish is the final call."""
    vals = np.asarray(vals, dtype=np.int64)
    edges = [0] + list(cuts) + [len(vals)]
    out, first, start = [], 0, 0                    # start: the index of received value idx(first)
    for i, hi in enumerate(edges[1:]):
        final = i == len(edges) - 2
        nb = min(start, nbefore_wanted(code, first, B, W, D))
        bits, _ = run(code, vals[start - nb:hi], nb, first, final, B, W, D, hard)
        out.append(bits)
        start += idx(code, first + len(bits)) - idx(code, first)
        first += len(bits)
    return np.concatenate(out)


def free_distance(code):
    """The least weight of the transmitted bits of a path that leaves state 0 and returns to it, over every place of the period
    at which it may leave."""
    best = None
    for phase in range(code.period):
        front = {}
        c = code.code_bits(0, 1)
        front[1 & (code.ns - 1)] = sum(c[i] for i in code.kept[phase])
        t = phase + 1
        for _ in range(40 * code.K):
            nxt = {}
            for h, wgt in front.items():
                for b in (0, 1):
                    cb = code.code_bits(h, b)
                    w2 = wgt + sum(cb[i] for i in code.kept[t % code.period])
                    h2 = ((h << 1) | b) & (code.ns - 1)
                    if h2 == 0:
                        best = w2 if best is None else min(best, w2)
                    elif w2 < nxt.get(h2, 1 << 30) and (best is None or w2 < best):
                        nxt[h2] = w2
            front, t = nxt, t + 1
            if not front:
                break
    return best


# The closed loop (tests/test_conv_host.py computes and asserts these on this model; tests/test_gpu_conv.py holds the GPU to the
# same): 8192 bits of default_rng(25) through (0171, 0133), transmitted bit c sent as (2c - 1) * 64 plus rint of default_rng(26)
# normal noise of the given sigma, default geometry, not terminated.  A hard decision is value >= 0, RX.slice's rule (with > 0 the
# channel and hard counts are 933 / 24 and 242 / 141: the 44 and 15 values that are exactly 0 decide it).
LOOP = {"1/2": dict(puncture=None, sigma=40), "3/4": dict(puncture="3/4", sigma=32)}
LOOP_COUNTS = {"1/2": dict(ncoded=16384, channel=925, hard=34, soft=3), "3/4": dict(ncoded=10923, channel=245, hard=132, soft=0)}

_loop = {}


def loop_record(name):
    """(code, data bits, transmitted bits, received int16 values) of a closed-loop case, computed once."""
    if name not in _loop:
        L = LOOP[name]
        period, keep = PRESETS[L["puncture"]] if L["puncture"] else (1, None)
        code = Code(7, (0o171, 0o133), period, keep)
        bits = np.random.default_rng(25).integers(0, 2, 8192)
        tx, _ = encode(code, bits)
        rx = (2 * tx.astype(np.int64) - 1) * 64 + np.rint(np.random.default_rng(26).normal(0, L["sigma"], len(tx))).astype(np.int64)
        _loop[name] = (code, bits, tx, np.clip(rx, -32768, 32767).astype(np.int16))
    return _loop[name]


def loop_counts(name):
    code, bits, tx, rx = loop_record(name)
    hard = (rx >= 0).astype(np.int64)
    return dict(ncoded=len(tx), channel=int((hard != tx).sum()), hard=int((run(code, hard, hard=True)[0] != bits).sum()),
                soft=int((run(code, rx)[0] != bits).sum()))
