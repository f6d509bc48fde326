"""The LDPC codec's definition (include/bbb.h, bbb_ldpc_*) in numpy, with R kept explicitly per edge.

`decode` is vectorised over the codewords and over the rows of a layer (which touch disjoint variables); `decode_serial` is the
definition as a literal loop, check by check, and tests/test_ldpc_host.py asserts the two equal on small codes.  `grid_cases()`
holds the shapes at which the kernel can go wrong; everything that needs an expected value takes it from here.
"""
import functools

import numpy as np

FAILED = 255
SOFT16, HARD = 0, 1


class Code:
    def __init__(self, base, Z, max_iter=20, norm=12, hard_mag=32):
        self.base = [[int(v) for v in row] for row in base]
        self.Z, self.J, self.K = int(Z), len(self.base), len(self.base[0])
        self.max_iter, self.norm, self.hard_mag = max_iter, norm, hard_mag
        self.n, self.m, self.k = self.K * self.Z, self.J * self.Z, (self.K - self.J) * self.Z
        # the edges of block row j by ascending column: (column, shift)
        self.edges = [[(c, s) for c, s in enumerate(row) if s >= 0] for row in self.base]
        r = np.arange(self.Z)
        self.var = [np.array([c * self.Z + (r + s) % self.Z for c, s in e]) for e in self.edges]        # [deg, Z]

    def with_(self, **kw):
        c = Code(self.base, self.Z, self.max_iter, self.norm, self.hard_mag)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    @property
    def triangular(self):
        K, J = self.K, self.J
        return all(self.base[j][K - J + j] >= 0 and all(self.base[j][K - J + i] < 0 for i in range(j)) for j in range(J))


def array_base(p, J, K):
    return [[j * (c + J - j) % p for c in range(K - J)] + [j * (i - j) % p if i >= j else -1 for i in range(J)] for j in range(J)]


def array(p, J, K, **kw):
    return Code(array_base(p, J, K), p, **kw)


def pack(bits):
    """uint8 bits to uint64 words, LSB first, zero-filled."""
    b = np.zeros(-(-len(bits) // 64) * 64, dtype=np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint64)


def unpack(words, nbits):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:nbits]


def encode(code, data):
    """data: uint8 bits [ncw * k]; the coded bits [ncw * n]."""
    Z, J, K = code.Z, code.J, code.K
    assert code.triangular
    d = np.asarray(data, dtype=np.uint8).reshape(-1, code.k)
    x = np.zeros((len(d), code.n), dtype=np.uint8)
    x[:, :code.k] = d
    r = np.arange(Z)
    for j in range(J - 1, -1, -1):
        t = np.zeros((len(d), Z), dtype=np.uint8)
        for c, s in code.edges[j]:
            if c != K - J + j:
                t ^= x[:, c * Z + (r + s) % Z]
        x[:, (K - J + j) * Z + (r + code.base[j][K - J + j]) % Z] = t
    return x.reshape(-1)


def received(code, values, hard):
    """The decoder's r[v] as integers [ncw, n]: int16 soft values, or bits as +-hard_mag."""
    v = np.asarray(values).astype(np.int64)
    if hard:
        v = np.where(v > 0, code.hard_mag, -code.hard_mag)
    return v.reshape(-1, code.n)


def _unsatisfied(code, P):
    """[ncw]: some check of hard(P) is not satisfied."""
    bad = np.zeros(len(P), dtype=bool)
    for V in code.var:
        bad |= np.bitwise_xor.reduce(P[:, V] > 0, axis=1).any(axis=1)
    return bad


def decode(code, values, hard=False):
    """(data bits [ncw * k] uint8, iters [ncw] uint8, stats [5]) of whole codewords."""
    P = np.clip(received(code, values, hard), -32767, 32767)
    first = P > 0
    ncw = len(P)
    R = [np.zeros((ncw, len(e), code.Z), dtype=np.int64) for e in code.edges]
    run = _unsatisfied(code, P)
    iters = np.where(run, FAILED, 0)
    for it in range(code.max_iter):
        idx = np.flatnonzero(run)
        if not len(idx):
            break
        for j, V in enumerate(code.var):
            Q = np.clip(P[idx][:, V] - R[j][idx], -32767, 32767)                    # [na, deg, Z]
            b = Q > 0
            S = np.bitwise_xor.reduce(b, axis=1)
            A = np.abs(Q)
            i1 = A.argmin(axis=1)                                                   # the lowest e among equals
            m1 = A.min(axis=1)
            e = np.arange(A.shape[1])[None, :, None]
            m2 = np.where(e == i1[:, None, :], 1 << 40, A).min(axis=1)
            a = (np.where(e == i1[:, None, :], m2[:, None, :], m1[:, None, :]) * code.norm) >> 4
            Rn = np.where(S[:, None, :] ^ b, a, -a)
            R[j][idx] = Rn
            P[idx[:, None, None], V[None]] = np.clip(Q + Rn, -32767, 32767)
        ok = ~_unsatisfied(code, P[idx])
        iters[idx[ok]] = it + 1
        run[idx[ok]] = False
    conv = iters != FAILED
    stats = [ncw, int((iters == 0).sum()), int((~conv).sum()), int(iters[conv].sum()), int(((P > 0) != first)[conv].sum())]
    return (P[:, :code.k] > 0).astype(np.uint8).reshape(-1), iters.astype(np.uint8), stats


def decode_serial(code, values, hard=False):
    """The definition as written: codeword by codeword, layer by layer, check by check, edge by edge."""
    Z, K = code.Z, code.K
    out, iters, stats = [], [], [0] * 5
    for r_ in received(code, values, hard).tolist():
        P = [max(-32767, min(32767, v)) for v in r_]
        first = [v > 0 for v in P]
        R = {}

        def satisfied():
            for j, edges in enumerate(code.edges):
                for r in range(Z):
                    x = 0
                    for c, s in edges:
                        x ^= P[c * Z + (r + s) % Z] > 0
                    if x:
                        return False
            return True
        res = 0
        if not satisfied():
            res = FAILED
            for it in range(code.max_iter):
                for j, edges in enumerate(code.edges):
                    for r in range(Z):
                        vs = [c * Z + (r + s) % Z for c, s in edges]
                        Q = [max(-32767, min(32767, P[v] - R.get((j, r, e), 0))) for e, v in enumerate(vs)]
                        S = 0
                        for q in Q:
                            S ^= q > 0
                        mags = [abs(q) for q in Q]
                        m1 = min(mags)
                        i1 = mags.index(m1)
                        m2 = min(a for e, a in enumerate(mags) if e != i1)
                        for e, v in enumerate(vs):
                            a = ((m2 if e == i1 else m1) * code.norm) >> 4
                            R[(j, r, e)] = a if S ^ (Q[e] > 0) else -a
                            P[v] = max(-32767, min(32767, Q[e] + R[(j, r, e)]))
                if satisfied():
                    res = it + 1
                    break
        out += [int(v > 0) for v in P[:code.k]]
        iters.append(res)
        stats[0] += 1
        stats[1] += res == 0
        stats[2] += res == FAILED
        if res != FAILED:
            stats[3] += res
            stats[4] += sum(a != (v > 0) for a, v in zip(first, P))
    return np.array(out, dtype=np.uint8), np.array(iters, dtype=np.uint8), stats


def stream(code, values, cuts):
    """The record handed over in the pieces the cuts make, each decoded with what was held back: (data bits, iters, values left
    over at the end)."""
    held = np.zeros(0, dtype=np.int16)
    out, its = [], []
    for a, b in zip([0] + list(cuts), list(cuts) + [len(values)]):
        buf = np.concatenate([held, values[a:b]])
        whole = len(buf) // code.n * code.n
        held = buf[whole:]
        d, i, _ = decode(code, buf[:whole])
        out.append(d)
        its.append(i)
    return np.concatenate(out), np.concatenate(its), len(held)


# ---- the grid --------------------------------------------------------------------------------------------------------------------

def random_base(rng, Z, J, K, triangular=True, density=0.7, force=()):
    """A random base matrix whose parity part is block upper triangular (or, triangular=False, anything), rows of 2..32 entries,
    no empty column; force: (j, c, s) entries put in afterwards."""
    while True:
        base = np.where(rng.random((J, K)) < density, rng.integers(0, Z, (J, K)), -1)
        if triangular:
            for j in range(J):
                base[j, K - J:K - J + j] = -1
                base[j, K - J + j] = rng.integers(0, Z)
        for j, c, s in force:
            base[j, c] = s
        deg = (base >= 0).sum(axis=1)
        if deg.min() >= 2 and deg.max() <= 32 and (base >= 0).any(axis=0).all():
            return base.tolist()


KINDS = ("clean", "light", "heavy", "zero", "extreme", "tie")


def make_case(code, rng, kinds, in_first=0, hard=False, light=34.0):
    """One record: a codeword per entry of `kinds`.  clean: +-64; light: +-64 and noise of sigma `light`; heavy: sigma 150, hopeless;
    zero: all values 0 (erasures); extreme: +32767 / -32768 with a few wrong values of -+100; tie: +-64 with a few signs turned,
    every magnitude equal.  The values lie in_first elements (or bits) behind the buffer's start, behind values that are not theirs."""
    ncw, n, k = len(kinds), code.n, code.k
    data = rng.integers(0, 2, ncw * k).astype(np.uint8) if code.triangular else np.zeros(ncw * k, dtype=np.uint8)
    coded = encode(code, data) if code.triangular else np.zeros(ncw * n, dtype=np.uint8)
    tx = (2 * coded.astype(np.int64) - 1).reshape(ncw, n)
    vals = np.zeros((ncw, n), dtype=np.int64)
    for w, kind in enumerate(kinds):
        flips = np.ones(n, dtype=np.int64)
        flips[rng.choice(n, max(1, n // 60), replace=False)] = -1
        if kind == "clean":
            vals[w] = 64 * tx[w]
        elif kind == "light":
            vals[w] = 64 * tx[w] + np.rint(rng.normal(0.0, light, n))
        elif kind == "heavy":
            vals[w] = 64 * tx[w] + np.rint(rng.normal(0.0, 150.0, n))
        elif kind == "zero":
            vals[w] = 0
        elif kind == "extreme":
            vals[w] = np.where(flips > 0, np.where(tx[w] > 0, 32767, -32768), -100 * tx[w])
        elif kind == "tie":
            vals[w] = 64 * tx[w] * flips
        else:
            raise ValueError(kind)
    vals = np.clip(vals, -32768, 32767).astype(np.int16).reshape(-1)
    if hard:
        vals = (vals > 0).astype(np.uint8)
        buf = np.concatenate([rng.integers(0, 2, in_first).astype(np.uint8), vals])
    else:
        buf = np.concatenate([rng.integers(-300, 300, in_first).astype(np.int16), vals])
    out, iters, stats = decode(code, vals, hard)
    return dict(code=code, ncw=ncw, kinds=kinds, in_first=in_first, hard=hard, values=vals, buf=buf, data=data, coded=coded, out=out,
                iters=iters, stats=stats)


@functools.lru_cache(maxsize=None)
def grid_cases():
    rng = np.random.default_rng(2032)
    mix7 = ("clean", "light", "heavy", "zero", "extreme", "tie", "light")
    a31 = array(31, 3, 6)                                                          # k = 93: no whole words anywhere
    cases = []

    def add(code, kinds, **kw):
        cases.append(make_case(code, rng, kinds, **kw))
    # the small array code: every kind, starts that are odd and no multiple of 8, the decoder's settings at their ends
    add(a31, mix7)
    add(a31, mix7, in_first=3)
    add(a31, ("light", "clean", "heavy"), in_first=13)
    add(a31, ("heavy", "light", "light", "clean", "light", "heavy", "tie", "extreme", "zero"), in_first=2)     # nine: a ragged second group
    add(a31.with_(max_iter=1), ("light", "tie", "clean", "heavy", "light"), in_first=1)
    add(a31.with_(max_iter=64), ("light", "heavy", "tie", "clean"), light=38.0)
    add(a31.with_(norm=1), ("light", "tie", "heavy", "extreme"))
    add(a31.with_(norm=16), ("light", "tie", "heavy", "extreme", "clean"), in_first=5)
    # a group in which one codeword converges at once and its neighbour fails (G = 8 here, G = 2 below)
    add(a31, ("clean", "heavy", "clean", "heavy", "zero", "heavy", "light", "heavy"))
    # HARD: bit offsets that straddle words, the magnitude at its ends
    add(a31, mix7, hard=True)
    add(a31, ("tie", "clean", "tie", "heavy", "tie"), hard=True, in_first=5)
    add(a31.with_(hard_mag=1), ("tie", "tie", "clean", "heavy"), hard=True, in_first=67)
    add(a31.with_(hard_mag=32767), ("tie", "heavy", "tie", "clean"), hard=True, in_first=63)
    # Z at and around the wave and the workgroup: 2 (sixteen codewords a group), 63, 64, 65, 127 (two a group), 511, 512
    add(Code(random_base(rng, 2, 2, 5, density=0.9), 2), ("clean", "tie", "heavy", "zero", "tie", "extreme", "tie", "heavy", "clean"), in_first=1)
    add(Code(random_base(rng, 2, 3, 7, density=0.9), 2), ("tie",) * 5 + ("heavy", "clean", "heavy", "tie"), hard=True, in_first=9)
    for Z, J, K in ((63, 3, 8), (64, 3, 8), (65, 3, 7)):
        add(Code(random_base(rng, Z, J, K, force=((0, 0, 0), (1, 1, Z - 1))), Z), ("light", "clean", "heavy", "tie", "extreme"), in_first=Z % 8 + 1)
    add(array(127, 4, 16), ("clean", "heavy", "light", "heavy", "light"), in_first=7)
    add(array(127, 4, 16), ("light", "light", "tie"), hard=True, in_first=129)
    add(Code(random_base(rng, 511, 2, 6, force=((0, 1, 510), (1, 0, 0))), 511), ("light", "heavy", "clean"), in_first=3, light=22.0)
    add(Code(random_base(rng, 512, 3, 7, force=((0, 0, 511), (2, 1, 0))), 512), ("tie", "light", "heavy"), in_first=11, light=22.0)
    # the LDS maxima: n = 16384 and m = 8192
    add(Code(random_base(rng, 512, 16, 32, density=0.25, force=((0, 0, 0), (15, 3, 511))), 512), ("light", "clean", "heavy"), in_first=1, light=24.0)
    add(Code(random_base(rng, 256, 32, 64, density=0.12), 256), ("light", "heavy", "zero"), in_first=6, light=24.0)      # J = 32, K = 64
    # J = 1; row degrees 2 and 32; K = 64
    add(Code(random_base(rng, 31, 1, 8, density=1.0), 31), ("light", "tie", "clean", "heavy", "extreme"), in_first=3)
    add(Code([[4, 9, -1], [0, -1, 30]], 31), ("light", "tie", "heavy", "clean"), in_first=1)
    row0 = [int(s) for s in rng.integers(0, 16, 31)] + [-1] * 31 + [15, -1]
    row1 = [-1] * 31 + [int(s) for s in rng.integers(0, 16, 31)] + [-1, 0]
    add(Code([row0, row1], 16), ("tie", "light", "heavy", "clean", "extreme", "zero", "tie"), in_first=5)
    add(Code([row0, row1], 16), ("tie", "heavy", "tie", "clean"), hard=True, in_first=77)
    # a random base that is not triangular: the decoder takes it, the encoder does not (the all-zero codeword is sent)
    nt = random_base(rng, 31, 3, 7, triangular=False, force=((2, 4, 3), (1, 5, 0), (2, 5, 30)))
    assert not Code(nt, 31).triangular
    add(Code(nt, 31), ("light", "clean", "heavy", "tie", "zero"), in_first=9)
    add(Code(nt, 31), ("tie", "heavy", "clean"), hard=True, in_first=33)
    return cases


# ---- the closed loop: encode, BPSK at +-64, Gaussian noise, decode -------------------------------------------------------------

LOOP = dict(p=127, J=4, K=16, ncw=40, amp=64, seed=127)
# loop_counts(sigma, hard) with the seeds above: channel = hard-decision errors among all coded bits; data = data-bit errors
# behind the decoder; failed = codewords with iters 255; iters = the sum over the converged codewords
LOOP_COUNTS = {
    (32, False): dict(channel=1860, data=0, failed=0, iters=112),
    (40, False): dict(channel=4447, data=1211, failed=34, iters=64),
    (32, True): dict(channel=1860, data=194, failed=17, iters=191),
}


def loop_record(sigma):
    """(code, data bits, int16 values) of the loop's record at this sigma."""
    code = array(LOOP["p"], LOOP["J"], LOOP["K"])
    rng = np.random.default_rng(LOOP["seed"])
    data = rng.integers(0, 2, LOOP["ncw"] * code.k).astype(np.uint8)
    coded = encode(code, data)
    noise = np.random.default_rng(LOOP["seed"] + 1).normal(0.0, 1.0, len(coded))
    vals = np.clip(np.rint((2 * coded.astype(np.int64) - 1) * LOOP["amp"] + sigma * noise), -32768, 32767).astype(np.int16)
    return code, data, coded, vals


def loop_counts(sigma, hard=False, decoder=None):
    code, data, coded, vals = loop_record(sigma)
    rx = (vals > 0).astype(np.uint8)
    out, iters, stats = (decoder or decode)(code, rx if hard else vals, hard)
    return dict(channel=int((rx != coded).sum()), data=int((out != data).sum()), failed=int((iters == FAILED).sum()), iters=stats[3])
