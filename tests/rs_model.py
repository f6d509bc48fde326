"""A serial model of the Reed-Solomon codec of include/bbb.h (bbb_rs_*), written from the definition with plain Python ints and
without anything of the C code: its own field (shift and xor, tables of its own making), the generator multiplied out, the
encoder as the remainder of a long division, and a bounded-distance decoder -- Berlekamp-Massey in its textbook form, the roots
by trying every stored position, the error values by SOLVING the syndrome equations (Gaussian elimination, not Forney's
formula), and a last check that is the definition itself: the corrected word must have all-zero syndromes and differ from
the received one in at most t symbols, else the word failed.  tests/test_rs_host.py holds this model to an exhaustive search.

Symbol 0 of a codeword is the coefficient of x^(n-1); the k data symbols come first.  A coded frame of depth I is I n bytes,
byte j symbol j // I of codeword j % I; a data frame is its first I k bytes.
"""
import numpy as np

FAILED = 255


def gf_mul(poly, a, b):
    """a b in GF(2^8) modulo poly, by shift and xor."""
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a & 0x100:
            a ^= poly
        b >>= 1
    return r


def is_primitive(poly):
    if poly >> 9 or not poly >> 8:
        return False
    x, seen = 1, set()
    for _ in range(255):
        if x in seen or x == 0:
            return False
        seen.add(x)
        x = gf_mul(poly, x, 2)
    return x == 1


class Code:
    def __init__(self, n=255, k=223, prim_poly=0x11D, fcr=0, prim=1, depth=1):
        self.n, self.k, self.prim_poly, self.fcr, self.prim, self.depth = n, k, prim_poly, fcr, prim, depth
        self.nroots, self.t = n - k, (n - k) // 2
        assert is_primitive(prim_poly) and self.nroots % 2 == 0 and 2 <= self.nroots <= 32 and k >= 1 and n <= 255
        self.exp, self.log, x = [0] * 510, [0] * 256, 1
        for i in range(255):
            self.exp[i] = self.exp[i + 255] = x
            self.log[x] = i
            x = gf_mul(prim_poly, x, 2)
        self.roots = [self.exp[prim * (fcr + i) % 255] for i in range(self.nroots)]
        g = [1]                                     # highest power first
        for r in self.roots:
            g = [a ^ self.mul(b, r) for a, b in zip(g + [0], [0] + g)]
        self.gen = g

    def mul(self, a, b):
        return self.exp[self.log[a] + self.log[b]] if a and b else 0

    def inv(self, a):
        return self.exp[255 - self.log[a]]

    def eval(self, word, x):
        """word (highest power first) at x, by Horner."""
        v = 0
        for c in word:
            v = self.mul(v, x) ^ c
        return v

    @property
    def frame_bytes(self):
        return self.depth * self.n

    @property
    def data_bytes(self):
        return self.depth * self.k


def ccsds(depth=1, k=223):
    return Code(255, k, 0x187, 112 if k == 223 else 120, 11, depth)


def dvb():
    return Code(204, 188, 0x11D, 0, 1, 1)


def encode_word(code, data):
    """The n symbols of the codeword of k data symbols: data, then the remainder of data(x) x^nroots by g(x)."""
    rem = list(data) + [0] * code.nroots
    for i in range(code.k):
        f = rem[i]
        if f:
            for j in range(1, code.nroots + 1):
                rem[i + j] ^= code.mul(f, code.gen[j])
    return list(data) + rem[code.k:]


def syndromes(code, word):
    return [code.eval(word, r) for r in code.roots]


def _solve(code, rows, rhs):
    """The solution of a square system over the field, or None."""
    m = len(rows)
    a = [list(r) + [b] for r, b in zip(rows, rhs)]
    for c in range(m):
        p = next((r for r in range(c, m) if a[r][c]), None)
        if p is None:
            return None
        a[c], a[p] = a[p], a[c]
        iv = code.inv(a[c][c])
        a[c] = [code.mul(v, iv) for v in a[c]]
        for r in range(m):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [v ^ code.mul(f, w) for v, w in zip(a[r], a[c])]
    return [a[r][m] for r in range(m)]


def decode_word(code, recv):
    """(word, nerr): the codeword within t symbols of recv and how many symbols differ, or (recv, FAILED)."""
    recv = list(recv)
    S = syndromes(code, recv)
    if not any(S):
        return recv, 0
    C, B, L, m, b = [1], [1], 0, 1, 1               # lowest power first
    for k in range(code.nroots):
        d = S[k]
        for i in range(1, L + 1):
            if i < len(C):
                d ^= code.mul(C[i], S[k - i])
        if d == 0:
            m += 1
            continue
        T = list(C)
        f = code.mul(d, code.inv(b))
        C = C + [0] * (len(B) + m - len(C))
        for i, v in enumerate(B):
            C[i + m] ^= code.mul(f, v)
        if 2 * L <= k:
            L, B, b, m = k + 1 - L, T, d, 1
        else:
            m += 1
    if L > code.t:
        return recv, FAILED
    beta = code.exp[code.prim]
    pos = []
    for s in range(code.n):
        X = code.exp[code.log[beta] * (code.n - 1 - s) % 255]
        if code.eval(C[::-1], code.inv(X)) == 0:
            pos.append(s)
    if len(pos) != L:
        return recv, FAILED
    # S_i = sum_k e_k X_k^(fcr + i): L unknowns, the first L equations
    X = [code.exp[code.log[beta] * (code.n - 1 - s) % 255] for s in pos]
    rows = [[code.exp[code.log[x] * (code.fcr + i) % 255] for x in X] for i in range(L)]
    e = _solve(code, rows, S[:L])
    if e is None:
        return recv, FAILED
    word = list(recv)
    for s, v in zip(pos, e):
        word[s] ^= v
    nerr = sum(1 for a, c in zip(recv, word) if a != c)
    if any(syndromes(code, word)) or nerr > code.t:
        return recv, FAILED
    return word, nerr


def encode(code, data):
    """Coded frames (uint8 array) of whole data frames."""
    data = np.asarray(data, dtype=np.uint8)
    I, n, k = code.depth, code.n, code.k
    assert len(data) % (I * k) == 0
    out = np.zeros(len(data) // (I * k) * I * n, dtype=np.uint8)
    for f in range(len(data) // (I * k)):
        fr = data[f * I * k:(f + 1) * I * k]
        for c in range(I):
            out[f * I * n + c:(f + 1) * I * n:I] = encode_word(code, fr[c::I].tolist())
    return out


def decode(code, coded):
    """(data uint8, nerr uint8 per codeword at f I + c, stats [codewords, clean, failed, symbols corrected, bits corrected])."""
    coded = np.asarray(coded, dtype=np.uint8)
    I, n, k = code.depth, code.n, code.k
    assert len(coded) % (I * n) == 0
    nf = len(coded) // (I * n)
    data, nerr, stats = np.zeros(nf * I * k, dtype=np.uint8), np.zeros(nf * I, dtype=np.uint8), [0] * 5
    for f in range(nf):
        fr = coded[f * I * n:(f + 1) * I * n]
        for c in range(I):
            recv = fr[c::I].tolist()
            word, ne = decode_word(code, recv)
            data[f * I * k + c:(f + 1) * I * k:I] = word[:k]
            nerr[f * I + c] = ne
            stats[0] += 1
            stats[1] += int(ne == 0)
            stats[2] += int(ne == FAILED)
            if ne != FAILED:
                stats[3] += int(ne)
                stats[4] += sum(bin(a ^ b).count("1") for a, b in zip(recv, word))
    return data, nerr, stats


def stream(code, coded, cuts):
    """The record handed over in pieces cut at `cuts` (byte offsets), as fec.RSStream holds back an incomplete frame: the
    concatenated data and nerr of the pieces, and the bytes still held at the end."""
    held, data, nerr = np.zeros(0, dtype=np.uint8), [], []
    edges = [0] + list(cuts) + [len(coded)]
    for lo, hi in zip(edges[:-1], edges[1:]):
        buf = np.concatenate([held, np.asarray(coded[lo:hi], dtype=np.uint8)])
        whole = len(buf) // code.frame_bytes * code.frame_bytes
        d, e, _ = decode(code, buf[:whole])
        data.append(d)
        nerr.append(e)
        held = buf[whole:]
    return np.concatenate(data), np.concatenate(nerr), len(held)


def prbs_bits(k, nbits, tap, state=1):
    """The project's PRBS-k from `state` (the feedback of bits k and tap, the new bit shifted in at the bottom)."""
    out = np.zeros(nbits, dtype=np.uint8)
    mask = (1 << k) - 1
    for i in range(nbits):
        bit = ((state >> (k - 1)) ^ (state >> (tap - 1))) & 1
        state = ((state << 1) | bit) & mask
        out[i] = bit
    return out


# The closed loop (tests/test_rs_host.py computes and asserts these on the two models; tests/test_gpu_rs.py holds the GPU to the
# same): 16 frames of CCSDS (255, 223) at depth 4 whose data bytes are the first 16 * 4 * 223 * 8 bits of PRBS-31 (bit 8j + i of
# the stream is bit i of byte j), and the same bytes as 64 frames at depth 1; the coded bytes' bits through (0171, 0133) at rate
# 1/2 from step 0, not terminated, transmitted bit c sent as (2c - 1) * 64 plus rint of default_rng(43) normal noise of sigma
# 42; hard decisions value >= 0 (RX.slice's rule), the Viterbi decoder of conv_model with its default geometry, then this
# model.  channel / viterbi are bit errors in front of and behind the Viterbi decoder, failed the codewords that failed,
# data_bits the wrong data bits left, symbols the symbols corrected, worst the most symbols corrected in one codeword.
LOOP = dict(frames=16, depth=4, sigma=42, prbs=(31, 28), seed=43)
LOOP_COUNTS = {4: dict(channel=16522, viterbi=1204, failed=0, data_bits=0, symbols=406, worst=12),
               1: dict(channel=16531, viterbi=1254, failed=2, data_bits=103, symbols=382, worst=16)}

_loop = {}


def loop_record(depth):
    """(rs code, data bytes, coded bytes, transmitted bits, received int16 values) of the closed loop at a depth, computed once."""
    import conv_model
    if depth not in _loop:
        code = ccsds(depth)
        nbytes = LOOP["frames"] * LOOP["depth"] * code.k
        data = np.packbits(prbs_bits(LOOP["prbs"][0], 8 * nbytes, LOOP["prbs"][1]), bitorder="little")
        coded = encode(code, data)
        inner = conv_model.Code(7, (0o171, 0o133))
        tx, _ = conv_model.encode(inner, np.unpackbits(coded, bitorder="little"))
        rx = (2 * tx.astype(np.int64) - 1) * 64 + np.rint(np.random.default_rng(LOOP["seed"]).normal(0, LOOP["sigma"], len(tx))).astype(np.int64)
        _loop[depth] = (code, data, coded, tx, np.clip(rx, -32768, 32767).astype(np.int16))
    return _loop[depth]


def loop_counts(depth):
    import conv_model
    code, data, coded, tx, rx = loop_record(depth)
    hard = (rx >= 0).astype(np.int64)
    bits, _ = conv_model.run(conv_model.Code(7, (0o171, 0o133)), hard, hard=True)
    got = np.packbits(bits.astype(np.uint8), bitorder="little")
    out, nerr, stats = decode(code, got)
    ok = nerr[nerr != FAILED]
    return dict(channel=int((hard != tx).sum()), viterbi=int((bits != np.unpackbits(coded, bitorder="little")).sum()), failed=int(stats[2]),
                data_bits=int(np.unpackbits(out ^ data).sum()), symbols=int(stats[3]), worst=int(ok.max()) if len(ok) else 0)


# ---- the cases both test files walk (tests/test_rs_host.py on the host entry points and the lane core, tests/test_gpu_rs.py
# on the GPU), with what this model says of them, computed once ---------------------------------------------------------------
FIELDS = (0x11D, 0x187, 0x12B)
PATTERNS = ("clean", "one", "t", "t+1", "symbol 0", "symbol n-1", "parity only", "all zero", "all 0xFF", "half")

_cases = []


def damage(code, rng, word, pattern):
    """A received word: the codeword `word` with the errors of `pattern`."""
    n, t = code.n, code.t
    word = list(word)

    def hit(places):
        for s in places:
            word[s] ^= int(rng.integers(1, 256))

    if pattern == "one":
        hit([int(rng.integers(0, n))])
    elif pattern == "t":
        hit(rng.choice(n, t, replace=False).tolist())
    elif pattern == "t+1":
        hit(rng.choice(n, min(n, t + 1), replace=False).tolist())
    elif pattern == "symbol 0":
        hit([0] + (1 + rng.choice(n - 1, int(rng.integers(0, t)), replace=False)).tolist())
    elif pattern == "symbol n-1":
        hit([n - 1] + rng.choice(n - 1, int(rng.integers(0, t)), replace=False).tolist())
    elif pattern == "parity only":
        hit((code.k + rng.choice(code.nroots, t, replace=False)).tolist())
    elif pattern == "all zero":
        word = [0] * n
    elif pattern == "all 0xFF":
        word = [255] * n
    elif pattern == "half":
        hit(rng.choice(n, max(1, n // 2), replace=False).tolist())
    return word


def make_case(code, rng, nframes, patterns):
    """A record of nframes frames whose codeword number i (f I + c) carries patterns[i % len(patterns)], and the model's answer."""
    data = rng.integers(0, 256, nframes * code.data_bytes).astype(np.uint8)
    coded = encode(code, data)
    recv = coded.copy()
    I, n = code.depth, code.n
    for f in range(nframes):
        for c in range(I):
            sl = slice(f * I * n + c, (f + 1) * I * n, I)
            recv[sl] = damage(code, rng, coded[sl].tolist(), patterns[(f * I + c) % len(patterns)])
    out, nerr, stats = decode(code, recv)
    return dict(code=code, nframes=nframes, data=data, coded=coded, recv=recv, out=out, nerr=nerr, stats=stats)


def grid_cases():
    """Every (nroots, n) of the grid once, the fields, fcr, prim and depths dealt round so that each meets each nroots; every
    record long enough for all ten patterns; and nroots = 2 at n = 255 with two errors in every codeword."""
    if not _cases:
        rng = np.random.default_rng(41)
        i = 0
        for nroots in (2, 4, 16, 32):
            for n in sorted({nroots + 1, 4, 5, 63, 64, 65, 204, 252, 253, 254, 255}):
                if n <= nroots:
                    continue
                depth = (1, 3, 8)[i % 3]
                code = Code(n, n - nroots, FIELDS[(i // 3) % 3], (0, 1, 112)[(i + i // 9) % 3], (1, 11)[(i + i // 2) % 2], depth)
                shift = i % len(PATTERNS)
                _cases.append(make_case(code, rng, -(-len(PATTERNS) // depth), PATTERNS[shift:] + PATTERNS[:shift]))
                i += 1
        two = Code(255, 253, 0x11D, 0, 1, 8)
        case = make_case(two, rng, 8, ("clean",))
        for w in range(64):
            for s in rng.choice(255, 2, replace=False).tolist():
                case["recv"][(w // 8) * 8 * 255 + s * 8 + w % 8] ^= int(rng.integers(1, 256))
        case["out"], case["nerr"], case["stats"] = decode(two, case["recv"])
        _cases.append(case)
    return _cases
