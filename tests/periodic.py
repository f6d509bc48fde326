"""Periodic records: how one call over more than 2^32 items is compared with a serial model, everywhere.

A serial Python model cannot walk 2^32 items, and a few windows would miss an index that wrapped anywhere else.  So a UNIT
of p items is built and modelled on the CPU; the device record is that unit tiled to the wanted length with a ragged tail; one
call takes it; the whole output is compared on the device, chunk by chunk, with the model's output tiled the same way.

Three conditions make that a proof, and the model alone must meet them (tests/test_periodic_host.py asserts them without a GPU,
on the units of the table below, which tests/test_gpu_wide.py imports too):

  1. The model is periodic from period 1 on.  It runs over three periods and the tail; period 2 must equal period 3 in every
     output, the state behind period 1 the state behind period 2 (`Expect.cut`).  Period 0 (windows that start at item 0) and
     the tail are kept on their own.  Counters are linear in the periods (`linear`).
  2. No power of two is a multiple of the period, in any unit the kernel indexes (`odd_factor`): an index that lost a high bit
     is then off by 2^k mod p != 0 places of the unit.
  3. A shifted read meets different data (`assert_shift_shows`): the unit turned by 2^31 mod p and by 2^32 mod p differs from
     itself in more than 90 % of places, and so does the expected output.  Decisions are packed, a word is what a kernel loads
     and stores: they are compared by the 64 bits from every place on, as a word at that place would hold them.

No GPU code runs at import; torch is imported by the device functions alone.
"""
import functools

import numpy as np

P31, P32 = 1 << 31, 1 << 32
CHUNK = 1 << 26                                   # items compared at a time (a multiple of the period below it)


# ---- the conditions, on the CPU ---------------------------------------------------------------------------------------------

def odd_factor(p):
    """p with its factors of two taken out: above 1 exactly when no power of two is a multiple of p."""
    p = int(p)
    assert p > 0
    while p % 2 == 0:
        p //= 2
    return p


def residues(p):
    """(2^31 mod p, 2^32 mod p): where an index that lost bit 31 or bit 32 lands in the unit."""
    return P31 % p, P32 % p


def shift_differs(a, shift, group=1):
    """The fraction of places i of the periodic array `a` (its first axis) at which the `group` items from i on differ from the
    `group` items from i + shift on."""
    a = np.asarray(a)
    a = a.reshape(len(a), -1)
    bad = (a != np.roll(a, -shift, axis=0)).any(axis=1)
    if group > 1:
        c = np.concatenate([[0], np.cumsum(np.concatenate([bad, bad[:group - 1]]))])
        bad = c[group:group + len(bad)] - c[:len(bad)] > 0
    return float(bad.mean())


def assert_shift_shows(a, what, group=1, least=0.9):
    """Conditions 2 and 3 on one periodic array (a unit, or one period of an expected output)."""
    p = len(a)
    assert odd_factor(p) > 1, f"{what}: a power of two is a multiple of the period {p}"
    for r in residues(p):
        assert r != 0
        f = shift_differs(a, r, group)
        assert f > least, f"{what}: turned by {r} of {p} it differs in only {f:.3f} of the places"


def linear(c2, c3, c4):
    """Counters of the model over 2, 3 and 4 periods plus the tail: they must grow by the same amount per period.  Returns
    count(K) for any K >= 2."""
    c2, c3, c4 = (np.asarray(c, dtype=np.int64) for c in (c2, c3, c4))
    per = c3 - c2
    assert np.array_equal(c4 - c3, per), f"counters are not linear in the periods: {c2.tolist()} {c3.tolist()} {c4.tolist()}"
    return lambda K: (c2 + (K - 2) * per).tolist()


class Expect:
    """One output of a periodic record: head (what period 0 gives), period (what every later period gives) and tail."""

    def __init__(self, head, period, tail):
        self.head, self.period, self.tail = head, period, tail

    @classmethod
    def cut(cls, out, bounds, what):
        """From the model's output over three periods and the tail; bounds = the output index at which each of the periods 1,
        2 and 3 starts (3: the tail).  Asserts condition 1."""
        b1, b2, b3 = (int(b) for b in bounds)
        out = np.asarray(out)
        assert 0 < b1 < b2 < b3 <= len(out) and b3 - b2 == b2 - b1, f"{what}: periods of {b2 - b1} and {b3 - b2} outputs"
        assert np.array_equal(out[b1:b2], out[b2:b3]), f"{what}: period 1 differs from period 2"
        t = len(out) - b3
        assert t <= b2 - b1
        return cls(out[:b1].copy(), out[b1:b2].copy(), out[b3:].copy())

    def length(self, K):
        """Outputs of a record of K >= 2 periods and the tail."""
        return len(self.head) + (K - 1) * len(self.period) + len(self.tail)


def periods_past(limit, p, tail):
    """The smallest K for which a record of K periods and the tail carries an index past `limit` with three periods and the
    tail behind it."""
    assert tail < p
    return limit // p + 4


# ---- the device side ----------------------------------------------------------------------------------------------------------

def _plain(t):
    """A view torch.equal and != take: unsigned 16, 32 and 64 bit tensors as their signed kind."""
    import torch
    signed = {torch.uint16: torch.int16, torch.uint32: torch.int32, torch.uint64: torch.int64}
    return t.view(signed[t.dtype]) if t.dtype in signed else t


def to_dev(a, device="cuda:0"):
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed[a.dtype]) if a.dtype in signed else a).to(device)


def tile(unit, n, out=None):
    """A device tensor of n items (first axis) with out[i] = unit[i mod p]: the unit once, then the filled part copied behind
    itself, doubling; every copy is device to device and starts at a multiple of p."""
    import torch
    p = unit.shape[0]
    if out is None:
        out = torch.empty((n,) + tuple(unit.shape[1:]), dtype=unit.dtype, device=unit.device)
    assert out.shape[0] == n and p > 0
    m = min(p, n)
    out[:m] = unit[:m]
    while m < n:
        k = min(m, n - m)
        out[m:m + k] = out[:k]
        m += k
    return out


def assert_same(got, want, at, what):
    """torch.equal of two device tensors; `at` is the index of their first item in the record, for the message."""
    import torch
    if torch.equal(got, want):
        return
    bad = (got != want).reshape(got.shape[0], -1).any(dim=1).nonzero()
    i = int(bad[0])
    raise AssertionError(f"{what}: {bad.numel()} items of [{at}, {at + got.shape[0]}) differ, the first at {at + i}: "
                         f"{got[i].reshape(-1).tolist()} != {want[i].reshape(-1).tolist()}")


def assert_tiled(got, head, period=None, tail=None, what=""):
    """got == head, then period over and over, then tail: torch.equal chunk by chunk, the chunks multiples of the period.
    head, period and tail are numpy arrays (or an Expect in head's place); names the first bad index."""
    if isinstance(head, Expect):
        head, period, tail = head.head, head.period, head.tail
    got = _plain(got)
    h, pp, t = len(head), len(period), len(tail)
    n = got.shape[0]
    assert n >= h + t and pp > 0 and (n - h - t) % pp == 0, f"{what}: {n} items are not {h} + k * {pp} + {t}"
    if h:
        assert_same(got[:h], _plain(to_dev(head, got.device)), 0, what + " head")
    end = n - t
    if end > h:
        reps = max(1, CHUNK // pp)
        ref = tile(_plain(to_dev(period, got.device)), min(reps * pp, end - h))
        for a in range(h, end, reps * pp):
            b = min(end, a + reps * pp)
            assert_same(got[a:b], ref[:b - a], a, what)
    if t:
        assert_same(got[end:], _plain(to_dev(tail, got.device)), end, what + " tail")


def unpack(words, a, b):
    """Bits [a, b) of packed int64 words as a uint8 device tensor (bit t at word t // 64, bit t % 64)."""
    import torch
    w0, w1 = a // 64, (b + 63) // 64
    sh = torch.arange(64, dtype=torch.int64, device=words.device)
    bits = ((words[w0:w1].unsqueeze(1) >> sh) & 1).to(torch.uint8).reshape(-1)
    return bits[a - 64 * w0:b - 64 * w0]


def pack(bits):
    """uint8 bits to uint64 words, zero-filled (numpy)."""
    b = np.zeros(-(-len(bits) // 64) * 64, dtype=np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint64)


def assert_tiled_bits(words, expect, K, what="", chunk_bits=1 << 24):
    """assert_tiled for packed decisions of a record of K periods (period 0 among them) and the tail: the parts of `expect`
    are uint8 bit arrays, and every bit of `words` behind the tail must be 0.  Where head and period are whole words the
    words are compared as they are; where they are not (a per-period count that is no multiple of 64), the words are unpacked
    on the device, chunk by chunk.  Returns the number of decisions."""
    head, period, tail = expect.head, expect.period, expect.tail
    h, pp, t = len(head), len(period), len(tail)
    nw = words.numel()
    end = h + (K - 1) * pp
    assert K >= 2 and nw * 64 >= end + t, f"{what}: {nw} words do not hold {end + t} bits"
    last = np.concatenate([tail, np.zeros(nw * 64 - end - t, dtype=np.uint8)])
    if h % 64 == 0 and pp % 64 == 0:
        assert_tiled(words, pack(head), pack(period), pack(last), what)
        return end + t
    assert_same(unpack(words, 0, h), to_dev(head, words.device), 0, what + " head")
    reps = max(1, chunk_bits // pp)
    ref = tile(to_dev(period, words.device), min(reps * pp, end - h))
    for a in range(h, end, reps * pp):
        b = min(end, a + reps * pp)
        assert_same(unpack(words, a, b), ref[:b - a], a, what)
    assert_same(unpack(words, end, nw * 64), to_dev(last, words.device), end, what + " tail")
    return end + t


# ---- the units: one table for the host test and the GPU test ---------------------------------------------------------------------

UNITS = {
    # L = 24: 384 blocks a period; a BPSK constellation that turns twice a period, with noise
    "carrier": dict(L=24, blocks=384, turns=2, amp=9000, sigma=1500.0, seed=1, init_phase=5000, threshold=3, strict=True,
                    tail=5 * 24 + 7),
    # spb 1: the decision index is the sample index; three default regions a period
    "dfe": dict(spb=1, taps=(3, 1), fb=(1800, -900, 600, 300), period=3 * 4096, amp=1000, seed=1, threshold=-5, tail=1037,
                region=4096, warmup=64),
    # P = 4, L = 64, 192 blocks of timing_model.drift_record: 15 wraps up and 10 down a period, so a period holds 192 * 64 - 5
    # bits, which is no multiple of 64 ...
    "timing_wraps": dict(P=4, L=64, blocks=192, seed=9, amp=2000, hold=2, tail=3 * 256 + 77),
    # ... and a record with ten wraps each way in a period: 192 * 64 bits
    "timing_level": dict(P=4, L=64, blocks=192, seed=31, amp=2000, hold=2, tail=3 * 256 + 77),
    # the 256-thread kernel with four states (tests/test_mlse_host.py, mlse_shape): blocks of 8 symbols, 192 of them a period
    "mlse": dict(spb=1, taps=(2, 1, -1), shift=1, g=(60, 45, -20), geom=(8, 8, 8), period=3 * 512, noise=40, seed=1, init_state=1,
                 tail=8 * 5 + 3),
    # CCSDS (255, 223) frames, 0 .. 18 wrong symbols in a codeword (more than 16: it fails): 61 frames at depth 1, 31 at depth 2
    "rs1": dict(depth=1, frames=61, seed=1, tail_frames=7),
    "rs2": dict(depth=2, frames=31, seed=2, tail_frames=5),
    # frames of 248 bits (a marker of 32 and 27 bytes, randomised), inverted; 61 frames a period: 15128 bits, no whole words
    "framesync": dict(payload_bytes=27, frames=61, seed=1, tol_search=2, tol_lock=6, verify=1, flywheel=2, inverted=True,
                      marker_errors={3: (1,), 17: (0, 9, 31), 40: (2, 3, 5, 7, 11, 13, 17, 19, 23, 29)}, tail_bits=3 * 248 + 100),
    # fcw * p = 0 mod 2^24: the oscillator has the record's period
    "ddc4": dict(period=3 * 4096, fcw=0x2A5 << 12, pa0=0x123456, taps=(2100, -3900, 7000, 12000, 15535, 12000, 7000, -3900, 2100),
                 shift=15, decim=4, phase=1, seed=1, tail=4 * 250 + 3),
    "ddc1": dict(period=3 * 4096, fcw=0x2A5 << 12, pa0=0x123456, taps=(2100, -3900, 7000, 12000, 15535, 12000, 7000, -3900, 2100),
                 shift=15, decim=1, phase=0, seed=2, tail=1003),
    # 5 blocks of 192 steps a period: 15 words in, 20 words out at rate 3/4
    "conv34": dict(K=7, gens=(0o171, 0o133), puncture="3/4", steps=5 * 192, seed=1, flip_every=41, tail=192 + 64 + 31),
    # K = 3 unpunctured for the soft decoder: 1920 int16 values a period
    "conv12": dict(K=3, gens=(0o7, 0o5), puncture=None, steps=5 * 192, seed=2, sigma=40.0, tail=192 + 64 + 31),
}


def _bounds(per):
    return per, 2 * per, 3 * per


@functools.lru_cache(maxsize=None)
def carrier():
    """unit [p, 2] int16; expect: iq, bits, soft, phases; stats(K); state(K)."""
    import carrier_model as M
    u = UNITS["carrier"]
    L, p = u["L"], u["L"] * u["blocks"]
    rng = np.random.default_rng(u["seed"])
    d = rng.integers(0, 2, p) * 2 - 1
    th = 2 * np.pi * (u["turns"] * np.arange(p) / p + 0.05)
    x = np.stack([u["amp"] * d * np.cos(th), u["amp"] * d * np.sin(th)], axis=1) + rng.normal(0.0, u["sigma"], (p, 2))
    unit = np.clip(np.rint(x), -32768, 32767).astype(np.int16)

    def run(K):
        rec = np.concatenate([unit] * K + [unit[:u["tail"]]])
        return M.run(rec, L, u["init_phase"], u["threshold"], u["strict"])
    r2, r3, r4 = run(2), run(3), run(4)
    ex = dict(iq=Expect.cut(r3["iq"], _bounds(p), "carrier iq"), bits=Expect.cut(r3["bits"], _bounds(p), "carrier bits"),
              soft=Expect.cut(r3["soft"], _bounds(p), "carrier soft"),
              phases=Expect.cut(r3["phases"], _bounds(u["blocks"]), "carrier phases"))
    # the estimate behind period 1 is the estimate behind period 2 (the state's first word holds the last one)
    assert r3["phases"][u["blocks"] - 1] == r3["phases"][2 * u["blocks"] - 1] == r3["phases"][3 * u["blocks"] - 1]
    assert r2["state"][0] == r3["state"][0] == r4["state"][0]
    return dict(unit=unit, p=p, tail=u["tail"], expect=ex, stats=linear(r2["stats"], r3["stats"], r4["stats"]),
                state=lambda K: (r3["state"][0], K * p + u["tail"]), per_period=(np.array(r3["stats"]) - np.array(r2["stats"])).tolist())


@functools.lru_cache(maxsize=None)
def dfe():
    """unit int16 [p]; expect: bits, soft; state; stats(K) as the four counters of stats_dev."""
    import dfe_model as M
    import fir_model
    u = UNITS["dfe"]
    p = u["period"]
    unit = np.random.default_rng(u["seed"]).integers(-u["amp"], u["amp"] + 1, p).astype(np.int16)

    def run(K):
        rec = np.concatenate([unit] * K + [unit[:u["tail"]]])
        bits, soft, s = M.run(rec, u["taps"], u["fb"], u["spb"], threshold=u["threshold"])
        st = M.replay(fir_model.acc(rec, u["taps"]), u["fb"], u["threshold"], region=u["region"], warmup=u["warmup"])
        return bits, soft, s, [st[k] for k in ("regions", "not_proven", "repaired", "symbols")]
    r2, r3, r4 = run(2), run(3), run(4)
    ex = dict(bits=Expect.cut(r3[0], _bounds(p), "dfe bits"), soft=Expect.cut(r3[1], _bounds(p), "dfe soft"))
    assert r2[2] == r3[2] == r4[2]
    # the state behind period 1 is the state behind period 2: the last nfb decisions of each
    nfb = len(u["fb"])
    assert np.array_equal(r3[0][p - nfb:p], r3[0][2 * p - nfb:2 * p]) and np.array_equal(r3[0][p - nfb:p], r3[0][3 * p - nfb:3 * p])
    return dict(unit=unit, p=p, tail=u["tail"], expect=ex, state=r3[2], stats=linear(r2[3], r3[3], r4[3]))


def _timing(name):
    import timing_model as M
    u = UNITS[name]
    P, L = u["P"], u["L"]
    p = P * L * u["blocks"]
    unit = M.drift_record(np.random.default_rng(u["seed"]), P, L, p, u["amp"], u["hold"]).astype(np.int16)

    def run(K):
        rec = np.concatenate([unit] * K + [unit[:u["tail"]]])
        return M.run(rec, P, L=L)
    r2, r3, r4 = run(2), run(3), run(4)
    nb = u["blocks"]
    bounds = [int(np.searchsorted(r3["instants"], k * p)) for k in (1, 2, 3)]
    # a wrap down emits a sample in front of its block: where that is a period's first block the bit belongs to the period
    for k in (1, 2, 3):
        if r3["wraps"][k * nb] < 0:
            bounds[k - 1] -= 1
    ex = dict(bits=Expect.cut(r3["bits"], bounds, name + " bits"), soft=Expect.cut(r3["soft"], bounds, name + " soft"),
              phases=Expect.cut(r3["phases"], _bounds(nb), name + " phases"))
    assert r3["phases"][nb - 1] == r3["phases"][2 * nb - 1] == r3["phases"][3 * nb - 1]
    assert r2["state"][0] == r3["state"][0] == r4["state"][0]
    stats = linear(r2["stats"], r3["stats"], r4["stats"])
    nbits = linear([r2["nbits"]], [r3["nbits"]], [r4["nbits"]])
    return dict(unit=unit, p=p, tail=u["tail"], expect=ex, stats=stats, nbits=lambda K: nbits(K)[0],
                state=lambda K: (r3["state"][0], nbits(K)[0]), per_period=(np.array(r3["stats"]) - np.array(r2["stats"])).tolist())


@functools.lru_cache(maxsize=None)
def timing_wraps():
    return _timing("timing_wraps")


@functools.lru_cache(maxsize=None)
def timing_level():
    return _timing("timing_level")


def _ddc(name):
    import ddc_model as M
    u = UNITS[name]
    p = u["period"]
    assert (u["fcw"] * p) % (1 << 24) == 0 and p % u["decim"] == 0
    unit = np.random.default_rng(u["seed"]).integers(-32768, 32768, p).astype(np.int16)
    rec = np.concatenate([unit] * 3 + [unit[:u["tail"]]])
    ex = {}
    for mode, key in ((M.IQ16, "iq"), (M.POLAR, "polar")):
        out = M.ddc(rec, u["fcw"], u["taps"], u["shift"], u["decim"], u["phase"], 0, u["pa0"], mode=mode)
        ex[key] = Expect.cut(out, _bounds(p // u["decim"]), f"{name} {key}")
    return dict(unit=unit, p=p, tail=u["tail"], expect=ex)


@functools.lru_cache(maxsize=None)
def ddc4():
    return _ddc("ddc4")


@functools.lru_cache(maxsize=None)
def ddc1():
    return _ddc("ddc1")


def _conv_code(u):
    import conv_model as M
    period, keep = M.PRESETS[u["puncture"]] if u["puncture"] else (1, None)
    return M.Code(u["K"], u["gens"], period, keep)


@functools.lru_cache(maxsize=None)
def conv34():
    """Rate 3/4, K = 7.  data: the unit of input bits and the encoder's expect; hard: the unit of received bits (the
    period-1 transmitted bits with every flip_every-th wrong: the encoder's state is periodic from period 1 on, so the received
    record is the tiled unit) and the decoder's expect, windows and steps."""
    import conv_model as M
    u = UNITS["conv34"]
    code = _conv_code(u)
    T = u["steps"]
    assert T % 192 == 0 and T % code.period == 0
    data = np.random.default_rng(u["seed"]).integers(0, 2, T).astype(np.uint8)
    rec = np.concatenate([data] * 3 + [data[:u["tail"]]])
    tx, enc_state = M.encode(code, rec)                       # the state behind the record: its last K - 1 bits, whatever K
    per = M.idx(code, T)
    bounds = [M.idx(code, k * T) for k in (1, 2, 3)]
    assert bounds == list(_bounds(per))
    enc = Expect.cut(tx, bounds, "conv34 encode")
    # the encoder's state behind period 1 and behind period 2: the last K - 1 input bits, the same by construction
    rx_unit = enc.period.copy()
    rx_unit[::u["flip_every"]] ^= 1
    ntail = M.idx(code, u["tail"])

    def run(K):
        return M.run(code, np.concatenate([rx_unit] * K + [rx_unit[:ntail]]), hard=True)
    (b2, w2), (b3, w3), (b4, w4) = run(2), run(3), run(4)
    dec = Expect.cut(b3, _bounds(T), "conv34 hard decode")
    assert len(b3) == 3 * T + u["tail"]
    return dict(code=code, data=data, T=T, tail=u["tail"], encode=enc, enc_state=enc_state, rx_unit=rx_unit, rx_tail=ntail, decode=dec,
                stats=linear([w2, len(b2)], [w3, len(b3)], [w4, len(b4)]), errors=int((dec.period != data).sum()))


@functools.lru_cache(maxsize=None)
def conv12():
    """K = 3 unpunctured, soft: the unit of int16 received values (data encoded from the state the data's own end leaves,
    sent as +-64 with noise) and the decoder's expect."""
    import conv_model as M
    u = UNITS["conv12"]
    code = _conv_code(u)
    T = u["steps"]
    rng = np.random.default_rng(u["seed"])
    data = rng.integers(0, 2, T).astype(np.uint8)
    tx, _ = M.encode(code, np.concatenate([data, data]))
    tx = tx[len(tx) // 2:]                                              # period 1: the state in front is the data's own end
    unit = np.clip((2 * tx.astype(np.int64) - 1) * 64 + np.rint(rng.normal(0.0, u["sigma"], len(tx))), -32768, 32767).astype(np.int16)
    ntail = M.idx(code, u["tail"])

    def run(K):
        return M.run(code, np.concatenate([unit] * K + [unit[:ntail]]))
    (b2, w2), (b3, w3), (b4, w4) = run(2), run(3), run(4)
    dec = Expect.cut(b3, _bounds(T), "conv12 soft decode")
    return dict(code=code, data=data, T=T, tail=u["tail"], unit=unit, rx_tail=ntail, decode=dec,
                stats=linear([w2, len(b2)], [w3, len(b3)], [w4, len(b4)]), errors=int((dec.period != data).sum()))


@functools.lru_cache(maxsize=None)
def mlse():
    """unit int16 [p]: +-1 data through the target plus uniform noise, as tests/test_mlse_host.py builds its records; expect of
    the decisions; stats(K) = [windows, symbols]."""
    import mlse_model as M
    u = UNITS["mlse"]
    p, g, (B, W, D) = u["period"], list(u["g"]), u["geom"]
    assert p % B == 0 and u["tail"] < p
    rng = np.random.default_rng(u["seed"])
    d = rng.integers(0, 2, p) * 2 - 1
    unit = rng.integers(-u["noise"], u["noise"] + 1, p)
    for i, v in enumerate(g):
        unit += v * np.roll(d, i)                                        # the data is periodic too
    unit = unit.astype(np.int16)

    def run(K):
        rec = np.concatenate([unit] * K + [unit[:u["tail"]]])
        return M.run(rec, list(u["taps"]), g, u["spb"], 0, u["shift"], init_state=u["init_state"], B=B, W=W, D=D)
    (b2, w2), (b3, w3), (b4, w4) = run(2), run(3), run(4)
    ex = Expect.cut(b3, _bounds(p), "mlse bits")
    return dict(unit=unit, p=p, tail=u["tail"], expect=ex,
                stats=linear([w2, len(b2)], [w3, len(b3)], [w4, len(b4)]))


def _rs(name):
    """recv: the unit of coded bytes as received; out, nerr: what the model decodes from it; coded: the unit as the encoder gives
    it.  Frames do not depend on one another: period 0 is a period like any other, and the counters of K periods and the tail
    are K times the unit's plus those of the tail's frames."""
    import rs_model as M
    u = UNITS[name]
    code = M.ccsds(u["depth"])
    rng = np.random.default_rng(u["seed"])
    nf, I, n = u["frames"], u["depth"], 255
    data = rng.integers(0, 256, nf * code.data_bytes).astype(np.uint8)
    coded = M.encode(code, data)
    recv = coded.copy()
    for w in range(nf * I):
        f, c = divmod(w, I)
        for s in rng.choice(n, int(rng.integers(0, 19)), replace=False).tolist():
            recv[f * I * n + s * I + c] ^= int(rng.integers(1, 256))
    out, nerr, stats = M.decode(code, recv)
    tf = u["tail_frames"]
    out_t, nerr_t, stats_t = M.decode(code, recv[:tf * code.frame_bytes])
    assert np.array_equal(out_t, out[:tf * code.data_bytes]) and np.array_equal(nerr_t, nerr[:tf * I])
    return dict(code=code, data=data, coded=coded, recv=recv, out=out, nerr=nerr, tail_frames=tf, unit_stats=stats,
                stats=lambda K: [K * a + b for a, b in zip(stats, stats_t)])


@functools.lru_cache(maxsize=None)
def rs1():
    return _rs("rs1")


@functools.lru_cache(maxsize=None)
def rs2():
    return _rs("rs2")


def framesync_cfg():
    import framesync_model as M
    u = UNITS["framesync"]
    return M.Cfg(M.CCSDS_MARKER, 32, 32 + 8 * u["payload_bytes"], u["tol_search"], u["tol_lock"], u["verify"], u["flywheel"], True, M.CCSDS_RAND)


@functools.lru_cache(maxsize=None)
def framesync(nbits=None):
    """A stream locked from bit 0 on, nbits long (None: three periods and the table's tail; the GPU test asks for its own sizes,
    the periods are counted from nbits).  payload: the unit of payload bytes; clean: the bits attach makes of it; unit: those
    bits as received, inverted and with the table's marker errors; words: 64 units packed, which is whole words; expect of the
    meta words; K; frames(K), state words(K)."""
    import framesync_model as M
    u = UNITS["framesync"]
    cfg = framesync_cfg()
    U, F = u["frames"], cfg.F
    per = U * F
    payload = np.random.default_rng(u["seed"]).integers(0, 256, U * u["payload_bytes"]).astype(np.uint8)
    clean = M.attach(cfg, payload)
    unit = clean.copy()
    for f, places in u["marker_errors"].items():
        unit[f * F + np.array(places)] ^= 1
    if u["inverted"]:
        unit ^= 1
    K, tail = (3, u["tail_bits"]) if nbits is None else (nbits // per, nbits % per)
    assert K >= 3 and (nbits is None or K * per + tail == nbits)

    def run(k):
        pos, meta, s = M.run(cfg, np.concatenate([unit] * k + [unit[:tail]]))
        assert pos == list(range(0, len(pos) * F, F)) and len(pos) == (k * per + tail) // F
        return np.array(meta, dtype=np.int16), M.words(s)
    (m2, s2), (m3, s3), (m4, s4) = run(2), run(3), run(4)
    ex = Expect.cut(m3, _bounds(U), "framesync meta")
    state = linear(s2, s3, s4)
    return dict(cfg=cfg, payload=payload, clean=clean, unit=unit, words=pack(np.tile(unit, 64)), per=per, K=K, tail=tail, expect=ex,
                frames=(K * per + tail) // F, state=state(K), per_period=(np.array(s3) - np.array(s2)).tolist())


# ---- the capture eye: counts of a tiled record in closed form ---------------------------------------------------------------------

def eye_hist(samples, first, ncols=64, shift=4):
    """hist [256, ncols] of samples numbered from `first` (include/bbb.h: row = 127 - clamp(x >> shift), col = n mod ncols)."""
    x = np.asarray(samples, dtype=np.int64)
    rows = 127 - np.clip(x >> shift, -128, 127)
    cols = (first + np.arange(len(x))) % ncols
    h = np.zeros((256, ncols), dtype=np.int64)
    np.add.at(h, (rows, cols), 1)
    return h


def eye_hist_tiled(unit, first, n, ncols=64, shift=4):
    """hist of the n samples unit[i mod p] numbered first + i: the unit's histogram turned by each period's first column, times
    the periods that start there, and the tail's."""
    p = len(unit)
    K = n // p
    h0 = eye_hist(unit, 0, ncols, shift)
    starts = np.bincount((first + np.arange(K, dtype=np.int64) * p) % ncols, minlength=ncols)
    out = np.zeros_like(h0)
    for c in np.flatnonzero(starts):
        out += int(starts[c]) * np.roll(h0, int(c), axis=1)
    return out + eye_hist(unit[:n - K * p], first + K * p, ncols, shift)
