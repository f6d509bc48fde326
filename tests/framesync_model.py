"""The frame synchroniser's definition (include/bbb.h, bbb_framesync_*) in plain Python and numpy: distances, the SEARCH / LOCK
machine with its decidability rules, the state words, the randomiser, attach and extract.  It shares nothing with the C side.
`brute` is the literal transcription of the two state rules one bit position at a time, for tiny streams, against which
tests/test_framesync_host.py holds `run`.  `grid_cases()` are the cases both test files walk."""
import numpy as np

SEARCH, LOCK = 0, 1
OVERFLOW, ERROR = 1 << 24, 1 << 25
COUNTERS = ("frames", "flywheeled", "acquisitions", "losses", "rejected", "marker_bit_errors")
CCSDS_MARKER, CCSDS_RAND = 0x1DFCCF1A, (0x1A9, 0xFF)


class Cfg:
    def __init__(self, marker, M, F, tol_search=0, tol_lock=None, v=1, w=2, both=True, rand=None):
        self.marker, self.M, self.F, self.tol_search = marker, M, F, tol_search
        self.tol_lock = tol_search if tol_lock is None else tol_lock
        self.v, self.w, self.both, self.rand = v, w, both, rand
        self.mbits = np.array([marker >> i & 1 for i in range(M)], dtype=np.uint8)

    @property
    def payload_bytes(self):
        assert (self.F - self.M) % 8 == 0
        return (self.F - self.M) // 8


def ccsds(depth, **kw):
    return Cfg(CCSDS_MARKER, 32, 32 + 8 * depth * 255, rand=CCSDS_RAND, **kw)


# ---- the randomiser ---------------------------------------------------------------------------------------------------------------

def rand_bits(poly, seed, n):
    """n bits of the Fibonacci register: the bit is s & 1, then s = s >> 1 | parity(s & poly & 0xFF) << 7."""
    s, out = seed, []
    for _ in range(n):
        out.append(s & 1)
        s = s >> 1 | (bin(s & poly & 0xFF).count("1") & 1) << 7
    return out


def rand_bytes(rand, n):
    """The first n table bytes: the register's bits from the seed, packed most significant first."""
    if rand is None:
        return np.zeros(n, dtype=np.uint8)
    b = rand_bits(rand[0], rand[1], 8 * n)
    return np.array([int("".join(map(str, b[8 * j:8 * j + 8])), 2) for j in range(n)], dtype=np.uint8)


def rand_period(rand):
    """The period of the table in bytes: the smallest p with byte j + p = byte j."""
    t = rand_bytes(rand, 600).tolist()
    return next(p for p in range(1, 300) if t[p:p + 300] == t[:300])


# ---- attach and extract -----------------------------------------------------------------------------------------------------------

def attach(cfg, payload):
    """The bits (uint8 array) of the frames of whole payloads: marker, then the payload XOR the table, bytes least significant bit first."""
    pb = cfg.payload_bytes
    payload = np.asarray(payload, dtype=np.uint8).reshape(-1, pb)
    table = rand_bytes(cfg.rand, pb)
    out = [np.concatenate([cfg.mbits, np.unpackbits(fr ^ table, bitorder="little")]) for fr in payload]
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)


def extract(cfg, bits, pos, meta, first_bit=0):
    """The payload bytes of the records: cut out, complemented where the polarity bit is set, derandomised."""
    pb = cfg.payload_bytes
    table = rand_bytes(cfg.rand, pb)
    out = np.zeros((len(pos), pb), dtype=np.uint8)
    for i, (p, m) in enumerate(zip(pos, meta)):
        r = p - first_bit + cfg.M
        out[i] = np.packbits(bits[r:r + 8 * pb] ^ (m >> 8 & 1), bitorder="little") ^ table
    return out.reshape(-1)


# ---- the machine --------------------------------------------------------------------------------------------------------------------

def new_state(pos=0):
    s = dict(mode=SEARCH, pol=0, fresh=0, misses=0, overflow=0, error=0, last=0, pos=pos)
    s.update({k: 0 for k in COUNTERS})
    return s


def words(s):
    """The eight words of bbb.h."""
    w0 = s["mode"] | s["pol"] << 8 | s["fresh"] << 9 | s["misses"] << 16 | s["overflow"] << 24 | s["error"] << 25 | s["last"] << 32
    return [w0, s["pos"]] + [s[k] for k in COUNTERS]


def distances(cfg, bits):
    """dist(r, 0) for every r whose marker lies inside the bits."""
    n = len(bits) - cfg.M + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    d = np.zeros(n, dtype=np.int64)
    for i in range(cfg.M):
        d += bits[i:i + n] ^ cfg.mbits[i]
    return d


def run(cfg, bits, first_bit=0, final=True, state=None, max_frames=None):
    """One call over `bits` (uint8 array, bit 0 at position first_bit): (pos, meta, state); the state is changed in place."""
    s = new_state(first_bit) if state is None else state
    if s["pos"] < first_bit:
        s["error"] = 1
        return [], [], s
    M, F, n = cfg.M, cfg.F, len(bits)
    d0 = distances(cfg, bits)

    def dist(r, pol):                                 # relative position; beyond the data: M + 1
        if r + M > n:
            return M + 1
        return int(M - d0[r] if pol else d0[r])
    hit = d0 <= cfg.tol_search
    if cfg.both:
        hit = hit | (M - d0 <= cfg.tol_search)
    cand = np.flatnonzero(hit)
    pos, meta, emitted = [], [], 0
    r = s["pos"] - first_bit
    while True:
        if s["mode"] == SEARCH:
            stop = True
            for p in cand[np.searchsorted(cand, r):].tolist():
                pol = 0 if d0[p] <= cfg.tol_search else 1
                if not final and p + cfg.v * F + M > n:
                    r, stop = p, None
                    break
                if all(dist(p + j * F, pol) <= cfg.tol_lock for j in range(1, cfg.v + 1)):
                    r, stop = p, False
                    s.update(mode=LOCK, pol=pol, misses=0, fresh=1)
                    s["acquisitions"] += 1
                    break
                s["rejected"] += 1
            if stop:                                  # no candidate left: the first position whose marker is not inside
                r = max(r, n - M + 1)
            if stop is not False:
                break
        else:
            if r + F > n:
                break
            d = dist(r, s["pol"])
            fly = d > cfg.tol_lock
            if fly:
                s["misses"] += 1
                if s["misses"] > cfg.w:
                    s.update(mode=SEARCH, misses=0)
                    s["losses"] += 1
                    continue
                s["flywheeled"] += 1
            else:
                s["misses"] = 0
                s["marker_bit_errors"] += d
            if max_frames is None or emitted < max_frames:
                pos.append(first_bit + r)
                meta.append(d | s["pol"] << 8 | int(fly) << 9 | s["fresh"] << 10)
            else:
                s["overflow"] = 1
            s["fresh"] = 0
            emitted += 1
            s["frames"] += 1
            r += F
    s["pos"], s["last"] = first_bit + r, emitted
    return pos, meta, s


def brute(cfg, bits):
    """One final call from a zero state, transcribed literally from the two rules: one bit position at a time, every distance
    counted bit by bit.  (frames as (pos, dist, pol, flywheeled, first), the counters, (mode, pol, misses, pos))."""
    N, M, F = len(bits), cfg.M, cfg.F

    def dist(p, pol):
        if p + M > N:
            return M + 1
        return sum(1 for i in range(M) if bits[p + i] != (cfg.marker >> i & 1) ^ pol)
    mode, pol, misses, pos, first = SEARCH, 0, 0, 0, 0
    frames, c = [], dict.fromkeys(COUNTERS, 0)
    while True:
        if mode == SEARCH:
            if pos + M > N:
                break
            found = [q for q in ((0, 1) if cfg.both else (0,)) if dist(pos, q) <= cfg.tol_search]
            if not found:
                pos += 1
            elif all(dist(pos + j * F, found[0]) <= cfg.tol_lock for j in range(1, cfg.v + 1)):
                mode, pol, misses, first = LOCK, found[0], 0, 1
                c["acquisitions"] += 1
            else:
                c["rejected"] += 1
                pos += 1
        else:
            if pos + F > N:
                break
            d = dist(pos, pol)
            if d <= cfg.tol_lock:
                misses = 0
                frames.append((pos, d, pol, 0, first))
                c["marker_bit_errors"] += d
            else:
                misses += 1
                if misses > cfg.w:
                    mode, misses = SEARCH, 0
                    c["losses"] += 1
                    continue
                frames.append((pos, d, pol, 1, first))
                c["flywheeled"] += 1
            c["frames"] += 1
            first = 0
            pos += F
    return frames, c, (mode, pol, misses, pos)


def brute_all(cfg, B):
    """`brute` for every row of B (streams of one length) at once: the same two rules, every stream taking one transition a
    round -- one bit position in SEARCH, one frame in LOCK -- and every distance counted bit by bit.  (fpos, fmeta, nf, counters
    as a dict of arrays, mode, pol, misses, pos); fpos and fmeta hold nf records a row, meta as bbb.h packs it."""
    n, N = B.shape
    M, F = cfg.M, cfg.F
    maxf = N // F + 1
    mode, pol, misses, pos, first = (np.zeros(n, dtype=np.int64) for _ in range(5))
    done = np.zeros(n, dtype=bool)
    c = {k: np.zeros(n, dtype=np.int64) for k in COUNTERS}
    fpos, fmeta, nf = np.zeros((n, maxf), dtype=np.int64), np.zeros((n, maxf), dtype=np.int64), np.zeros(n, dtype=np.int64)

    def dist(rows, p, q):                             # rows: stream numbers; p, q: their positions and polarities
        inside = p + M <= N
        d = np.zeros(len(rows), dtype=np.int64)
        for i in range(M):
            d += B[rows, np.where(inside, p + i, 0)] != ((cfg.marker >> i & 1) ^ q)
        return np.where(inside, d, M + 1)
    while not done.all():
        s = np.flatnonzero(~done & (mode == SEARCH))
        k = np.flatnonzero(~done & (mode == LOCK))
        if len(s):
            end = pos[s] + M > N
            done[s[end]] = True
            s = s[~end]
            hit0 = dist(s, pos[s], 0) <= cfg.tol_search
            hit1 = ~hit0 & (dist(s, pos[s], 1) <= cfg.tol_search) if cfg.both else np.zeros(len(s), dtype=bool)
            pos[s[~hit0 & ~hit1]] += 1
            s, q = s[hit0 | hit1], hit1[hit0 | hit1].astype(np.int64)
            ok = np.ones(len(s), dtype=bool)
            for j in range(1, cfg.v + 1):
                ok &= dist(s, pos[s] + j * F, q) <= cfg.tol_lock
            c["rejected"][s[~ok]] += 1
            pos[s[~ok]] += 1
            a = s[ok]
            mode[a], pol[a], misses[a], first[a] = LOCK, q[ok], 0, 1
            c["acquisitions"][a] += 1
        if len(k):
            end = pos[k] + F > N
            done[k[end]] = True
            k = k[~end]
            d = dist(k, pos[k], pol[k])
            miss = d > cfg.tol_lock
            misses[k[~miss]] = 0
            c["marker_bit_errors"][k[~miss]] += d[~miss]
            misses[k[miss]] += 1
            lost = miss & (misses[k] > cfg.w)
            mode[k[lost]], misses[k[lost]] = SEARCH, 0
            c["losses"][k[lost]] += 1
            c["flywheeled"][k[miss & ~lost]] += 1
            e, de, fl = k[~lost], d[~lost], miss[~lost].astype(np.int64)
            fpos[e, nf[e]], fmeta[e, nf[e]] = pos[e], de | pol[e] << 8 | fl << 9 | first[e] << 10
            nf[e] += 1
            c["frames"][e] += 1
            first[e] = 0
            pos[e] += F
    return fpos, fmeta, nf, c, mode, pol, misses, pos


def pack(bits):
    """uint8 bits to uint64 words, bit j at bit j % 64 of word j / 64 (zero padded)."""
    b = np.zeros((len(bits) + 63) // 64 * 64, dtype=np.uint8)
    b[:len(bits)] = bits
    return np.packbits(b, bitorder="little").view(np.uint64)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

def _marker(rng, M):
    """A marker with low self-correlation is not needed: any fixed pattern will do, the model says what comes out."""
    return int(rng.integers(0, 1 << 62)) & ((1 << M) - 1) | 1


def _frames(cfg, rng, n, pol=0):
    """n frames as bits: marker and random payload, complemented for pol = 1."""
    out = []
    for _ in range(n):
        out.append(np.concatenate([cfg.mbits, rng.integers(0, 2, cfg.F - cfg.M).astype(np.uint8)]) ^ pol)
    return out


def _flip(fr, rng, M, k):
    """k wrong bits in the marker of a frame."""
    fr = fr.copy()
    fr[rng.choice(M, k, replace=False)] ^= 1
    return fr


def stream_kinds():
    return ("clean", "junk", "slip1", "slipF-1", "tol search", "tol search+1", "tol lock", "tol lock+1", "w bad", "w+1 bad", "false candidate",
            "inverted", "inverted middle", "ends in marker", "ends in frame", "ends at frame end", "lose and regain")


def make_stream(cfg, rng, kind, nframes=8):
    """The bits of one stream of a kind (see the issue's list); what the machine makes of it is the model's business."""
    M, F = cfg.M, cfg.F
    fr = _frames(cfg, rng, nframes)
    junk = rng.integers(0, 2, int(rng.integers(1, 2 * F))).astype(np.uint8)
    tail = []
    if kind == "junk":
        fr = [junk] + fr
    elif kind == "slip1":
        fr.insert(nframes // 2, rng.integers(0, 2, 1).astype(np.uint8))
    elif kind == "slipF-1":
        fr.insert(nframes // 2, rng.integers(0, 2, F - 1).astype(np.uint8))
    elif kind in ("tol search", "tol search+1"):
        fr[0] = _flip(fr[0], rng, M, cfg.tol_search + (kind[-1] == "1"))
        fr = [junk] + fr
    elif kind in ("tol lock", "tol lock+1"):
        fr[nframes // 2] = _flip(fr[nframes // 2], rng, M, cfg.tol_lock + (kind[-1] == "1"))
    elif kind in ("w bad", "w+1 bad"):
        for j in range(cfg.w + (kind[0:3] == "w+1")):
            fr[1 + j] = _flip(fr[1 + j], rng, M, cfg.tol_lock + 1)
    elif kind == "false candidate":
        # a marker whose chain holds up to its last confirmation but one, a few bits ahead of the true chain
        gap = int(rng.integers(1, F))
        fake = [np.concatenate([cfg.mbits, rng.integers(0, 2, F - M).astype(np.uint8)]) for _ in range(max(cfg.v, 1))]
        fr = fake + [rng.integers(0, 2, gap).astype(np.uint8)] + fr
    elif kind == "inverted":
        fr = [junk] + [f ^ 1 for f in fr]
    elif kind == "inverted middle":
        fr = fr[:nframes // 2] + [f ^ 1 for f in fr[nframes // 2:]]
    elif kind == "ends in marker":
        tail = [cfg.mbits[:M // 2]]
    elif kind == "ends in frame":
        tail = [np.concatenate([cfg.mbits, rng.integers(0, 2, (F - M) // 2).astype(np.uint8)])]
    elif kind == "lose and regain":
        fr = _frames(cfg, rng, 4 * nframes)
        for j in range(3, len(fr), 5):
            for i in range(cfg.w + 1):
                if j + i < len(fr):
                    fr[j + i] = _flip(fr[j + i], rng, M, cfg.tol_lock + 1)
    return np.concatenate(fr + tail)


_grid = None


def grid_cases():
    """dicts of cfg, bits, and what `run` makes of them in one final call from a zero state (pos, meta, words), computed once:
    M in {8, 13, 32, 64}, F in {M + 8, 72, 200, 8192 + 32}, v in {0, 1, 3}, w in {0, 2}, both tolerance extremes, every kind of
    stream; with randomiser or without where the payload is whole bytes."""
    global _grid
    if _grid is not None:
        return _grid
    rng = np.random.default_rng(271)
    out, i = [], 0
    kinds = stream_kinds()
    for M in (8, 13, 32, 64):
        for F in (M + 8, 72, 200, 8192 + 32):
            if F < M + 8:
                continue
            for v in (0, 1, 3):
                for w in (0, 2):
                    for tol in ((0, 0), (M // 4, M // 4), (0, M // 4)):
                        i += 1
                        # every setting sees three kinds, so that the grid as a whole sees every kind under every v and w
                        for kind in (kinds[i % len(kinds)], kinds[(5 * i + 1) % len(kinds)], kinds[(7 * i + 3) % len(kinds)]):
                            cfg = Cfg(_marker(rng, M), M, F, tol[0], tol[1], v, w, both=True,
                                      rand=CCSDS_RAND if (F - M) % 8 == 0 and i % 2 else None)
                            bits = make_stream(cfg, rng, kind, nframes=5 if F > 8000 else 8)
                            out.append(dict(cfg=cfg, bits=bits, kind=kind))
    # both_polarities off on an inverted stream; every position a candidate; a full max_frames
    c = Cfg(0x1ACFFC1D, 32, 200, 1, 3, 1, 2, both=False)
    out.append(dict(cfg=c, bits=make_stream(c, rng, "inverted"), kind="inverted, one polarity"))
    for v in (0, 1, 3):
        c = Cfg(0, 16, 40, 0, 2, v, 1)
        out.append(dict(cfg=c, bits=np.zeros(1000, dtype=np.uint8), kind="all candidates"))
        c = Cfg(0, 16, 40, 0, 0, v, 1)
        z = np.zeros(1500, dtype=np.uint8)
        z[36::37] = 1                                  # every position whose window is clear is a candidate; many chains break
        out.append(dict(cfg=c, bits=z, kind="all candidates, rejected"))
    # LOCK over more frames than one round of the chain pass takes (1024, 256 lanes of four, waves of 64): runs of bad markers
    # that straddle a wave's, a lane round's and a whole round's boundary, ridden over (w) and lost (w + 1)
    for w, bad in ((2, (63, 64, 255, 256, 1023, 1024)), (2, (1022, 1023, 1024)), (1, (1023, 1024, 2047)), (0, (1024,)), (2, (1021, 1022, 1023))):
        c = Cfg(0x2D4B, 16, 32, 0, 1, 1, w)
        fr = _frames(c, rng, 2600)
        for j in bad:
            fr[j] = _flip(fr[j], rng, 16, 2)
        out.append(dict(cfg=c, bits=np.concatenate(fr), kind="long lock"))
    for case in out:
        pos, meta, st = run(case["cfg"], case["bits"])
        case.update(pos=pos, meta=meta, words=words(st))
    _grid = out
    return out


# ---- the closed loop (tests/test_framesync_host.py asserts it on the CPU models, tests/test_gpu_framesync.py holds the GPU to it) ----

# 16 CCSDS frames at depth 4 (rs_model.LOOP's data and code), a CCSDS marker attached to each and the payload randomised, 1237
# junk bits (default_rng(seed) integers) in front of the framed bits at the Viterbi decoder's output, that is in front of them
# at the convolutional encoder's input; (0171, 0133) at rate 1/2; the WHOLE channel inverted: transmitted bit c is sent as
# -(2c - 1) * 64 plus rint of default_rng(seed) normal noise of sigma 42 (drawn after the junk); hard decisions value >= 0.
# Both generators have odd weight, so the Viterbi decoder returns the complement of the framed bits.  tol_search 2, tol_lock 6,
# verify 1, flywheel 2.
SYNC_LOOP = dict(junk=1237, seed=43, tol_search=2, tol_lock=6, verify=1, flywheel=2)
SYNC_LOOP_COUNTS = dict(viterbi=1299, inverted=1, frames=16, flywheeled=0, acquisitions=1, losses=0, rejected=0, marker_bit_errors=6, failed=0,
                        symbols=417, data_bits=0, blind_failed=64, blind_codewords=64)

_sync_loop = {}


def sync_loop_record(seed=None):
    """(data bytes, transmitted bits, received int16 values, Viterbi output bits) of the loop, computed once a seed."""
    import conv_model
    import rs_model
    seed = SYNC_LOOP["seed"] if seed is None else seed
    if seed not in _sync_loop:
        code, data, coded, _, _ = rs_model.loop_record(4)
        fs = ccsds(4, tol_search=SYNC_LOOP["tol_search"], tol_lock=SYNC_LOOP["tol_lock"], v=SYNC_LOOP["verify"], w=SYNC_LOOP["flywheel"])
        rng = np.random.default_rng(seed)
        junk = rng.integers(0, 2, SYNC_LOOP["junk"]).astype(np.uint8)
        framed = np.concatenate([junk, attach(fs, coded)])
        inner = conv_model.Code(7, (0o171, 0o133))
        tx, _ = conv_model.encode(inner, framed)
        rx = -(2 * tx.astype(np.int64) - 1) * 64 + np.rint(rng.normal(0, rs_model.LOOP["sigma"], len(tx))).astype(np.int64)
        rx = np.clip(rx, -32768, 32767).astype(np.int16)
        vit, _ = conv_model.run(inner, (rx >= 0).astype(np.int64), hard=True)
        _sync_loop[seed] = (fs, data, framed, tx, rx, vit.astype(np.uint8))
    return _sync_loop[seed]


def sync_loop_counts(seed=None):
    import rs_model
    fs, data, framed, tx, rx, vit = sync_loop_record(seed)
    code = rs_model.ccsds(4)
    pos, meta, st = run(fs, vit)
    frames = extract(fs, vit, pos, meta)
    out, nerr, stats = rs_model.decode(code, frames)
    blind, nerr0, stats0 = rs_model.decode(code, np.packbits(vit, bitorder="little")[:len(vit) // 8 // code.frame_bytes * code.frame_bytes])
    return dict(viterbi=int((vit != framed[:len(vit)] ^ 1).sum()), inverted=int(all(m >> 8 & 1 for m in meta)), pos=pos,
                frames=st["frames"], flywheeled=st["flywheeled"], acquisitions=st["acquisitions"], losses=st["losses"], rejected=st["rejected"],
                marker_bit_errors=st["marker_bit_errors"], failed=int(stats[2]), symbols=int(stats[3]),
                data_bits=int(np.unpackbits(out[:len(data)] ^ data[:len(out)]).sum()) + 8 * abs(len(out) - len(data)),
                blind_failed=int(stats0[2]), blind_codewords=int(stats0[0]))
