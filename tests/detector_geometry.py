"""What bbb_prbs_detector_stream does with a call's geometry, restated from detector_api.hip (det_plan) and detector_kernels.hip
for the tests (test_detector_geometry_host.py holds this restatement to the text of those files, test_sched_model_detector.py to
what det_plan returns; test_gpu_detector_forms.py uses it to name the form each of its cells is meant to take).  Nothing here
is read by the product."""

KS = (7, 9, 11, 15, 20, 23, 31)
TAPS = {7: 6, 9: 5, 11: 9, 15: 14, 20: 3, 23: 18, 31: 28}            # det_tap_of (prbs.py:14)
FUSED_MAX_CHUNK_WORDS = 1024                                          # kDetFusedMaxChunkWords
MASK64 = (1 << 64) - 1


def det_lag(k):
    """DetLag<K>: dict(M, LAGK, LAGT, NH, OK) -- the trinomial squared M times until the tap's lag is a whole word."""
    tap = TAPS[k]
    m = next((i for i in range(5) if (tap << i) >= 64), 5)
    lagk, lagt = k << m, tap << m
    nh = (lagk + 63) // 64
    return dict(M=m, LAGK=lagk, LAGT=lagt, NH=nh, OK=nh <= 3)


def default_chunk_words(nbits, ncu=256):
    """det_plan (detector_api.hip) with chunk_bits == 0."""
    want = (nbits // 262144 + 127) // 128 * 128
    chunk_bits = 4096 if want < 4096 else (32768 if want > 32768 else want)
    if want > 32768:
        nwords = (nbits + 63) // 64
        best_cost, best_cw = None, 512
        for cw in range(512, FUSED_MAX_CHUNK_WORDS + 1, 128):
            nblocks = ((nwords + cw - 1) // cw + 255) // 256
            cost = (nblocks + ncu - 1) // ncu * cw
            if best_cost is None or cost <= best_cost:
                best_cost, best_cw = cost, cw
        chunk_bits = best_cw * 64
    return chunk_bits // 64


def form_of(k, chunk_words, warm_bits, aligned16=True):
    """The execution form det_plan (detector_api.hip) chooses: 'fused', 'two-kernel', 'dense-tiled' (tiles offered: a wave with 64
    full chunks behind a full warm-up takes them) or 'dense-lane'."""
    warm_words = (warm_bits + 63) // 64
    if det_lag(k)["OK"] and aligned16:
        if chunk_words % 128 == 0 and chunk_words <= FUSED_MAX_CHUNK_WORDS and warm_words <= 128:
            return "fused"
        return "two-kernel"
    if chunk_words % 16 == 0 and warm_words % 16 == 0 and warm_words > 0 and aligned16:
        return "dense-tiled"
    return "dense-lane"


def delayed_words(w):
    """V[n] = (w[n] << 1) | (w[n-1] >> 63): the input as the detector's bit_in register delays it (V[0] takes a 0)."""
    return [((int(w[n]) << 1) | (int(w[n - 1]) >> 63 if n else 0)) & MASK64 for n in range(len(w))]


def window(hist, off):
    """64 bits from bit `off` of the words `hist` laid end to end, bit 0 = the oldest bit of hist[0] (det_hist_window)."""
    big = 0
    for q, h in enumerate(hist):
        big |= int(h) << (64 * q)
    return (big >> off) & MASK64


def word_recurrence_holds(k, v, n):
    """V[n] == window(V[n-NH .. n-1], 64 NH - LAGK) ^ window(.., 64 NH - LAGT): the equality part of the clean predicate."""
    lg = det_lag(k)
    nh = lg["NH"]
    hist = v[n - nh: n]
    return v[n] == window(hist, 64 * nh - lg["LAGK"]) ^ window(hist, 64 * nh - lg["LAGT"])


def last_term_holds(k, v, w, n):
    """bit 63 of word n == V[n][64 - K] ^ V[n][64 - TAP]: the `last` term (err after the word's last clock)."""
    return (int(w[n]) >> 63) & 1 == ((v[n] >> (64 - k)) ^ (v[n] >> (64 - TAPS[k]))) & 1
