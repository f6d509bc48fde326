"""tests/detector_geometry.py restates constants and rules of the stream detector -- detector_kernels.hip (the kernels and their
launchers), detector_launch.hpp (what the kernel file exports) and detector_api.hip (the host scheduler and its det_plan) -- for
the GPU form matrix (test_gpu_detector_forms.py).  This file makes drift loud: it reads the three files as text and holds the
restatement to them, and it checks the word recurrence the sparse forms rest on against the oracle's PRBS, in plain integers.
It is also the one place that lists which template instantiations exist."""
import pathlib
import re

import pytest

from detector_geometry import (FUSED_MAX_CHUNK_WORDS, KS, TAPS, default_chunk_words, delayed_words, det_lag, form_of, last_term_holds,
                               word_recurrence_holds)

CSRC = pathlib.Path(__file__).resolve().parent.parent / "basebandboard_amd" / "csrc"
SRC = (CSRC / "detector_kernels.hip").read_text()          # the kernels, DetLag, det_tap_of, the launchers and their switch over k
HDR = (CSRC / "detector_launch.hpp").read_text()           # what the kernel file exports to the host file
API = (CSRC / "detector_api.hip").read_text()              # the scheduler: det_plan holds the geometry
SPARSE_KS = (7, 9, 11, 15, 23, 31)


def squeeze(s):
    return re.sub(r"\s+", " ", s)


def test_constants_of_the_kernel_file():
    assert f"constexpr int kDetFusedMaxChunkWords = {FUSED_MAX_CHUNK_WORDS};" in HDR and FUSED_MAX_CHUNK_WORDS == 1024
    taps = re.search(r"det_tap_of\(int k\) \{\s*return (.*?);", SRC).group(1)
    assert {int(a): int(b) for a, b in re.findall(r"k == (\d+) \? (\d+)", taps)} == TAPS
    # DetLag: M by the tap, the lags, the history length and the rule for OK
    assert "M = TAP >= 64 ? 0 : TAP * 2 >= 64 ? 1 : TAP * 4 >= 64 ? 2 : TAP * 8 >= 64 ? 3 : TAP * 16 >= 64 ? 4 : 5;" in SRC
    assert "LAGK = K << M, LAGT = TAP << M;" in SRC and "NH = (LAGK + 63) / 64;" in SRC and "OK = NH <= 3;" in SRC


def test_form_selection_of_the_kernel_file():
    """The conditions detector_geometry.form_of restates, as they stand in det_plan and, for the tiles, in det_chunk_kernel."""
    s = squeeze(API)
    assert "if (chunk_words % 128 == 0 && chunk_words <= (u64)kDetFusedMaxChunkWords && warm_words <= 128 && !two_kernels)" in s
    assert "const bool sparse = kSparse && !dense && ((uintptr_t)src & 15) == 0;" in s
    # (what exports DetLag<K>::OK to the host: the kernel file's det_sparse_ok, and det_plan's use of it)
    assert "const bool kSparse = det_sparse_ok(k);" in s
    assert "bool det_sparse_ok(int k) {" in SRC and "return (int)DetLag<decltype(kc)::value>::OK;" in squeeze(SRC)
    assert "const int tiles_ok = chunk_words % 16 == 0 && warm_words % 16 == 0 && warm_words > 0 && ((uintptr_t)src & 15) == 0;" in s
    assert "if (tiles_ok && c0 + 64 <= nchunks && c0 * chunk_words >= warm_words && (c0 + 64) * chunk_words * 64 <= nbits)" in squeeze(SRC)
    assert "const u64 chunk_words = chunk_bits / 64, warm_words = (warm_bits + 63) / 64;" in s
    # the knobs that could send a call another way exist in the experiments build only
    assert "BBB_EXPERIMENTS" in (pathlib.Path(__file__).resolve().parent.parent / "basebandboard_amd" / "csrc" / "bbb_common.hpp").read_text()


def test_default_chunk_rule_of_the_kernel_file():
    s = squeeze(API)
    assert "const uint64_t want = (nbits / 262144 + 127) / 128 * 128;" in s
    assert "chunk_bits = want < 4096 ? 4096 : (want > 32768 ? 32768 : want);" in s
    assert "for (uint64_t cw = 512; cw <= (uint64_t)kDetFusedMaxChunkWords; cw += 128) {" in s
    assert "const uint64_t nblocks = ((nwords + cw - 1) / cw + 255) / 256;" in s
    assert "const uint64_t cost = ((nblocks + (uint64_t)ncu - 1) / (uint64_t)ncu) * cw;" in s
    assert "if (cost <= best_cost) { best_cost = cost; best_cw = cw; }" in s
    assert "if (warm_bits == 0) warm_bits = 1024;" in s


@pytest.mark.parametrize("nbits,words,form", [(300_001, 64, "two-kernel"), (2_000_000, 64, "two-kernel"), (1_000_000_000, 64, "two-kernel"),
                                              (2_120_000_000, 128, "fused"), (2_147_000_000, 128, "fused"), (4_260_000_000, 254, "two-kernel"),
                                              (8_590_000_000, 512, "fused"), (10_000_000_000, 640, "fused")])
def test_default_geometry_at_the_lengths_in_use(nbits, words, form):
    """What a default call (chunk_bits = 0, warm_bits = 0) gets on 256 CUs: every default-geometry test below 2e9 bits
    is a two-kernel call, the benchmark's 1e10 bits a fused one."""
    assert default_chunk_words(nbits, 256) == words
    for k in SPARSE_KS:
        assert form_of(k, words, 1024) == form
    assert form_of(20, words, 1024) == ("dense-tiled" if words % 16 == 0 else "dense-lane")
    assert form_of(31, words, 1024, aligned16=False) == "dense-lane"


def test_lag_constants_and_instantiations():
    got = [(det_lag(k)["M"], det_lag(k)["NH"]) for k in KS]
    assert got == [(4, 2), (4, 3), (3, 2), (3, 2), (5, 10), (2, 2), (2, 2)]
    assert [(det_lag(k)["LAGK"], det_lag(k)["LAGT"]) for k in SPARSE_KS] == [(112, 96), (144, 80), (88, 72), (120, 112), (92, 72), (124, 112)]
    assert tuple(k for k in KS if det_lag(k)["OK"]) == SPARSE_KS
    for k in KS:
        lg = det_lag(k)
        assert lg["OK"] == (lg["NH"] <= 3) and lg["LAGT"] >= 64            # every bit of the next word depends on earlier words only
    # one case per k in the launchers' one switch, and with it det_chunk_kernel<K, true / false>, det_serial_kernel<K>, and for the
    # k with OK det_fused_kernel<K>, det_classify_kernel<K>, det_sparse_kernel<K>
    cases = re.findall(r"(?:case (\d+)|default): return f\(std::integral_constant<int, (\d+)>", SRC)
    assert sorted(int(b) for _, b in cases) == list(KS) and all(a in ("", b) for a, b in cases)
    assert "detector_stream_k" not in SRC + API and SRC.count("switch (k)") == 1      # the host scheduler is no template on K
    assert "static_assert(NH + 2 <= 5" in SRC                              # det_classify_256: the two lanes below hold the history


def failing_words(k, w, lo, hi):
    v = delayed_words(w)
    return [n for n in range(lo, hi) if not word_recurrence_holds(k, v, n)], [n for n in range(lo, hi) if not last_term_holds(k, v, w, n)]


# the words whose equality fails after ONE flipped bit in word 100 (the windows that reach it), and whose `last` term fails
PINNED_BIT20 = {7: [100, 101, 102], 9: [100, 101, 102], 11: [100, 101], 15: [100, 102], 23: [100, 101], 31: [100, 102]}
PINNED_BIT63 = {7: [101, 102], 9: [101, 102, 103], 11: [101, 102], 15: [101, 102], 23: [101, 102], 31: [101, 102]}


@pytest.mark.parametrize("k", SPARSE_KS)
def test_word_recurrence_on_the_oracle_stream(oracle, k):
    """With V[n] = (w[n] << 1) | (w[n-1] >> 63) a clean stream satisfies V[n] == window(V[n-NH .. n-1], 64 NH - K 2^M) ^
    window(.., 64 NH - TAP 2^M) for every n >= NH + 1, and the `last` term everywhere: what det_classify_256, det_half_flags,
    det_span_sparse and det_span_tiled all test.  One flipped bit fails the equality for the word that holds it and the
    following words whose windows reach it -- except bit 63, which is not in V[n]: there only the `last` term sees it."""
    nh = det_lag(k)["NH"]
    w = [int(x) for x in oracle.prbs_packed(k, 200 * 64)[0]]
    eq, last = failing_words(k, w, nh + 1, 200)
    assert eq == [] and last == []
    bad = list(w)
    bad[100] ^= 1 << 20
    eq, last = failing_words(k, bad, nh + 1, 200)
    assert eq == PINNED_BIT20[k] and last == []
    bad = list(w)
    bad[100] ^= 1 << 63
    eq, last = failing_words(k, bad, nh + 1, 200)
    assert eq == PINNED_BIT63[k] and last == [100]
