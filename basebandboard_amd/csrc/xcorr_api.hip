// xcorr_api.hip -- the extern "C" entry points of the data-to-waveform correlation (include/bbb.h).  Host logic only:
// argument checks and, on the transmitter side, what a chunk of tx_chunks.hpp's loop does and its scratch.
#include "capture.hpp"
#include "tx_chunks.hpp"

#include <memory>
#include <string>

using namespace bbb;

namespace {

constexpr uint64_t kXcorrChunkDefault = 1ull << 26;     // 128 MiB of int16: the correlator finds the chunk in the Infinity Cache
constexpr uint64_t kXcorrChunkMax = 1ull << 30;
constexpr uint64_t kXcorrLimit = 1ull << 62;
constexpr uint32_t kTxSpb = 8, kTxMaxLags = 512;

int xcorr_cfg_check(const bbb_xcorr_cfg *c) {
    if (!c) return fail(BBB_EINVAL, "null xcorr cfg");
    if (c->spb != 1 && c->spb != 2 && c->spb != 4 && c->spb != 8 && c->spb != 16 && c->spb != 32)
        return fail(BBB_EINVAL, "spb must be 1, 2, 4, 8, 16 or 32 (got " + std::to_string(c->spb) + ")");
    const uint32_t most = std::min<uint32_t>(64 * c->spb, BBB_XCORR_MAX_LAGS);
    if (c->nlags == 0 || c->nlags > most)
        return fail(BBB_EINVAL, "nlags must be 1.." + std::to_string(most) + " at spb " + std::to_string(c->spb) + " (got " +
                                    std::to_string(c->nlags) + ")");
    if (c->origin > kXcorrLimit) return fail(BBB_EINVAL, "origin must be <= 2^62");
    return BBB_OK;
}

}  // namespace

struct bbb_tx_xcorr {
    bbb_xcorr_cfg xc{};
    XcorrPlan plan{};
    DevBuf<uint64_t> scratch;        // per-workgroup partial counters
    DevBuf<uint64_t> bits;           // the chunk's data bits
    DevBuf<int16_t> buf;             // the chunk's waveform
    TxChunks tx;
};

extern "C" {

int bbb_xcorr_accumulate_i16(const int16_t *samples_dev, uint64_t nsamples, uint64_t first_sample,
                             const uint64_t *bits_packed_dev, uint64_t bit0, uint64_t nbits, const bbb_xcorr_cfg *cfg,
                             int64_t *xc_dev, int device, void *hip_stream) {
    int rc = xcorr_cfg_check(cfg);
    if (rc) return rc;
    if (!xc_dev) return fail(BBB_EINVAL, "null xc_dev: the counters are the only output");
    if (nsamples && !samples_dev) return fail(BBB_EINVAL, "null samples_dev");
    if (((uintptr_t)samples_dev & 1) || ((uintptr_t)xc_dev & 7) || ((uintptr_t)bits_packed_dev & 7))
        return fail(BBB_EINVAL, "misaligned device pointer");
    if ((rc = tx_range_check(first_sample, nsamples))) return rc;
    if (bit0 > kXcorrLimit || nbits > kXcorrLimit - bit0) return fail(BBB_EINVAL, "bit0 + nbits must be <= 2^62");
    if (nsamples == 0) return BBB_OK;
    const auto [lo, hi] = xcorr_bit_range(first_sample, nsamples, *cfg);
    if (hi < lo) return BBB_OK;                        // every sample lies below bit 0: no term counts
    if (!bits_packed_dev) return fail(BBB_EINVAL, "null bits_packed_dev");
    if ((int64_t)bit0 > lo || (int64_t)(bit0 + nbits) <= hi)
        return fail(BBB_EINVAL, "the call needs data bits " + std::to_string(lo) + " .. " + std::to_string(hi) + ", given are " +
                                    std::to_string(bit0) + " .. " + std::to_string(bit0 + nbits) + " (exclusive)");
    if ((rc = use_device(device))) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const XcorrPlan p = xcorr_plan(cfg->spb, cfg->nlags, nsamples);
    if (p.gx < 0) return fail(BBB_EHIP, "could not size the correlator's grid");
    // the slab belongs to this call (stream-ordered allocation, as bbb_eye_accumulate_i16's)
    CallScratch<uint64_t> scratch;
    if ((rc = scratch.alloc(p.scratch_words, st))) return rc;
    const XcorrLaunch l{samples_dev, nsamples, first_sample, bits_packed_dev, bit0, nbits, cfg->spb, cfg->nlags, cfg->origin};
    return xcorr_launch(p, l, scratch, xc_dev, st);
}

int bbb_tx_xcorr_open(bbb_lutopt *h, const bbb_tx_cfg *cfg, uint32_t nlags, uint64_t chunk_samples, bbb_tx_xcorr **out) {
    auto x = std::make_unique<bbb_tx_xcorr>();
    int rc = tx_chunks_open(&x->tx, h, out, cfg, chunk_samples, kXcorrChunkDefault, kXcorrChunkMax, [&] {
        if (const int bad = tx_cfg_check(cfg)) return bad;
        if (nlags == 0 || nlags > kTxMaxLags)
            return fail(BBB_EINVAL, "nlags must be 1.." + std::to_string(kTxMaxLags) + " (got " + std::to_string(nlags) + ")");
        return BBB_OK;
    });
    if (rc) return rc;
    x->xc = bbb_xcorr_cfg{kTxSpb, nlags, BBB_TX_BIT_ORIGIN};
    x->plan = xcorr_plan(kTxSpb, nlags, x->tx.chunk);
    if (x->plan.gx < 0) return fail(BBB_EHIP, "could not size the correlator's grid");
    if ((rc = x->buf.grow((x->tx.chunk + 7) & ~7ull)) || (rc = x->bits.grow(xcorr_bits_words(x->tx.chunk, nlags))) ||
        (rc = x->scratch.grow(x->plan.scratch_words)))
        return rc;
    *out = x.release();
    return BBB_OK;
}

int bbb_tx_xcorr_run(bbb_tx_xcorr *x, uint64_t first_sample, uint64_t nsamples, int64_t *xc_dev) {
    if (!x) return fail(BBB_EINVAL, "null xcorr object");
    if (!xc_dev) return fail(BBB_EINVAL, "null xc_dev: the counters are the only output");
    if ((uintptr_t)xc_dev & 7) return fail(BBB_EINVAL, "misaligned device pointer");
    if (const int rc = tx_range_check(first_sample, nsamples)) return rc;
    return tx_chunks_walk(x->tx, x->buf.p, first_sample, nsamples, tx_same_range, [&](uint64_t s, uint64_t n, hipStream_t st) {
        TxBits b;
        if (const int rc = tx_chunk_bits(x->tx, xcorr_bit_range(s, n, x->xc), x->bits, x->bits.cap, st, &b)) return rc;
        if (b.n == 0) return BBB_OK;              // every sample lies below bit 0: no term counts
        const XcorrLaunch l{x->buf, n, s, x->bits, (uint64_t)b.lo, b.n, x->xc.spb, x->xc.nlags, x->xc.origin};
        return xcorr_launch(x->plan, l, x->scratch, xc_dev, st);
    });
}

int bbb_tx_xcorr_close(bbb_tx_xcorr *x) {
    if (!x) return fail(BBB_EINVAL, "null xcorr object");
    delete x;
    return BBB_OK;
}

}  // extern "C"
