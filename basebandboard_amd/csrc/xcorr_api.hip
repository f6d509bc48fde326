// xcorr_api.hip -- the extern "C" entry points of the data-to-waveform correlation (include/bbb.h).  Host logic only:
// argument checks, the transmitter side's chunk loop and its scratch.  Like acf_api.hip, it uses a handle only through
// public calls (bbb_tx_fill_i16, bbb_awgn_prefetch, bbb_prbs_fill) and the accessors of bbb_common.hpp, so bbb_api.hip's
// scheduler model is unchanged.
#include "bbb_common.hpp"

#include <algorithm>
#include <memory>
#include <string>

using namespace bbb;

namespace {

constexpr uint64_t kXcorrChunkDefault = 1ull << 26;     // 128 MiB of int16: the correlator finds the chunk in the Infinity Cache
constexpr uint64_t kXcorrChunkMax = 1ull << 30;
constexpr uint64_t kXcorrLimit = 1ull << 62;
constexpr uint32_t kTxSpb = 8, kTxMaxLags = 512;

int64_t floor_div(int64_t v, int64_t d) { return v >= 0 ? v / d : -((-v + d - 1) / d); }

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

// the data bits samples [first, first + n) need, n > 0: [*lo, *hi], or none at all (*hi < *lo)
void needed_bits(uint64_t first, uint64_t n, const bbb_xcorr_cfg &c, int64_t *lo, int64_t *hi) {
    const int64_t f = (int64_t)first - (int64_t)c.origin;
    *hi = floor_div(f + (int64_t)n - 1, c.spb);
    *lo = std::max<int64_t>(0, floor_div(f - (int64_t)(c.nlags - 1), c.spb));
}

}  // namespace

struct bbb_tx_xcorr {
    bbb_lutopt *h = nullptr;
    bbb_tx_cfg cfg{};
    bbb_xcorr_cfg xc{};
    uint64_t chunk = 0;
    int device = 0;
    XcorrPlan plan{};
    int16_t *buf = nullptr;          // the chunk's waveform
    uint64_t *bits = nullptr;        // the chunk's data bits
    uint64_t *scratch = nullptr;     // per-workgroup partial counters
    uint64_t bits_words = 0;

    ~bbb_tx_xcorr() {
        if (device >= 0) (void)hipSetDevice(device);
        if (buf) (void)hipFree(buf);
        if (bits) (void)hipFree(bits);
        if (scratch) (void)hipFree(scratch);
    }
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
    int64_t lo, hi;
    needed_bits(first_sample, nsamples, *cfg, &lo, &hi);
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
    uint64_t *scratch = nullptr;
    BBB_HIP(hipMallocAsync((void **)&scratch, p.scratch_words * sizeof(uint64_t), st));
    const XcorrLaunch l{samples_dev, nsamples, first_sample, bits_packed_dev, bit0, nbits, cfg->spb, cfg->nlags, cfg->origin};
    rc = xcorr_launch(p, l, scratch, xc_dev, st);
    (void)hipFreeAsync(scratch, st);
    return rc;
}

int bbb_tx_xcorr_open(bbb_lutopt *h, const bbb_tx_cfg *cfg, uint32_t nlags, uint64_t chunk_samples, bbb_tx_xcorr **out) {
    if (!h) return fail(BBB_EINVAL, "null handle");
    if (!out) return fail(BBB_EINVAL, "null out");
    int rc = tx_cfg_check(cfg);
    if (rc) return rc;
    if (nlags == 0 || nlags > kTxMaxLags)
        return fail(BBB_EINVAL, "nlags must be 1.." + std::to_string(kTxMaxLags) + " (got " + std::to_string(nlags) + ")");
    if (chunk_samples > kXcorrChunkMax) return fail(BBB_EINVAL, "chunk_samples must be <= 2^30");
    const int device = lutopt_device(h);
    if (device < 0) return fail(BBB_ENODEV, "host-only handle (device -1) cannot generate samples");
    if ((rc = use_device(device))) return rc;
    auto x = std::make_unique<bbb_tx_xcorr>();
    x->h = h;
    x->cfg = *cfg;
    x->xc = bbb_xcorr_cfg{kTxSpb, nlags, BBB_TX_BIT_ORIGIN};
    x->device = device;
    x->chunk = chunk_samples ? chunk_samples : kXcorrChunkDefault;
    x->plan = xcorr_plan(kTxSpb, nlags, x->chunk);
    if (x->plan.gx < 0) return fail(BBB_EHIP, "could not size the correlator's grid");
    // the data bits of a chunk: at most (chunk + nlags - 1) / 8 + 2 of them
    x->bits_words = ((x->chunk + nlags) / kTxSpb + 2) / 64 + 3;
    BBB_HIP(hipMalloc((void **)&x->buf, ((x->chunk + 7) & ~7ull) * sizeof(int16_t)));
    BBB_HIP(hipMalloc((void **)&x->bits, x->bits_words * sizeof(uint64_t)));
    BBB_HIP(hipMalloc((void **)&x->scratch, x->plan.scratch_words * sizeof(uint64_t)));
    *out = x.release();
    return BBB_OK;
}

int bbb_tx_xcorr_run(bbb_tx_xcorr *x, uint64_t first_sample, uint64_t nsamples, int64_t *xc_dev) {
    if (!x) return fail(BBB_EINVAL, "null xcorr object");
    if (!xc_dev) return fail(BBB_EINVAL, "null xc_dev: the counters are the only output");
    if ((uintptr_t)xc_dev & 7) return fail(BBB_EINVAL, "misaligned device pointer");
    int rc = tx_range_check(first_sample, nsamples);
    if (rc) return rc;
    if (nsamples == 0) return BBB_OK;
    BBB_HIP(hipSetDevice(x->device));
    for (uint64_t off = 0; off < nsamples;) {
        const uint64_t n = std::min(x->chunk, nsamples - off), s = first_sample + off;
        if ((rc = bbb_tx_fill_i16(x->h, &x->cfg, x->buf, n, s))) return rc;
        // announce the next chunk's fill, as bbb_tx_eye_run does: its noise start states are derived beside this chunk
        if (x->cfg.noise_en && off + n < nsamples &&
            (rc = bbb_awgn_prefetch(x->h, std::min(x->chunk, nsamples - off - n), x->cfg.warmup + s + n)))
            return rc;
        hipStream_t st = lutopt_stream(x->h);     // the handle's stream, read per chunk like the fill itself does
        BBB_HIP(hipSetDevice(x->device));
        int64_t lo, hi;
        needed_bits(s, n, x->xc, &lo, &hi);
        if (hi >= lo) {
            const uint64_t nbits = (uint64_t)(hi - lo + 1);
            if ((nbits + 63) / 64 > x->bits_words) return fail(BBB_EHIP, "the chunk's data bits do not fit their buffer");
            if (x->cfg.source == 1)
                rc = xcorr_pulser_bits_launch(x->bits, (uint64_t)lo, (nbits + 63) / 64, st);
            else
                rc = bbb_prbs_fill(x->cfg.prbs_k, x->cfg.prbs_state, (uint64_t)lo, nbits, x->bits, x->device, st);
            if (rc) return rc;
            const XcorrLaunch l{x->buf, n, s, x->bits, (uint64_t)lo, nbits, x->xc.spb, x->xc.nlags, x->xc.origin};
            if ((rc = xcorr_launch(x->plan, l, x->scratch, xc_dev, st))) return rc;
        }
        off += n;
    }
    return BBB_OK;
}

int bbb_tx_xcorr_close(bbb_tx_xcorr *x) {
    if (!x) return fail(BBB_EINVAL, "null xcorr object");
    delete x;
    return BBB_OK;
}

}  // extern "C"
