// eye_api.hip -- the extern "C" entry points of the eye diagram and bathtub (include/bbb.h).  Host logic only: argument
// checks, the transmitter side's chunk loop and its scratch.  Kept out of bbb_api.hip, whose scheduler is compiled unchanged
// against a model of HIP (tests/sched_model/): the eye object uses the handle only through public calls (bbb_tx_fill_i16,
// bbb_awgn_prefetch) and two accessors that read its device and stream.
#include "bbb_common.hpp"

#include <algorithm>
#include <memory>
#include <string>

using namespace bbb;

namespace {

constexpr uint64_t kEyeChunkDefault = 1ull << 26;     // 128 MiB of int16: the reader finds the chunk in the Infinity Cache
constexpr uint64_t kEyeChunkMax = 1ull << 30;

EyeLaunch launch_of(const bbb_eye_cfg &e) {
    EyeLaunch a{};
    a.ncols = e.ncols;
    a.shift = e.shift;
    a.col_origin = e.col_origin;
    a.threshold = e.threshold;
    a.strict = e.strict != 0;
    return a;
}

}  // namespace

int bbb::eye_cfg_check(const bbb_eye_cfg *eye) {
    if (!eye) return fail(BBB_EINVAL, "null eye cfg");
    if (eye->ncols != 8 && eye->ncols != 16 && eye->ncols != 32 && eye->ncols != 64)
        return fail(BBB_EINVAL, "eye ncols must be 8, 16, 32 or 64 (got " + std::to_string(eye->ncols) + ")");
    if (eye->shift > 15) return fail(BBB_EINVAL, "eye shift must be 0..15 (got " + std::to_string(eye->shift) + ")");
    return BBB_OK;
}

struct bbb_tx_eye {
    bbb_lutopt *h = nullptr;
    bbb_tx_cfg cfg{};
    bbb_eye_cfg eye{};
    uint64_t chunk = 0;
    int device = 0, blocks = 0;
    int16_t *buf = nullptr;          // the chunk's waveform
    uint64_t *bits = nullptr;        // the chunk's data bits
    uint32_t *scratch = nullptr;     // per-block partial histograms
    uint64_t bits_words = 0;

    ~bbb_tx_eye() {
        if (device >= 0) (void)hipSetDevice(device);
        if (buf) (void)hipFree(buf);
        if (bits) (void)hipFree(bits);
        if (scratch) (void)hipFree(scratch);
    }
};

extern "C" {

int bbb_eye_accumulate_i16(const int16_t *samples_dev, uint64_t nsamples, uint64_t first_sample, const bbb_eye_cfg *eye,
                           uint64_t *hist_dev, int device, void *hip_stream) {
    int rc = eye_cfg_check(eye);
    if (rc) return rc;
    if (!hist_dev) return fail(BBB_EINVAL, "null hist_dev: the histogram is the only output of the capture side");
    if (nsamples && !samples_dev) return fail(BBB_EINVAL, "null samples_dev");
    if (((uintptr_t)samples_dev & 1) || ((uintptr_t)hist_dev & 7)) return fail(BBB_EINVAL, "misaligned device pointer");
    if ((rc = tx_range_check(first_sample, nsamples))) return rc;
    if (nsamples == 0) return BBB_OK;
    if ((rc = use_device(device))) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const int blocks = eye_grid_blocks(nsamples);
    if (blocks < 0) return blocks;
    // the slab belongs to this call (stream-ordered allocation from the device's pool, as bbb_prbs_check's counter)
    uint32_t *scratch = nullptr;
    BBB_HIP(hipMallocAsync((void **)&scratch, eye_scratch_words(blocks, eye->ncols) * sizeof(uint32_t), st));
    EyeLaunch a = launch_of(*eye);
    a.want_hist = 1;
    rc = eye_accumulate_launch(a, samples_dev, nsamples, first_sample, scratch, blocks, hist_dev, nullptr, st);
    (void)hipFreeAsync(scratch, st);
    return rc;
}

int bbb_tx_eye_open(bbb_lutopt *h, const bbb_tx_cfg *cfg, const bbb_eye_cfg *eye, uint64_t chunk_samples, bbb_tx_eye **out) {
    if (!h) return fail(BBB_EINVAL, "null handle");
    if (!out) return fail(BBB_EINVAL, "null out");
    int rc = tx_cfg_check(cfg);
    if (rc) return rc;
    if ((rc = eye_cfg_check(eye))) return rc;
    if (chunk_samples > kEyeChunkMax) return fail(BBB_EINVAL, "chunk_samples must be <= 2^30");
    const int device = lutopt_device(h);
    if (device < 0) return fail(BBB_ENODEV, "host-only handle (device -1) cannot generate samples");
    if ((rc = use_device(device))) return rc;
    auto e = std::make_unique<bbb_tx_eye>();
    e->h = h;
    e->cfg = *cfg;
    e->eye = *eye;
    e->device = device;
    e->chunk = chunk_samples ? chunk_samples : kEyeChunkDefault;
    e->blocks = eye_grid_blocks(e->chunk);
    if (e->blocks < 0) return e->blocks;
    // the data bits of a chunk: bits floor((s - 45) / 8) .. floor((s + chunk - 46) / 8), at most chunk / 8 + 1 of them
    e->bits_words = (e->chunk / 8 + 2) / 64 + 3;
    BBB_HIP(hipMalloc((void **)&e->buf, ((e->chunk + 7) & ~7ull) * sizeof(int16_t)));
    BBB_HIP(hipMalloc((void **)&e->bits, e->bits_words * sizeof(uint64_t)));
    BBB_HIP(hipMalloc((void **)&e->scratch, eye_scratch_words(e->blocks, eye->ncols) * sizeof(uint32_t)));
    *out = e.release();
    return BBB_OK;
}

int bbb_tx_eye_run(bbb_tx_eye *e, uint64_t first_sample, uint64_t nsamples, uint64_t *hist_dev, uint64_t *bathtub_dev) {
    if (!hist_dev && !bathtub_dev) return fail(BBB_EINVAL, "hist_dev and bathtub_dev are both NULL");
    if (!e) return fail(BBB_EINVAL, "null eye object");
    if (((uintptr_t)hist_dev & 7) || ((uintptr_t)bathtub_dev & 7)) return fail(BBB_EINVAL, "misaligned device pointer");
    int rc = tx_range_check(first_sample, nsamples);
    if (rc) return rc;
    if (nsamples == 0) return BBB_OK;
    BBB_HIP(hipSetDevice(e->device));
    EyeLaunch a = launch_of(e->eye);
    a.want_hist = hist_dev != nullptr;
    a.want_tub = bathtub_dev != nullptr;
    a.pulser = e->cfg.source == 1;
    for (uint64_t off = 0; off < nsamples;) {
        const uint64_t n = std::min(e->chunk, nsamples - off), s = first_sample + off;
        if ((rc = bbb_tx_fill_i16(e->h, &e->cfg, e->buf, n, s))) return rc;
        // announce the next chunk, as TX.generate does: its noise start states are derived beside this chunk's kernels
        if (e->cfg.noise_en && off + n < nsamples &&
            (rc = bbb_awgn_prefetch(e->h, std::min(e->chunk, nsamples - off - n), e->cfg.warmup + s + n)))
            return rc;
        hipStream_t st = lutopt_stream(e->h);     // the handle's stream, read per chunk like the fill itself does
        BBB_HIP(hipSetDevice(e->device));
        if (a.want_tub && !a.pulser) {
            const int64_t lo = std::max<int64_t>(0, floor8((int64_t)s - BBB_TX_BIT_SAMPLE0));
            const int64_t hi = floor8((int64_t)(s + n - 1) - BBB_TX_BIT_SAMPLE0);
            a.bits = reinterpret_cast<const unsigned long long *>(e->bits);
            a.bit0 = lo;
            a.nbits = hi >= lo ? (uint64_t)(hi - lo + 1) : 0;
            if (a.nbits && (rc = bbb_prbs_fill(e->cfg.prbs_k, e->cfg.prbs_state, (uint64_t)lo, a.nbits, e->bits, e->device, st)))
                return rc;
        }
        if ((rc = eye_accumulate_launch(a, e->buf, n, s, e->scratch, e->blocks, hist_dev, bathtub_dev, st))) return rc;
        off += n;
    }
    return BBB_OK;
}

int bbb_tx_eye_close(bbb_tx_eye *e) {
    if (!e) return fail(BBB_EINVAL, "null eye object");
    delete e;
    return BBB_OK;
}

}  // extern "C"
