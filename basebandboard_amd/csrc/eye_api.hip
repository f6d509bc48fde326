// eye_api.hip -- the extern "C" entry points of the eye diagram and bathtub (include/bbb.h).  Host logic only: argument
// checks and, on the transmitter side, what a chunk of tx_chunks.hpp's loop does and its scratch.
#include "capture.hpp"
#include "tx_chunks.hpp"

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
    bbb_eye_cfg eye{};
    int blocks = 0;
    DevBuf<uint32_t> scratch;        // per-block partial histograms
    DevBuf<uint64_t> bits;           // the chunk's data bits
    DevBuf<int16_t> buf;             // the chunk's waveform
    TxChunks tx;
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
    CallScratch<uint32_t> scratch;
    if ((rc = scratch.alloc(eye_scratch_words(blocks, eye->ncols), st))) return rc;
    EyeLaunch a = launch_of(*eye);
    a.want_hist = 1;
    return eye_accumulate_launch(a, samples_dev, nsamples, first_sample, scratch, blocks, hist_dev, nullptr, st);
}

int bbb_tx_eye_open(bbb_lutopt *h, const bbb_tx_cfg *cfg, const bbb_eye_cfg *eye, uint64_t chunk_samples, bbb_tx_eye **out) {
    auto e = std::make_unique<bbb_tx_eye>();
    int rc = tx_chunks_open(&e->tx, h, out, cfg, chunk_samples, kEyeChunkDefault, kEyeChunkMax, [&] {
        const int bad = tx_cfg_check(cfg);
        return bad ? bad : eye_cfg_check(eye);
    });
    if (rc) return rc;
    e->eye = *eye;
    e->blocks = eye_grid_blocks(e->tx.chunk);
    if (e->blocks < 0) return e->blocks;
    if ((rc = e->buf.grow((e->tx.chunk + 7) & ~7ull)) || (rc = e->bits.grow(eye_bits_words(e->tx.chunk))) ||
        (rc = e->scratch.grow(eye_scratch_words(e->blocks, eye->ncols))))
        return rc;
    *out = e.release();
    return BBB_OK;
}

int bbb_tx_eye_run(bbb_tx_eye *e, uint64_t first_sample, uint64_t nsamples, uint64_t *hist_dev, uint64_t *bathtub_dev) {
    if (!hist_dev && !bathtub_dev) return fail(BBB_EINVAL, "hist_dev and bathtub_dev are both NULL");
    if (!e) return fail(BBB_EINVAL, "null eye object");
    if (((uintptr_t)hist_dev & 7) || ((uintptr_t)bathtub_dev & 7)) return fail(BBB_EINVAL, "misaligned device pointer");
    if (const int rc = tx_range_check(first_sample, nsamples)) return rc;
    EyeLaunch a = launch_of(e->eye);
    a.want_hist = hist_dev != nullptr;
    a.want_tub = bathtub_dev != nullptr;
    a.pulser = e->tx.cfg.source == 1;
    return tx_chunks_walk(e->tx, e->buf.p, first_sample, nsamples, tx_same_range, [&](uint64_t s, uint64_t n, hipStream_t st) {
        if (a.want_tub && !a.pulser) {             // (the Pulser's bits are computed where they are needed)
            a.bits = reinterpret_cast<const unsigned long long *>(e->bits.p);
            TxBits b;
            if (const int rc = tx_chunk_bits(e->tx, eye_bit_range(s, n), e->bits, e->bits.cap, st, &b)) return rc;
            a.bit0 = b.lo;
            a.nbits = b.n;
        }
        return eye_accumulate_launch(a, e->buf, n, s, e->scratch, e->blocks, hist_dev, bathtub_dev, st);
    });
}

int bbb_tx_eye_close(bbb_tx_eye *e) {
    if (!e) return fail(BBB_EINVAL, "null eye object");
    delete e;
    return BBB_OK;
}

}  // extern "C"
