// hist_api.hip -- the extern "C" entry point of the sample histogram (include/bbb.h, bbb_awgn_hist).  Host logic only: argument
// checks and the chunk loop.  Kept out of bbb_api.hip, whose scheduler is compiled unchanged against a model of HIP
// (tests/sched_model/): this file uses the handle through public calls (bbb_awgn_fill_i8 / _i16, bbb_awgn_prefetch,
// bbb_lutopt_set_staged), through accessors that read its fields, and -- for the shipped n256 matrix -- through
// lutopt_stage_visit, which runs the staged sample kernel of a chunk and lets this file's kernel read the staging slot in the byte
// mover's place.
// What a call owns (its partial histograms, and the chunk buffer of the generators that have no planes form) is allocated
// stream-ordered from the device's pool on the handle's stream and released behind the last kernel, as bbb_eye_accumulate_i16's slab.
#include "capture.hpp"

#include <algorithm>
#include <string>

using namespace bbb;

namespace {

constexpr uint64_t kHistFusedMin = 1ull << 24;        // the staged form's own threshold (bbb_lutopt_set_staged)
constexpr uint64_t kHistFusedChunk = 1ull << 30;      // samples per staged sample kernel: 1 GiB of count planes per staging slot
constexpr uint64_t kHistBufChunk = 1ull << 26;        // samples per chunk that goes through memory

struct HistCall {
    uint32_t *scratch = nullptr;
    uint64_t *hist = nullptr;
    int blocks = 0;
};

// the reader of a staging slot: the histogram mover and the reduce behind it, on the mover's stream
int hist_visit(void *ctx, const void *stage, uint64_t nsamples, unsigned L, uint64_t, unsigned nlanes, hipStream_t st) {
    const HistCall *c = static_cast<const HistCall *>(ctx);
    unsigned used = 0;
    int rc = hist_planes_launch(stage, nsamples, L, nlanes, c->scratch, c->blocks, &used, st);
    if (rc) return rc;
    return hist_reduce_launch(c->scratch, used, 256, c->hist, st);
}

// the size of the chunk that starts with `left` samples to go
uint64_t chunk_of(bool fused_ok, uint64_t left) {
    if (fused_ok && left >= kHistFusedMin) return std::min(left, kHistFusedChunk);
    return std::min(left, kHistBufChunk);
}

int hist_chunks(bbb_lutopt *h, const HistCall &c, bool fused_ok, int k, void *buf, uint64_t nsamples, uint64_t first_step) {
    const int elem = k > 256 ? 2 : 1;
    int rc;
    for (uint64_t off = 0; off < nsamples;) {
        const uint64_t n = chunk_of(fused_ok, nsamples - off), s = first_step + off;
        const bool fused = fused_ok && n >= kHistFusedMin;
        if (fused) {
            if ((rc = lutopt_stage_visit(h, n, s, hist_visit, const_cast<HistCall *>(&c)))) return rc;
        } else {
            rc = elem == 1 ? bbb_awgn_fill_i8(h, (int8_t *)buf, n, s) : bbb_awgn_fill_i16(h, (int16_t *)buf, n, s);
            if (rc) return rc;
        }
        // announce the next chunk: its start states are derived beside this chunk's kernels
        if (off + n < nsamples && (rc = bbb_awgn_prefetch(h, chunk_of(fused_ok, nsamples - off - n), s + n))) return rc;
        if (!fused) {
            hipStream_t st = lutopt_stream(h);
            BBB_HIP(hipSetDevice(lutopt_device(h)));
            unsigned used = 0;
            if ((rc = hist_samples_launch(buf, elem, n, (unsigned)k, c.scratch, c.blocks, &used, st))) return rc;
            if ((rc = hist_reduce_launch(c.scratch, used, (unsigned)k, c.hist, st))) return rc;
        }
        off += n;
    }
    return BBB_OK;
}

}  // namespace

extern "C" {

int bbb_awgn_hist(bbb_lutopt *h, uint64_t *hist_dev, uint64_t nsamples, uint64_t first_step) {
    if (!h) return fail(BBB_EINVAL, "null handle");
    if (!hist_dev) return fail(BBB_EINVAL, "null hist_dev: the histogram is the only output");
    if ((uintptr_t)hist_dev & 7) return fail(BBB_EINVAL, "misaligned hist_dev");
    const int k = lutopt_k(h);
    if (k & (k - 1)) return fail(BBB_EUNSUP, "CLTGRNG needs k to be a power of two (rng.py:72-76)");
    if (k < 2 || (unsigned)k > kHistMaxBins) return fail(BBB_EUNSUP, "the histogram has k bins, k <= 512 (got k = " + std::to_string(k) + ")");
    const int device = lutopt_device(h);
    if (device < 0) return fail(BBB_ENODEV, "host-only handle (device -1) cannot generate samples");
    if (first_step + nsamples < first_step) return fail(BBB_EINVAL, "first_step + nsamples overflows");
    if (nsamples == 0) return BBB_OK;
    int rc = use_device(device);
    if (rc) return rc;
    hipStream_t st = lutopt_stream(h);
    HistCall c;
    c.hist = hist_dev;
    c.blocks = hist_grid_blocks();
    if (c.blocks < 0) return c.blocks;
    // the shipped n256 matrix has the planes form: chunks of 2^24 samples and more never leave the chip
    const bool fused_ok = bbb_lutopt_is_specialised(h) != 0;
    // what goes through memory: everything of another generator, and the pieces of this one that are too short for the planes form
    uint64_t buffered = 0;
    for (uint64_t off = 0; off < nsamples;) {
        const uint64_t n = chunk_of(fused_ok, nsamples - off);
        if (!(fused_ok && n >= kHistFusedMin)) buffered = std::max(buffered, n);
        off += n;
    }
    CallScratch<uint32_t> scratch;                    // released last: the chunk buffer, declared behind it, goes first
    CallScratch<char> buf;
    if ((rc = scratch.alloc((size_t)c.blocks * (size_t)k, st))) return rc;
    c.scratch = scratch;
    // (a fill may write up to the next multiple of 16 samples)
    if (buffered && (rc = buf.alloc((size_t)((buffered + 15) & ~15ull) * (k > 256 ? 2 : 1) + 256, st))) return rc;
    // The planes form runs as the stream does at one read per sample kernel (level 1): the announcements of bbb_awgn_prefetch then
    // match the chunks.  The handle's own level comes back behind the call; what a look-ahead level had produced ahead is
    // dropped, as bbb_lutopt_set_staged says of every call of it.
    const int level = lutopt_staged_level(h);
    const bool relevel = fused_ok && nsamples >= kHistFusedMin && level != 1;
    if (relevel) rc = bbb_lutopt_set_staged(h, 1);
    if (!rc) rc = hist_chunks(h, c, fused_ok, k, buf, nsamples, first_step);
    if (relevel) {
        const int rc2 = bbb_lutopt_set_staged(h, level);
        if (!rc) rc = rc2;
    }
    (void)hipSetDevice(device);                       // for the two releases
    return rc;
}

}  // extern "C"
