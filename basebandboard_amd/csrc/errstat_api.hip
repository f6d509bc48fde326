// errstat_api.hip -- the extern "C" entry points of the error statistics (include/bbb.h, bbb_errstat_*).  Host logic only:
// argument checks, the object's device memory (the result, which holds every counter and the carried state, and the tile
// summaries of one launch) and the loop over launches.
#include "capture.hpp"

#include <algorithm>
#include <memory>
#include <string>

using namespace bbb;

namespace {

int cfg_check(const bbb_errstat_cfg *c) {
    if (!c) return fail(BBB_EINVAL, "null cfg");
    if (c->nblock > 4) return fail(BBB_EINVAL, "nblock must be <= 4 (got " + std::to_string(c->nblock) + ")");
    for (uint32_t j = 0; j < c->nblock; ++j)
        if (c->block_bits[j] >= (1ull << 40))
            return fail(BBB_EINVAL, "block_bits[" + std::to_string(j) + "] must be in [1, 2^40), or 0 for an unused entry (got " +
                                        std::to_string(c->block_bits[j]) + ")");
    return BBB_OK;
}

}  // namespace

struct bbb_errstat {
    bbb_errstat_cfg cfg{};
    bool ended = false;                   // a call with nbits % 64 != 0 was queued: the record is over until reset
    DevBuf<unsigned char> scratch;        // the tile summaries of one launch: errstat_scratch_bytes()
    DevBuf<bbb_errstat_result> res;       // every counter and the carried state
    StreamObj on;                         // last: selects the device for the frees (res, then scratch)
};

extern "C" {

int bbb_errstat_geometry(uint64_t *tile_bits, uint64_t *wave_bits) {
    if (!tile_bits || !wave_bits) return fail(BBB_EINVAL, "null tile_bits or wave_bits");
    *tile_bits = kErrTileBits;
    *wave_bits = kErrWaveBits;
    return BBB_OK;
}

int bbb_errstat_open(const bbb_errstat_cfg *cfg, int device, void *hip_stream, bbb_errstat **out) {
    if (!out) return fail(BBB_EINVAL, "null out");
    int rc = cfg_check(cfg);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    auto e = std::make_unique<bbb_errstat>();
    e->on.device = device;
    e->on.st = (hipStream_t)hip_stream;
    e->cfg = *cfg;
    if ((rc = e->res.grow(1)) || (rc = e->scratch.grow(errstat_scratch_bytes()))) return rc;
    BBB_HIP(hipMemsetAsync(e->res, 0, sizeof(bbb_errstat_result), e->on.st));
    *out = e.release();
    return BBB_OK;
}

int bbb_errstat_accumulate(bbb_errstat *e, const uint64_t *err_packed_dev, const uint64_t *mask_packed_dev, uint64_t nbits) {
    if (!e) return fail(BBB_EINVAL, "null errstat object");
    if (e->ended) return fail(BBB_EINVAL, "the record ended with a call whose nbits was no multiple of 64: reset first");
    if (nbits == 0) return BBB_OK;
    if (!err_packed_dev) return fail(BBB_EINVAL, "null err_packed_dev");
    if (((uintptr_t)err_packed_dev & 7) || ((uintptr_t)mask_packed_dev & 7)) return fail(BBB_EINVAL, "misaligned device pointer");
    BBB_HIP(hipSetDevice(e->on.device));
    ErrLaunch a{};
    a.guard = e->cfg.guard;
    a.nblock = e->cfg.nblock;
    std::copy(e->cfg.block_bits, e->cfg.block_bits + 4, a.block);
    a.vec = !(((uintptr_t)err_packed_dev | (uintptr_t)mask_packed_dev) & 15);
    for (uint64_t off = 0; off < nbits; off += kErrLaunchBits) {   // a multiple of 128 bits: a launch keeps the alignment
        a.nbits = std::min(kErrLaunchBits, nbits - off);
        a.err = err_packed_dev + off / 64;
        a.mask = mask_packed_dev ? mask_packed_dev + off / 64 : nullptr;
        int rc = errstat_launch(a, e->res, e->scratch, e->on.st);
        if (rc) return rc;
    }
    if (nbits & 63) e->ended = true;
    return BBB_OK;
}

int bbb_errstat_skip(bbb_errstat *e, uint64_t nbits) {
    if (!e) return fail(BBB_EINVAL, "null errstat object");
    if (e->ended) return fail(BBB_EINVAL, "the record ended with a call whose nbits was no multiple of 64: reset first");
    if (nbits == 0) return BBB_OK;
    BBB_HIP(hipSetDevice(e->on.device));
    int rc = errstat_skip_launch(e->res, nbits, e->on.st);
    if (rc) return rc;
    if (nbits & 63) e->ended = true;
    return BBB_OK;
}

int bbb_errstat_read(bbb_errstat *e, bbb_errstat_result *out) {
    if (!e) return fail(BBB_EINVAL, "null errstat object");
    if (!out) return fail(BBB_EINVAL, "null result");
    BBB_HIP(hipSetDevice(e->on.device));
    auto r = std::make_unique<bbb_errstat_result>();
    BBB_HIP(hipMemcpyAsync(r.get(), e->res, sizeof *r, hipMemcpyDeviceToHost, e->on.st));
    BBB_HIP(hipStreamSynchronize(e->on.st));
    *out = *r;
    return BBB_OK;
}

int bbb_errstat_reset(bbb_errstat *e) {
    if (!e) return fail(BBB_EINVAL, "null errstat object");
    BBB_HIP(hipSetDevice(e->on.device));
    BBB_HIP(hipMemsetAsync(e->res, 0, sizeof(bbb_errstat_result), e->on.st));
    e->ended = false;
    return BBB_OK;
}

int bbb_errstat_set_stream(bbb_errstat *e, void *hip_stream) {
    if (!e) return fail(BBB_EINVAL, "null errstat object");
    return e->on.rebind((hipStream_t)hip_stream);
}

int bbb_errstat_close(bbb_errstat *e) {
    if (!e) return fail(BBB_EINVAL, "null errstat object");
    e->on.drain();
    delete e;
    return BBB_OK;
}

}  // extern "C"
