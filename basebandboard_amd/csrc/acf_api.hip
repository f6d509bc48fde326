// acf_api.hip -- the extern "C" entry points of the autocorrelation counters (include/bbb.h).  Host logic only: argument
// checks, the transmitter side's chunk loop and its scratch.  Like eye_api.hip, it uses a handle only through public calls
// (bbb_tx_fill_i16, bbb_awgn_prefetch) and the accessors of bbb_common.hpp, so bbb_api.hip's scheduler model is unchanged.
#include "bbb_common.hpp"

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>

using namespace bbb;

namespace {

constexpr uint64_t kAcfChunkDefault = 1ull << 26;     // 128 MiB of int16: the correlator finds the chunk in the Infinity Cache
constexpr uint64_t kAcfChunkMax = 1ull << 30;
constexpr uint64_t kAcfSampleLimit = 1ull << 62;

int lags_check(uint32_t nlags) {
    if (nlags == 0 || nlags > BBB_ACF_MAX_LAGS)
        return fail(BBB_EINVAL, "nlags must be 1.." + std::to_string(BBB_ACF_MAX_LAGS) + " (got " + std::to_string(nlags) + ")");
    return BBB_OK;
}

// the fill of a chunk of n first elements: n + nlags - 1 samples, rounded up to 16 (the length the fills' look-ahead serves)
uint64_t fill_len(uint64_t n, uint32_t nlags) { return (n + nlags - 1 + 15) & ~15ull; }

// The capture side's scratch comes from a pool of the library's own that keeps what is freed (release threshold: never),
// so that a call does not map and unmap its slab every time as the device's default pool does after a synchronisation.
// nullptr (a runtime without pools): the default pool.
hipMemPool_t scratch_pool(int device) {
    static std::mutex mu;
    static hipMemPool_t pools[64];
    static bool tried[64];
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!tried[device]) {
        tried[device] = true;
        hipMemPoolProps props{};
        props.allocType = hipMemAllocationTypePinned;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = device;
        hipMemPool_t p = nullptr;
        uint64_t keep = ~0ull;
        if (hipMemPoolCreate(&p, &props) == hipSuccess) {
            if (hipMemPoolSetAttribute(p, hipMemPoolAttrReleaseThreshold, &keep) == hipSuccess) pools[device] = p;
            else (void)hipMemPoolDestroy(p);
        }
    }
    return pools[device];
}

}  // namespace

struct bbb_tx_acf {
    bbb_lutopt *h = nullptr;
    bbb_tx_cfg cfg{};
    uint32_t nlags = 0;
    uint64_t chunk = 0;
    int device = 0;
    AcfPlan plan{};
    int16_t *buf = nullptr;          // the chunk's waveform and the nlags - 1 (and up to 15 more) samples after it
    uint64_t *scratch = nullptr;     // per-workgroup partial counters

    ~bbb_tx_acf() {
        if (device >= 0) (void)hipSetDevice(device);
        if (buf) (void)hipFree(buf);
        if (scratch) (void)hipFree(scratch);
    }
};

extern "C" {

int bbb_acf_accumulate_i16(const int16_t *samples_dev, uint64_t nfirst, uint64_t navail, uint32_t nlags, int64_t *acf_dev,
                           int device, void *hip_stream) {
    int rc = lags_check(nlags);
    if (rc) return rc;
    if (!acf_dev) return fail(BBB_EINVAL, "null acf_dev: the counters are the only output");
    if (navail < nfirst) return fail(BBB_EINVAL, "navail must be >= nfirst");
    if (navail > kAcfSampleLimit) return fail(BBB_EINVAL, "navail must be <= 2^62");
    if (nfirst && !samples_dev) return fail(BBB_EINVAL, "null samples_dev");
    if (((uintptr_t)samples_dev & 1) || ((uintptr_t)acf_dev & 7)) return fail(BBB_EINVAL, "misaligned device pointer");
    if (nfirst == 0) return BBB_OK;
    if ((rc = use_device(device))) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    const AcfPlan p = acf_plan(nlags, nfirst);
    if (p.gx < 0) return fail(BBB_EHIP, "could not size the correlator's grid");
    // the slab belongs to this call (stream-ordered allocation, as bbb_eye_accumulate_i16's)
    uint64_t *scratch = nullptr;
    if (hipMemPool_t pool = scratch_pool(device))
        BBB_HIP(hipMallocFromPoolAsync((void **)&scratch, p.scratch_words * sizeof(uint64_t), pool, st));
    else
        BBB_HIP(hipMallocAsync((void **)&scratch, p.scratch_words * sizeof(uint64_t), st));
    rc = acf_launch(p, samples_dev, nfirst, navail, nlags, scratch, reinterpret_cast<uint64_t *>(acf_dev), st);
    (void)hipFreeAsync(scratch, st);
    return rc;
}

int bbb_tx_acf_open(bbb_lutopt *h, const bbb_tx_cfg *cfg, uint32_t nlags, uint64_t chunk_samples, bbb_tx_acf **out) {
    if (!h) return fail(BBB_EINVAL, "null handle");
    if (!out) return fail(BBB_EINVAL, "null out");
    int rc = tx_cfg_check(cfg);
    if (rc) return rc;
    if ((rc = lags_check(nlags))) return rc;
    if (chunk_samples > kAcfChunkMax) return fail(BBB_EINVAL, "chunk_samples must be <= 2^30");
    const int device = lutopt_device(h);
    if (device < 0) return fail(BBB_ENODEV, "host-only handle (device -1) cannot generate samples");
    if ((rc = use_device(device))) return rc;
    auto a = std::make_unique<bbb_tx_acf>();
    a->h = h;
    a->cfg = *cfg;
    a->nlags = nlags;
    a->device = device;
    a->chunk = chunk_samples ? chunk_samples : kAcfChunkDefault;
    a->plan = acf_plan(nlags, a->chunk);
    if (a->plan.gx < 0) return fail(BBB_EHIP, "could not size the correlator's grid");
    BBB_HIP(hipMalloc((void **)&a->buf, fill_len(a->chunk, nlags) * sizeof(int16_t)));
    BBB_HIP(hipMalloc((void **)&a->scratch, a->plan.scratch_words * sizeof(uint64_t)));
    *out = a.release();
    return BBB_OK;
}

int bbb_tx_acf_run(bbb_tx_acf *a, uint64_t first_sample, uint64_t nsamples, int64_t *acf_dev) {
    if (!a) return fail(BBB_EINVAL, "null acf object");
    if (!acf_dev) return fail(BBB_EINVAL, "null acf_dev: the counters are the only output");
    if ((uintptr_t)acf_dev & 7) return fail(BBB_EINVAL, "misaligned device pointer");
    if (first_sample > kAcfSampleLimit - a->nlags - 16 || nsamples > kAcfSampleLimit - a->nlags - 16 - first_sample)
        return fail(BBB_EINVAL, "first_sample + nsamples + nlags + 16 must be <= 2^62");
    if (nsamples == 0) return BBB_OK;
    BBB_HIP(hipSetDevice(a->device));
    const uint64_t look = a->nlags - 1;
    int rc;
    for (uint64_t off = 0; off < nsamples;) {
        const uint64_t n = std::min(a->chunk, nsamples - off), s = first_sample + off;
        if ((rc = bbb_tx_fill_i16(a->h, &a->cfg, a->buf, fill_len(n, a->nlags), s))) return rc;
        // announce the next chunk's fill, as bbb_tx_eye_run does: its noise start states are derived beside this chunk
        if (a->cfg.noise_en && off + n < nsamples &&
            (rc = bbb_awgn_prefetch(a->h, fill_len(std::min(a->chunk, nsamples - off - n), a->nlags), a->cfg.warmup + s + n)))
            return rc;
        hipStream_t st = lutopt_stream(a->h);     // the handle's stream, read per chunk like the fill itself does
        BBB_HIP(hipSetDevice(a->device));
        if ((rc = acf_launch(a->plan, a->buf, n, n + look, a->nlags, a->scratch, reinterpret_cast<uint64_t *>(acf_dev), st)))
            return rc;
        off += n;
    }
    return BBB_OK;
}

int bbb_tx_acf_close(bbb_tx_acf *a) {
    if (!a) return fail(BBB_EINVAL, "null acf object");
    delete a;
    return BBB_OK;
}

}  // extern "C"
