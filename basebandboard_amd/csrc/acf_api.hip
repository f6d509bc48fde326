// acf_api.hip -- the extern "C" entry points of the autocorrelation counters (include/bbb.h).  Host logic only: argument
// checks and, on the transmitter side, what a chunk of tx_chunks.hpp's loop does and its scratch.
#include "capture.hpp"
#include "tx_chunks.hpp"

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
    uint32_t nlags = 0;
    AcfPlan plan{};
    DevBuf<uint64_t> scratch;        // per-workgroup partial counters
    DevBuf<int16_t> buf;             // the chunk's waveform and the nlags - 1 (and up to 15 more) samples after it
    TxChunks tx;
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
    CallScratch<uint64_t> scratch;
    if ((rc = scratch.alloc(p.scratch_words, st, scratch_pool(device)))) return rc;
    return acf_launch(p, samples_dev, nfirst, navail, nlags, scratch, reinterpret_cast<uint64_t *>(acf_dev), st);
}

int bbb_tx_acf_open(bbb_lutopt *h, const bbb_tx_cfg *cfg, uint32_t nlags, uint64_t chunk_samples, bbb_tx_acf **out) {
    auto a = std::make_unique<bbb_tx_acf>();
    int rc = tx_chunks_open(&a->tx, h, out, cfg, chunk_samples, kAcfChunkDefault, kAcfChunkMax, [&] {
        const int bad = tx_cfg_check(cfg);
        return bad ? bad : lags_check(nlags);
    });
    if (rc) return rc;
    a->nlags = nlags;
    a->plan = acf_plan(nlags, a->tx.chunk);
    if (a->plan.gx < 0) return fail(BBB_EHIP, "could not size the correlator's grid");
    if ((rc = a->buf.grow(fill_len(a->tx.chunk, nlags))) || (rc = a->scratch.grow(a->plan.scratch_words))) return rc;
    *out = a.release();
    return BBB_OK;
}

int bbb_tx_acf_run(bbb_tx_acf *a, uint64_t first_sample, uint64_t nsamples, int64_t *acf_dev) {
    if (!a) return fail(BBB_EINVAL, "null acf object");
    if (!acf_dev) return fail(BBB_EINVAL, "null acf_dev: the counters are the only output");
    if ((uintptr_t)acf_dev & 7) return fail(BBB_EINVAL, "misaligned device pointer");
    if (first_sample > kAcfSampleLimit - a->nlags - 16 || nsamples > kAcfSampleLimit - a->nlags - 16 - first_sample)
        return fail(BBB_EINVAL, "first_sample + nsamples + nlags + 16 must be <= 2^62");
    // a chunk of n first elements fills (and the chunk before it announces) the samples behind it that its lags reach
    const auto padded = [&](uint64_t first, uint64_t n) { return TxRange{first, fill_len(n, a->nlags)}; };
    return tx_chunks_walk(a->tx, a->buf.p, first_sample, nsamples, padded, [&](uint64_t, uint64_t n, hipStream_t st) {
        return acf_launch(a->plan, a->buf, n, n + a->nlags - 1, a->nlags, a->scratch, reinterpret_cast<uint64_t *>(acf_dev), st);
    });
}

int bbb_tx_acf_close(bbb_tx_acf *a) {
    if (!a) return fail(BBB_EINVAL, "null acf object");
    delete a;
    return BBB_OK;
}

}  // extern "C"
