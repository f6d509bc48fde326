// sinc_api.hip -- the extern "C" entry points of the 16x sinc interpolator (include/bbb.h, bbb_sinc_*).  Host logic only:
// the coefficient table, argument checks, and the interpolated eye's chunk loop, which uses public calls only
// (bbb_sinc_interpolate into the object's chunk, then bbb_eye_accumulate_i16).
#include "capture.hpp"

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>

using namespace bbb;

namespace {

constexpr uint64_t kSincChunkDefault = 1ull << 24;    // inputs: the best of 2^20, 2^22 and 2^24 measured
constexpr uint64_t kSincChunkMax = 1ull << 27;        // the eye kernel counts at most 2^31 samples per launch
constexpr uint64_t kSincSampleLimit = 1ull << 58;     // first_sample + nin: 16 times that is the eye's own limit

// h[k] = trunc(127 * sinc(t_k) * hamming_k), t = linspace(-4, 4, 128) (sinc.py:38-41).  np.linspace computes
// start + k * step with step = 8 / 127 and puts the last point exactly; np.sinc(t) = sin(pi t) / (pi t), 1 at 0;
// the symmetric Hamming window is 0.54 - 0.46 cos(2 pi k / 127).  No product lies within 0.015 of a non-zero integer
// and the two end values are -4e-16, which truncate to 0 from either side, so libm's last bits cannot change the table.
void table(int8_t h[128]) {
    const double step = 8.0 / 127.0;
    for (int k = 0; k < 128; ++k) {
        const double t = k == 127 ? 4.0 : -4.0 + k * step;
        const double pt = M_PI * t;
        const double s = pt == 0.0 ? 1.0 : std::sin(pt) / pt;
        const double w = 0.54 - 0.46 * std::cos(2.0 * M_PI * k / 127.0);
        h[k] = (int8_t)std::trunc(127.0 * s * w);
    }
}

// the reference's BRAM image (sinc.py:42-48)
void pack(const int8_t h[128], uint32_t words[32]) {
    for (int c = 0; c < 16; ++c)
        for (int half = 0; half < 2; ++half) {
            const int8_t *p = h + 64 * half + c;
            words[2 * c + half] = (uint32_t)(uint8_t)p[0] << 24 | (uint32_t)(uint8_t)p[16] << 16 | (uint32_t)(uint8_t)p[32] << 8 |
                                  (uint32_t)(uint8_t)p[48];
        }
}

int cfg_check(const bbb_sinc_cfg *c, bool eye) {
    if (!c) return fail(BBB_EINVAL, "null sinc cfg");
    if (c->in_bytes != 1 && c->in_bytes != 2) return fail(BBB_EINVAL, "in_bytes must be 1 or 2 (got " + std::to_string(c->in_bytes) + ")");
    if (!eye && c->out_bytes != 1 && c->out_bytes != 2)
        return fail(BBB_EINVAL, "out_bytes must be 1 or 2 (got " + std::to_string(c->out_bytes) + ")");
    if (c->shift > 15) return fail(BBB_EINVAL, "shift must be 0..15 (got " + std::to_string(c->shift) + ")");
    if (c->in_bytes == 1 && c->shift) return fail(BBB_EINVAL, "shift must be 0 with int8 input");
    return BBB_OK;
}

}  // namespace

struct bbb_sinc_eye {
    bbb_sinc_cfg cfg{};
    bbb_eye_cfg eye{};
    uint64_t chunk = 0;
    DevBuf<int16_t> buf;             // the chunk's interpolated samples
    StreamObj on;                    // last: selects the device for the free
};

extern "C" {

int bbb_sinc_coefficients(int8_t h[128]) {
    if (!h) return fail(BBB_EINVAL, "null h");
    table(h);
    return BBB_OK;
}

int bbb_sinc_interpolate(const void *in_dev, uint64_t nin, uint32_t nbefore, const bbb_sinc_cfg *cfg, void *out_dev,
                         int device, void *hip_stream) {
    int rc = cfg_check(cfg, false);
    if (rc) return rc;
    if (nin > kSincSampleLimit) return fail(BBB_EINVAL, "nin must be <= 2^58");
    if (nin && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    if (nin && !out_dev) return fail(BBB_EINVAL, "null out_dev");
    if (((uintptr_t)in_dev & (cfg->in_bytes - 1)) || ((uintptr_t)out_dev & (cfg->out_bytes - 1)))
        return fail(BBB_EINVAL, "misaligned device pointer");
    if (nin == 0) return BBB_OK;
    if ((rc = use_device(device))) return rc;
    int cus = 0;
    if ((rc = device_cus(device, &cus))) return rc;
    SincLaunch a{};
    a.in = in_dev;
    a.out = out_dev;
    a.n = nin;
    a.nbefore = std::min<uint32_t>(nbefore, BBB_SINC_TAPS - 1);
    a.shift = cfg->shift;
    a.vec = !((uintptr_t)out_dev & 15);
    int8_t h[128];
    table(h);
    pack(h, a.words);
    return sinc_launch(a, cfg->in_bytes == 2, cfg->out_bytes == 2, std::max(1, cus) * 8, (hipStream_t)hip_stream);
}

int bbb_sinc_eye_open(const bbb_sinc_cfg *cfg, const bbb_eye_cfg *eye, uint64_t chunk_in, int device, void *hip_stream,
                      bbb_sinc_eye **out) {
    if (!out) return fail(BBB_EINVAL, "null out");
    int rc = cfg_check(cfg, true);
    if (rc) return rc;
    if ((rc = eye_cfg_check(eye))) return rc;
    if (chunk_in > kSincChunkMax) return fail(BBB_EINVAL, "chunk_in must be <= 2^27");
    if ((rc = use_device(device))) return rc;
    auto e = std::make_unique<bbb_sinc_eye>();
    e->cfg = *cfg;
    e->cfg.out_bytes = 2;
    e->eye = *eye;
    e->chunk = chunk_in ? chunk_in : kSincChunkDefault;
    e->on.device = device;
    e->on.st = (hipStream_t)hip_stream;
    if ((rc = e->buf.grow(e->chunk * BBB_SINC_UP))) return rc;
    *out = e.release();
    return BBB_OK;
}

int bbb_sinc_eye_run(bbb_sinc_eye *e, const void *in_dev, uint64_t nin, uint32_t nbefore, uint64_t first_sample,
                     uint64_t *hist_dev) {
    if (!e) return fail(BBB_EINVAL, "null sinc eye object");
    if (!hist_dev) return fail(BBB_EINVAL, "null hist_dev");
    if (nin && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    if (((uintptr_t)in_dev & (e->cfg.in_bytes - 1)) || ((uintptr_t)hist_dev & 7)) return fail(BBB_EINVAL, "misaligned device pointer");
    if (first_sample > kSincSampleLimit || nin > kSincSampleLimit - first_sample)
        return fail(BBB_EINVAL, "first_sample + nin must be <= 2^58");
    for (uint64_t off = 0; off < nin;) {
        const uint64_t n = std::min(e->chunk, nin - off);
        const uint32_t before = (uint32_t)std::min<uint64_t>(off + nbefore, BBB_SINC_TAPS - 1);
        int rc = bbb_sinc_interpolate(static_cast<const char *>(in_dev) + off * e->cfg.in_bytes, n, before, &e->cfg, e->buf,
                                      e->on.device, e->on.st);
        if (rc) return rc;
        if ((rc = bbb_eye_accumulate_i16(e->buf, n * BBB_SINC_UP, (first_sample + off) * BBB_SINC_UP, &e->eye, hist_dev,
                                         e->on.device, e->on.st)))
            return rc;
        off += n;
    }
    return BBB_OK;
}

int bbb_sinc_eye_close(bbb_sinc_eye *e) {
    if (!e) return fail(BBB_EINVAL, "null sinc eye object");
    e->on.drain();
    delete e;
    return BBB_OK;
}

}  // extern "C"
