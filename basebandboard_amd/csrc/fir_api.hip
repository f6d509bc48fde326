// fir_api.hip -- the extern "C" entry points of the FIR filter (include/bbb.h, bbb_fir_*).  Host logic only: the checks of
// bbb_fir_cfg, the packing of the taps into the launch structure, and the moving-average presets.
#include "capture.hpp"

#include <algorithm>
#include <cstring>
#include <string>

using namespace bbb;

namespace {

// mode 0 / 1: out_dev holds int16 / int32 samples; 2: packed decisions
int run(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, const bbb_fir_cfg *cfg, int mode, int32_t threshold, int strict,
        void *out_dev, uint64_t *nout_out, int device, hipStream_t st) {
    if (nin > kFirSampleLimit) return fail(BBB_EINVAL, "nin must be <= 2^58");
    if (nin && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    const uint64_t nout = fir_nout(cfg, nin);
    if (nout && !out_dev) return fail(BBB_EINVAL, mode == 2 ? "null bits_packed_dev" : "null out_dev");
    const uint64_t obytes = mode == 2 ? (nout + 63) / 64 * 8 : nout * (mode ? 4 : 2);
    if (((uintptr_t)in_dev & 1) || ((uintptr_t)out_dev & (mode == 2 ? 7 : mode ? 3 : 1))) return fail(BBB_EINVAL, "misaligned device pointer");
    uint32_t before;
    int rc = fir_history(in_dev, nin, nbefore, cfg->ntaps, out_dev, obytes, mode == 2 ? "bits_packed_dev" : "out_dev", &before);
    if (rc) return rc;
    if (nout_out) *nout_out = nout;
    if (nout == 0) return BBB_OK;
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    FirLaunch a{};
    a.in = in_dev;
    a.out = out_dev;
    a.nin = nin;
    a.nout = nout;
    a.nbefore = before;
    a.ngroups = fir_pack_taps(cfg, a.taps);
    a.shift = cfg->shift;
    a.decim = cfg->decim;
    a.phase = cfg->phase;
    a.threshold = threshold;
    a.strict = strict != 0;
    a.in_vec = !((uintptr_t)in_dev & 15);
    a.out_vec = !((uintptr_t)out_dev & 15);
    // decisions of a decimating launch are ORed into the words that two workgroup steps share
    if (mode == 2 && cfg->decim > 1) BBB_HIP(hipMemsetAsync(out_dev, 0, obytes, st));
    return fir_launch(a, mode, std::max(1, cus) * 8, st);
}

}  // namespace

int bbb::fir_cfg_check(const bbb_fir_cfg *c, bool slice) {
    if (!c) return fail(BBB_EINVAL, "null fir cfg");
    if (c->ntaps < 1 || c->ntaps > BBB_FIR_MAX_TAPS) return fail(BBB_EINVAL, "ntaps must be 1..256 (got " + std::to_string(c->ntaps) + ")");
    uint32_t sum = 0;
    for (uint32_t i = 0; i < c->ntaps; ++i) sum += (uint32_t)std::abs((int)c->taps[i]);
    if (sum > 65535) return fail(BBB_EINVAL, "the sum of |taps| must be <= 65535 (got " + std::to_string(sum) + ")");
    if (!slice && c->shift > 31) return fail(BBB_EINVAL, "shift must be 0..31 (got " + std::to_string(c->shift) + ")");
    if (c->decim < 1 || c->decim > 256) return fail(BBB_EINVAL, "decim must be 1..256 (got " + std::to_string(c->decim) + ")");
    if (c->phase >= c->decim) return fail(BBB_EINVAL, "phase must be < decim (got " + std::to_string(c->phase) + ")");
    if (!slice && c->out_bytes != 2 && c->out_bytes != 4)
        return fail(BBB_EINVAL, "out_bytes must be 2 or 4 (got " + std::to_string(c->out_bytes) + ")");
    return BBB_OK;
}

uint32_t bbb::fir_pack_taps(const bbb_fir_cfg *c, uint32_t words[BBB_FIR_MAX_TAPS / 2]) {
    std::memset(words, 0, sizeof(uint32_t) * (BBB_FIR_MAX_TAPS / 2));
    for (uint32_t i = 0; i < c->ntaps; ++i) words[i / 2] |= (uint32_t)(uint16_t)c->taps[i] << (i & 1 ? 0 : 16);
    return (c->ntaps + 7) / 8;
}

extern "C" {

int bbb_fir_moving_average(bbb_fir_cfg *cfg, int pipeline) {
    if (!cfg) return fail(BBB_EINVAL, "null fir cfg");
    std::memset(cfg, 0, sizeof *cfg);
    const int lead = pipeline ? 3 : 0;                  // sr[0] and the two adder stages (average.py:27-33)
    cfg->ntaps = lead + 4;
    for (int i = 0; i < 4; ++i) cfg->taps[lead + i] = 1;
    cfg->decim = 1;
    cfg->out_bytes = 2;
    return BBB_OK;
}

int bbb_fir_filter(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, const bbb_fir_cfg *cfg, void *out_dev,
                   uint64_t *nout_out, int device, void *hip_stream) {
    int rc = fir_cfg_check(cfg, false);
    if (rc) return rc;
    return run(in_dev, nin, nbefore, cfg, cfg->out_bytes == 4 ? 1 : 0, 0, 0, out_dev, nout_out, device, (hipStream_t)hip_stream);
}

int bbb_fir_slice(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, const bbb_fir_cfg *cfg, int32_t threshold,
                  int strict, uint64_t *bits_packed_dev, uint64_t *nbits_out, int device, void *hip_stream) {
    int rc = fir_cfg_check(cfg, true);
    if (rc) return rc;
    return run(in_dev, nin, nbefore, cfg, 2, threshold, strict, bits_packed_dev, nbits_out, device, (hipStream_t)hip_stream);
}

}  // extern "C"
