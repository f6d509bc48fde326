// dfe_api.hip -- the extern "C" entry points of the decision-feedback equalizer (include/bbb.h, bbb_dfe_*).  Host logic only:
// the checks of bbb_dfe_cfg, the launch structure, the call's scratch and the serial host model.
#include "capture.hpp"
#include "dfe_launch.hpp"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

using namespace bbb;

namespace {

// everything wrong with cfg that needs no device; soft: shift and out_bytes count
int cfg_check(const bbb_dfe_cfg *c, bool soft) {
    if (!c) return fail(BBB_EINVAL, "null dfe cfg");
    int rc = fir_cfg_check(&c->ff, !soft);
    if (rc) return rc;
    if (c->nfb > BBB_DFE_MAX_FB) return fail(BBB_EINVAL, "nfb must be 0..4 (got " + std::to_string(c->nfb) + ")");
    int64_t sum_h = 0, sum_fb = 0;
    for (uint32_t i = 0; i < c->ff.ntaps; ++i) sum_h += std::abs((int)c->ff.taps[i]);
    for (uint32_t i = 0; i < c->nfb; ++i) sum_fb += std::llabs((long long)c->fb[i]);
    if (32768 * sum_h + sum_fb > 2147483647ll)
        return fail(BBB_EINVAL, "32768 * sum |ff taps| + sum |fb| must be <= 2^31 - 1 (got " + std::to_string(32768 * sum_h + sum_fb) + ")");
    return BBB_OK;
}

}  // namespace

extern "C" {

int bbb_dfe_geometry(uint32_t decim, uint64_t *step_samples, uint64_t *step_symbols, uint64_t *wave_symbols,
                     uint64_t *region_symbols, uint64_t *warmup_symbols) {
    if (decim < 1 || decim > 256) return fail(BBB_EINVAL, "decim must be 1..256 (got " + std::to_string(decim) + ")");
    if (step_samples) *step_samples = kDfeStepSamples;
    if (step_symbols) *step_symbols = (kDfeStepSamples + decim - 1) / decim;
    if (wave_symbols) *wave_symbols = decim == 1 ? 8 * kWave : kWave;      // the block form: eight symbols per lane
    if (region_symbols) *region_symbols = kDfeRegionDefault;
    if (warmup_symbols) *warmup_symbols = kDfeWarmupDefault;
    return BBB_OK;
}

int bbb_dfe_model_host(const int16_t *in, uint64_t nin, uint32_t nbefore, const bbb_dfe_cfg *cfg, uint32_t *state,
                       uint64_t *bits_packed, void *soft, uint64_t *nbits_out) {
    int rc = cfg_check(cfg, soft != nullptr);
    if (rc) return rc;
    if (nin && !in) return fail(BBB_EINVAL, "null in");
    if (!state) return fail(BBB_EINVAL, "null state");
    const bbb_fir_cfg &ff = cfg->ff;
    const uint64_t nsym = fir_nout(&ff, nin);
    if (nsym && !bits_packed) return fail(BBB_EINVAL, "null bits_packed");
    const uint32_t mask = (1u << cfg->nfb) - 1;
    uint32_t s = *state & mask;
    for (uint64_t w = 0; w < (nsym + 63) / 64; ++w) bits_packed[w] = 0;
    for (uint64_t k = 0; k < nsym; ++k) {
        const int64_t n = (int64_t)(ff.phase + k * ff.decim);
        int64_t v = 0;
        for (uint32_t i = 0; i < ff.ntaps && n - (int64_t)i >= -(int64_t)nbefore; ++i) v += (int64_t)ff.taps[i] * in[n - (int64_t)i];
        for (uint32_t i = 0; i < cfg->nfb; ++i) v -= (s >> i & 1) ? (int64_t)cfg->fb[i] : -(int64_t)cfg->fb[i];
        const bool bit = cfg->strict ? v > cfg->threshold : v >= cfg->threshold;
        bits_packed[k >> 6] |= (uint64_t)bit << (k & 63);
        if (soft) {
            if (ff.out_bytes == 2) ((int16_t *)soft)[k] = (int16_t)std::min<int64_t>(std::max<int64_t>(v >> ff.shift, -32768), 32767);
            else ((int32_t *)soft)[k] = (int32_t)v;
        }
        s = (s << 1 | (uint32_t)bit) & mask;
    }
    *state = s;
    if (nbits_out) *nbits_out = nsym;
    return BBB_OK;
}

int bbb_dfe_run(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, const bbb_dfe_cfg *cfg, uint32_t *state_dev,
                uint64_t *bits_packed_dev, void *soft_dev, uint64_t *stats_dev, uint64_t *nbits_out, int device, void *hip_stream) {
    int rc = cfg_check(cfg, soft_dev != nullptr);
    if (rc) return rc;
    if (nin > kFirSampleLimit) return fail(BBB_EINVAL, "nin must be <= 2^58");
    if (nin && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    if (!state_dev) return fail(BBB_EINVAL, "null state_dev");
    const bbb_fir_cfg &ff = cfg->ff;
    const uint64_t nsym = fir_nout(&ff, nin);
    if (nsym && !bits_packed_dev) return fail(BBB_EINVAL, "null bits_packed_dev");
    const unsigned soft_bytes = ff.out_bytes == 4 ? 4 : 2;
    if (((uintptr_t)in_dev & 1) || ((uintptr_t)bits_packed_dev & 7) || ((uintptr_t)soft_dev & (soft_bytes - 1)) ||
        ((uintptr_t)state_dev & 3) || ((uintptr_t)stats_dev & 7))
        return fail(BBB_EINVAL, "misaligned device pointer");
    const uint64_t bbytes = (nsym + 63) / 64 * 8, sbytes = soft_dev ? nsym * soft_bytes : 0;
    uint32_t before;
    if ((rc = fir_history(in_dev, nin, nbefore, ff.ntaps, bits_packed_dev, bbytes, "bits_packed_dev", &before))) return rc;
    if ((rc = fir_history(in_dev, nin, nbefore, ff.ntaps, soft_dev, sbytes, "soft_dev", &before))) return rc;
    if (overlap(bits_packed_dev, bbytes, soft_dev, sbytes)) return fail(BBB_EINVAL, "soft_dev overlaps bits_packed_dev");
    const uint32_t region = cfg->region_symbols ? cfg->region_symbols : kDfeRegionDefault;
    const uint32_t warmup = cfg->warmup_symbols ? cfg->warmup_symbols : kDfeWarmupDefault;
    const uint64_t nreg = (nsym + region - 1) / region;
    if (nreg > kDfeMaxRegions)
        return fail(BBB_EINVAL, "more than 2^26 regions: raise region_symbols or cut the record (got " + std::to_string(nreg) + ")");
    if (nbits_out) *nbits_out = nsym;
    const hipStream_t st = (hipStream_t)hip_stream;
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    CallScratch<uint64_t> scratch;
    if ((rc = scratch.alloc(dfe_scratch_words(nreg), st))) return rc;
    DfeLaunch a{};
    a.in = in_dev;
    a.nin = nin;
    a.nsym = nsym;
    a.nbefore = before;
    a.ngroups = fir_pack_taps(&ff, a.taps);
    a.shift = soft_dev ? ff.shift : 0;
    a.decim = ff.decim;
    a.phase = ff.phase;
    a.in_vec = !((uintptr_t)in_dev & 15);
    a.nfb = cfg->nfb;
    dfe_rule(a.rule, cfg->fb, cfg->nfb, cfg->threshold, cfg->strict);
    a.region = region;
    a.warmup = warmup;
    a.nreg = nreg;
    a.state = state_dev;
    a.bits = bits_packed_dev;
    a.soft = soft_dev;
    a.soft_bytes = soft_bytes;
    a.rec = scratch;
    a.flagged = scratch + 2 * nreg;
    a.stats = stats_dev;
    // the words that two rounds, steps or regions share are ORed together
    if (bbytes) BBB_HIP(hipMemsetAsync(bits_packed_dev, 0, bbytes, st));
    return dfe_launch(a, cus, st);
}

}  // extern "C"
