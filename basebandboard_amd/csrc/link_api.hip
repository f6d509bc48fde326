// link_api.hip -- the extern "C" entry points of the filtered link (include/bbb.h, bbb_link_sweep_*).  Host logic only:
// argument checks, the settings' tables, the chunk loop and its scratch.  Like txsweep_api.hip it is kept out of bbb_api.hip:
// the object uses the handle only through public calls (bbb_awgn_fill_i8, bbb_awgn_prefetch) and the two accessors that read
// its device and stream.
#include "bbb_common.hpp"

#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

using namespace bbb;

namespace {

constexpr uint64_t kLinkChunkDefault = 1ull << 26;    // 64 MiB of int8 noise: every launch of a chunk finds it in the Infinity Cache
constexpr uint64_t kLinkChunkMax = 1ull << 30;
constexpr int kLinkMaxSettings = 512;
constexpr uint32_t kLinkMaxDelay = 255;

struct LinkSetting {
    int table;                    // index into the object's tables
    int nv;                       // noise_var, 0 when the setting's noise is off
    bool noise;
    int32_t threshold, strict;
};

}  // namespace

struct bbb_link_sweep {
    bbb_lutopt *h = nullptr;
    bbb_tx_cfg base{};
    bool any_noise = false, have_eye = false;
    bbb_eye_cfg eye{};
    uint64_t chunk = 0;
    int device = 0, blocks = 0;
    uint32_t delay = 0, ngroups = 0, shift = 0;
    uint32_t taps[BBB_FIR_MAX_TAPS / 2] = {};
    std::vector<LinkSetting> settings;
    int8_t *noise = nullptr;         // the chunk's noise, with the filter's history in front
    uint64_t *bits = nullptr;        // the chunk's data bits
    uint64_t bits_words = 0;
    int16_t *coeffs = nullptr;       // the distinct coefficient sets
    uint16_t *tables = nullptr;      // their shaped-value tables, 8 x 256 u16 each
    uint32_t *scratch = nullptr;     // per-block partials of one launch

    ~bbb_link_sweep() {
        if (device >= 0) (void)hipSetDevice(device);
        if (noise) (void)hipFree(noise);
        if (bits) (void)hipFree(bits);
        if (coeffs) (void)hipFree(coeffs);
        if (tables) (void)hipFree(tables);
        if (scratch) (void)hipFree(scratch);
    }
};

extern "C" {

int bbb_link_sweep_open(bbb_lutopt *h, const bbb_tx_cfg *base, const bbb_tx_setting *settings, int nset, const bbb_fir_cfg *fir,
                        uint32_t delay, const bbb_eye_cfg *eye, uint64_t chunk_samples, bbb_link_sweep **out) {
    if (!h) return fail(BBB_EINVAL, "null handle");
    if (!out) return fail(BBB_EINVAL, "null out");
    if (!base) return fail(BBB_EINVAL, "null base cfg");
    if (!settings) return fail(BBB_EINVAL, "null settings");
    if (nset < 1 || nset > kLinkMaxSettings)
        return fail(BBB_EINVAL, "nset must be 1.." + std::to_string(kLinkMaxSettings) + " (got " + std::to_string(nset) + ")");
    for (int i = 0; i < nset; i++) {
        const bbb_tx_setting &st = settings[i];
        if (st.reserved != 0) return fail(BBB_EINVAL, "bbb_tx_setting.reserved must be 0 (setting " + std::to_string(i) + ")");
        // the checks of bbb_tx_fill_i16 on the cfg this setting stands for
        bbb_tx_cfg c = *base;
        std::memcpy(c.coeffs, st.coeffs, sizeof c.coeffs);
        c.bit_en = st.bit_en;
        c.noise_en = st.noise_en;
        c.noise_var = st.noise_var;
        if (const int rc = tx_cfg_check(&c)) return fail(rc, last_error() + " (setting " + std::to_string(i) + ")");
    }
    // the rules of bbb_fir_cfg (out_bytes is not looked at), and what the link adds to them
    if (const int rc = fir_cfg_check(fir, true)) return rc;
    if (fir->shift > 31) return fail(BBB_EINVAL, "shift must be 0..31 (got " + std::to_string(fir->shift) + ")");
    if (fir->decim != 1) return fail(BBB_EINVAL, "the link's filter runs at decim 1 (got " + std::to_string(fir->decim) + ")");
    if (delay > kLinkMaxDelay) return fail(BBB_EINVAL, "delay must be 0..255 (got " + std::to_string(delay) + ")");
    if (eye)
        if (const int rc = eye_cfg_check(eye)) return rc;
    if (chunk_samples > kLinkChunkMax) return fail(BBB_EINVAL, "chunk_samples must be <= 2^30");
    const int device = lutopt_device(h);
    if (device < 0) return fail(BBB_ENODEV, "host-only handle (device -1) cannot generate samples");
    int rc = use_device(device);
    if (rc) return rc;

    auto s = std::make_unique<bbb_link_sweep>();
    s->h = h;
    s->base = *base;
    s->device = device;
    s->chunk = chunk_samples ? chunk_samples : kLinkChunkDefault;
    s->have_eye = eye != nullptr;
    if (eye) s->eye = *eye;
    s->delay = delay;
    s->ngroups = fir_pack_taps(fir, s->taps);
    s->shift = fir->shift;
    s->blocks = link_grid_blocks(s->have_eye);
    if (s->blocks < 0) return s->blocks;

    // the distinct shaped-value tables: a setting's coefficient set, or all zeros when its bits are off (tx.py:65-66)
    std::map<std::array<int16_t, 64>, int> table_of;
    std::vector<std::array<int16_t, 64>> sets;
    for (int i = 0; i < nset; i++) {
        std::array<int16_t, 64> c{};
        if (settings[i].bit_en) std::memcpy(c.data(), settings[i].coeffs, sizeof c);
        auto it = table_of.find(c);
        if (it == table_of.end()) {
            it = table_of.emplace(c, (int)sets.size()).first;
            sets.push_back(c);
        }
        LinkSetting ls{};
        ls.table = it->second;
        ls.noise = settings[i].noise_en != 0 && settings[i].noise_var != 0;
        ls.nv = ls.noise ? settings[i].noise_var : 0;
        ls.threshold = settings[i].threshold;
        ls.strict = settings[i].strict != 0;
        s->settings.push_back(ls);
        s->any_noise = s->any_noise || settings[i].noise_en;
    }

    // scratch.  A chunk's launches read the waveform samples [first + delay - 8 ngroups, first + delay + chunk) (those below
    // 0 are 0) and the data bits of their shaper windows with 47 bits below them, where the decided bits lie
    if (s->any_noise) BBB_HIP(hipMalloc((void **)&s->noise, ((s->chunk + 8 * 32 + 8 + 15) & ~15ull) + 16));
    if (base->source == 0) {
        s->bits_words = (s->chunk / 8 + 160) / 64 + 4;
        BBB_HIP(hipMalloc((void **)&s->bits, s->bits_words * sizeof(uint64_t)));
    }
    BBB_HIP(hipMalloc((void **)&s->scratch, eye_scratch_words(s->blocks, s->have_eye ? eye->ncols : 0) * sizeof(uint32_t)));
    const int ntab = (int)sets.size();
    BBB_HIP(hipMalloc((void **)&s->coeffs, (size_t)ntab * 64 * sizeof(int16_t)));
    BBB_HIP(hipMalloc((void **)&s->tables, (size_t)ntab * 8 * 256 * sizeof(uint16_t)));
    BBB_HIP(hipMemcpy(s->coeffs, sets.data(), (size_t)ntab * 64 * sizeof(int16_t), hipMemcpyHostToDevice));
    hipStream_t st = lutopt_stream(h);
    if ((rc = sweep_tables_launch(s->coeffs, ntab, s->tables, st))) return rc;
    BBB_HIP(hipStreamSynchronize(st));             // run may be called on another stream the handle is bound to later
    *out = s.release();
    return BBB_OK;
}

int bbb_link_sweep_run(bbb_link_sweep *s, uint64_t first_sample, uint64_t nsamples, uint64_t *counters_dev, uint64_t *hist_dev) {
    if (!s) return fail(BBB_EINVAL, "null link object");
    uint64_t *hist = s->have_eye ? hist_dev : nullptr;
    if (!counters_dev && !hist) return fail(BBB_EINVAL, "counters_dev is NULL and there is no histogram to fill");
    if (((uintptr_t)counters_dev & 7) || ((uintptr_t)hist_dev & 7)) return fail(BBB_EINVAL, "misaligned device pointer");
    if (const int rc = tx_range_check(first_sample, nsamples)) return rc;
    if (nsamples == 0) return BBB_OK;
    if (s->any_noise && s->base.warmup + first_sample + nsamples + s->delay < nsamples + s->delay)
        return fail(BBB_EINVAL, "warmup + first_sample + nsamples overflows");
    BBB_HIP(hipSetDevice(s->device));
    const int64_t lead = 8 * (int64_t)s->ngroups;
    // the waveform samples a chunk of stream samples [first, first + n) reads the noise of: [norg, out_hi)
    auto noise_range = [&](uint64_t first, uint64_t n, int64_t *norg, int64_t *out_lo, int64_t *out_hi) {
        *out_lo = (int64_t)first + s->delay;
        *out_hi = *out_lo + (int64_t)n;
        *norg = std::max<int64_t>(0, *out_lo - lead);
    };
    int rc;
    for (uint64_t off = 0; off < nsamples;) {
        const uint64_t n = std::min(s->chunk, nsamples - off), first = first_sample + off;
        int64_t norg, out_lo, out_hi;
        noise_range(first, n, &norg, &out_lo, &out_hi);
        // 1. the noise, once for every setting: sample j's is the CLT value of state A^(warmup + j + 1) (tx.py:70-71)
        if (s->any_noise) {
            if ((rc = bbb_awgn_fill_i8(s->h, s->noise, (uint64_t)(out_hi - norg), s->base.warmup + (uint64_t)norg))) return rc;
            // 2. announce the next chunk, as bbb_tx_eye_run does: its start states are derived beside this chunk's kernels
            if (off + n < nsamples) {
                int64_t norg2, lo2, hi2;
                noise_range(first + n, std::min(s->chunk, nsamples - off - n), &norg2, &lo2, &hi2);
                if ((rc = bbb_awgn_prefetch(s->h, (uint64_t)(hi2 - norg2), s->base.warmup + (uint64_t)norg2))) return rc;
            }
        }
        hipStream_t st = lutopt_stream(s->h);     // the handle's stream, read per chunk like the fill itself does
        BBB_HIP(hipSetDevice(s->device));
        LinkLaunch a{};
        a.norg = norg;
        a.nnoise = ((uint64_t)(out_hi - norg) + 7) & ~7ull;
        a.source = s->base.source;
        a.tb = out_lo - ((out_lo - norg) & 7);
        a.out_lo = out_lo;
        a.out_hi = out_hi;
        a.delay = s->delay;
        a.ngroups = s->ngroups;
        a.shift = s->shift;
        a.ncols = s->have_eye ? s->eye.ncols : 8;
        a.eye_shift = s->eye.shift;
        a.col_origin = s->eye.col_origin;
        std::memcpy(a.taps, s->taps, sizeof a.taps);
        // 3. the data bits of the chunk's shaper windows and decisions (bits below 0 read as 0, the reset shift register);
        // the Pulser's are computed where they are needed
        if (s->base.source == 0) {
            // a thread looks at the 10 bits of its shaper window and up to 47 bits below them (link_kernels.hip)
            const int64_t lo = std::max<int64_t>(0, floor8(std::max<int64_t>(0, a.tb - lead) - 17) - 47);
            const int64_t hi = floor8(out_hi - 1 - 17) + 2;
            const uint64_t nbits = hi >= lo ? (uint64_t)(hi - lo + 1) : 0;
            a.bits = reinterpret_cast<const unsigned long long *>(s->bits);
            a.m0 = lo;
            a.nwords = s->bits_words;
            if (nbits + 64 > s->bits_words * 64) return fail(BBB_EINVAL, "internal: link bit buffer too small");
            if (nbits && (rc = bbb_prbs_fill(s->base.prbs_k, s->base.prbs_state, (uint64_t)lo, nbits, s->bits, s->device, st)))
                return rc;
        }
        // 4. one launch per setting; every one re-reads the chunk from the cache
        const size_t nbins = (size_t)256 * s->eye.ncols;
        for (size_t i = 0; i < s->settings.size(); i++) {
            const LinkSetting &ls = s->settings[i];
            a.noise = ls.noise ? s->noise : nullptr;
            a.nv = ls.nv;
            a.table = s->tables + (size_t)ls.table * 8 * 256;
            a.threshold = ls.threshold;
            a.strict = ls.strict;
            if ((rc = link_launch(a, hist != nullptr, first, n, s->scratch, s->blocks, hist ? hist + i * nbins : nullptr,
                                  counters_dev ? counters_dev + i * 16 : nullptr, st)))
                return rc;
        }
        off += n;
    }
    return BBB_OK;
}

int bbb_link_sweep_close(bbb_link_sweep *s) {
    if (!s) return fail(BBB_EINVAL, "null link object");
    delete s;
    return BBB_OK;
}

}  // extern "C"
