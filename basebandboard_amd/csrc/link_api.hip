// link_api.hip -- the extern "C" entry points of the filtered link (include/bbb.h, bbb_link_sweep_*).  Host logic only:
// argument checks, the settings' rows, what a chunk of tx_chunks.hpp's loop does and its scratch.
#include "tx_chunks.hpp"

#include <memory>

using namespace bbb;

namespace {

constexpr uint64_t kLinkChunkDefault = 1ull << 26;    // 64 MiB of int8 noise: every launch of a chunk finds it in the Infinity Cache
constexpr uint64_t kLinkChunkMax = 1ull << 30;
constexpr uint32_t kLinkMaxDelay = 255;

struct LinkSetting {
    int table;                    // index into the object's tables
    int nv;                       // noise_var, 0 when the setting's noise is off
    bool noise;
    int32_t threshold, strict;
};

}  // namespace

struct bbb_link_sweep {
    bool have_eye = false;
    bbb_eye_cfg eye{};
    int blocks = 0;
    uint32_t delay = 0, ngroups = 0, shift = 0;
    uint32_t taps[BBB_FIR_MAX_TAPS / 2] = {};
    std::vector<LinkSetting> settings;
    DevBuf<uint32_t> scratch;        // per-block partials of one launch
    ShapedTables shaped;
    DevBuf<uint64_t> bits;           // the chunk's data bits
    DevBuf<int8_t> noise;            // the chunk's noise, with the filter's history in front
    TxChunks tx;
};

extern "C" {

int bbb_link_sweep_open(bbb_lutopt *h, const bbb_tx_cfg *base, const bbb_tx_setting *settings, int nset, const bbb_fir_cfg *fir,
                        uint32_t delay, const bbb_eye_cfg *eye, uint64_t chunk_samples, bbb_link_sweep **out) {
    auto s = std::make_unique<bbb_link_sweep>();
    bool any_noise = false;
    int rc = tx_chunks_open(&s->tx, h, out, base, chunk_samples, kLinkChunkDefault, kLinkChunkMax, [&] {
        if (const int bad = tx_settings_check(base, settings, nset, &any_noise)) return bad;
        // the rules of bbb_fir_cfg (out_bytes is not looked at), and what the link adds to them
        if (const int bad = fir_cfg_check(fir, true)) return bad;
        if (fir->shift > 31) return fail(BBB_EINVAL, "shift must be 0..31 (got " + std::to_string(fir->shift) + ")");
        if (fir->decim != 1) return fail(BBB_EINVAL, "the link's filter runs at decim 1 (got " + std::to_string(fir->decim) + ")");
        if (delay > kLinkMaxDelay) return fail(BBB_EINVAL, "delay must be 0..255 (got " + std::to_string(delay) + ")");
        return eye ? eye_cfg_check(eye) : BBB_OK;
    });
    if (rc) return rc;
    s->tx.cfg.noise_en = any_noise;
    s->have_eye = eye != nullptr;
    if (eye) s->eye = *eye;
    s->delay = delay;
    s->ngroups = fir_pack_taps(fir, s->taps);
    s->shift = fir->shift;
    s->blocks = link_grid_blocks(s->have_eye);
    if (s->blocks < 0) return s->blocks;

    // scratch.  A chunk's launches read the waveform samples [first + delay - 8 ngroups, first + delay + chunk) (those below
    // 0 are 0) and the data bits of link_bit_range
    if (any_noise && (rc = s->noise.grow(((s->tx.chunk + 8 * 32 + 8 + 15) & ~15ull) + 16))) return rc;
    if (base->source == 0 && (rc = s->bits.grow(link_bits_words(s->tx.chunk)))) return rc;
    if ((rc = s->scratch.grow(eye_scratch_words(s->blocks, s->have_eye ? eye->ncols : 0))) ||
        (rc = s->shaped.build(settings, nset, lutopt_stream(h))))
        return rc;
    for (int i = 0; i < nset; i++) {
        LinkSetting ls{};
        ls.table = s->shaped.of[i];
        ls.noise = settings[i].noise_en != 0 && settings[i].noise_var != 0;
        ls.nv = ls.noise ? settings[i].noise_var : 0;
        ls.threshold = settings[i].threshold;
        ls.strict = settings[i].strict != 0;
        s->settings.push_back(ls);
    }
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
    const bbb_tx_cfg &base = s->tx.cfg;
    if (base.noise_en && base.warmup + first_sample + nsamples + s->delay < nsamples + s->delay)
        return fail(BBB_EINVAL, "warmup + first_sample + nsamples overflows");
    const int64_t lead = 8 * (int64_t)s->ngroups;
    // the waveform samples a chunk of stream samples [first, first + n) reads the noise of: the outputs re-timed by the delay,
    // with the filter's history in front
    const auto noise_range = [&](uint64_t first, uint64_t n) {
        const uint64_t norg = (uint64_t)std::max<int64_t>(0, (int64_t)first + s->delay - lead);
        return TxRange{norg, first + s->delay + n - norg};
    };
    return tx_chunks_walk(s->tx, s->noise.p, first_sample, nsamples, noise_range, [&](uint64_t first, uint64_t n, hipStream_t st) {
        const TxRange nr = noise_range(first, n);
        LinkLaunch a{};
        a.norg = (int64_t)nr.first;
        a.nnoise = (nr.n + 7) & ~7ull;
        a.source = base.source;
        a.out_lo = (int64_t)first + s->delay;
        a.out_hi = a.out_lo + (int64_t)n;
        a.tb = a.out_lo - ((a.out_lo - a.norg) & 7);
        a.delay = s->delay;
        a.ngroups = s->ngroups;
        a.shift = s->shift;
        a.ncols = s->have_eye ? s->eye.ncols : 8;
        a.eye_shift = s->eye.shift;
        a.col_origin = s->eye.col_origin;
        std::memcpy(a.taps, s->taps, sizeof a.taps);
        // the data bits of the chunk's shaper windows and decisions; the Pulser's are computed where they are needed
        if (base.source == 0) {
            TxBits b;
            if (const int rc = tx_chunk_bits(s->tx, link_bit_range(a.tb, lead, a.out_hi), s->bits, s->bits.cap - 1, st, &b)) return rc;
            a.bits = reinterpret_cast<const unsigned long long *>(s->bits.p);
            a.m0 = b.lo;
            a.nwords = s->bits.cap;
        }
        // one launch per setting; every one re-reads the chunk from the cache
        const size_t nbins = (size_t)256 * s->eye.ncols;
        for (size_t i = 0; i < s->settings.size(); i++) {
            const LinkSetting &ls = s->settings[i];
            a.noise = ls.noise ? s->noise.p : nullptr;
            a.nv = ls.nv;
            a.table = s->shaped.tables.p + (size_t)ls.table * 8 * 256;
            a.threshold = ls.threshold;
            a.strict = ls.strict;
            if (const int rc = link_launch(a, hist != nullptr, first, n, s->scratch, s->blocks, hist ? hist + i * nbins : nullptr,
                                           counters_dev ? counters_dev + i * 16 : nullptr, st))
                return rc;
        }
        return BBB_OK;
    });
}

int bbb_link_sweep_close(bbb_link_sweep *s) {
    if (!s) return fail(BBB_EINVAL, "null link object");
    delete s;
    return BBB_OK;
}

}  // extern "C"
