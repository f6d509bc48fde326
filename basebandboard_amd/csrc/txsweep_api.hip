// txsweep_api.hip -- the extern "C" entry points of the BER sweep over transmitter settings (include/bbb.h).  Host logic
// only: argument checks, the grouping of the settings into launches, the chunk loop and its scratch.  Kept out of
// bbb_api.hip, whose scheduler is compiled unchanged against a model of HIP (tests/sched_model/): the sweep object uses the
// handle only through public calls (bbb_awgn_fill_i8, bbb_awgn_prefetch) and the two accessors that read its device and
// stream.
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

constexpr uint64_t kSweepChunkDefault = 1ull << 26;   // 64 MiB of int8 noise: every launch of a chunk finds it in the Infinity Cache
constexpr uint64_t kSweepChunkMax = 1ull << 30;
constexpr int kSweepMaxSettings = 512;

// the decision x >= t of a setting (strict: x > threshold), t clamped to [-2048, 2048]: x is 12-bit, so nothing changes
int32_t decision_bound(const bbb_tx_setting &s) {
    int64_t t = (int64_t)s.threshold + (s.strict ? 1 : 0);
    return (int32_t)std::max<int64_t>(-2048, std::min<int64_t>(2048, t));
}

uint32_t sat16(int32_t v) { return (uint32_t)(uint16_t)(int16_t)std::max(-32768, std::min(32767, v)); }

}  // namespace

struct bbb_tx_ber_sweep {
    bbb_lutopt *h = nullptr;
    bbb_tx_cfg base{};
    int nset = 0;
    bool any_noise = false;
    uint64_t chunk = 0;
    int device = 0, blocks = 0;
    std::vector<SweepGroup> groups;
    int8_t *noise = nullptr;         // the chunk's noise
    uint64_t *bits = nullptr;        // the chunk's data bits
    uint64_t bits_words = 0;
    int16_t *coeffs = nullptr;       // the distinct coefficient sets
    uint16_t *tables = nullptr;      // their shaped-value tables, 8 x 256 u16 each
    uint32_t *scratch = nullptr;     // per-block partial counts of one launch

    ~bbb_tx_ber_sweep() {
        if (device >= 0) (void)hipSetDevice(device);
        if (noise) (void)hipFree(noise);
        if (bits) (void)hipFree(bits);
        if (coeffs) (void)hipFree(coeffs);
        if (tables) (void)hipFree(tables);
        if (scratch) (void)hipFree(scratch);
    }
};

extern "C" {

int bbb_tx_ber_sweep_open(bbb_lutopt *h, const bbb_tx_cfg *base, const bbb_tx_setting *settings, int nset, uint64_t chunk_samples,
                          bbb_tx_ber_sweep **out) {
    if (!h) return fail(BBB_EINVAL, "null handle");
    if (!out) return fail(BBB_EINVAL, "null out");
    if (!base) return fail(BBB_EINVAL, "null base cfg");
    if (!settings) return fail(BBB_EINVAL, "null settings");
    if (nset < 1 || nset > kSweepMaxSettings)
        return fail(BBB_EINVAL, "nset must be 1.." + std::to_string(kSweepMaxSettings) + " (got " + std::to_string(nset) + ")");
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
    if (chunk_samples > kSweepChunkMax) return fail(BBB_EINVAL, "chunk_samples must be <= 2^30");
    const int device = lutopt_device(h);
    if (device < 0) return fail(BBB_ENODEV, "host-only handle (device -1) cannot generate samples");
    int rc = use_device(device);
    if (rc) return rc;

    auto s = std::make_unique<bbb_tx_ber_sweep>();
    s->h = h;
    s->base = *base;
    s->nset = nset;
    s->device = device;
    s->chunk = chunk_samples ? chunk_samples : kSweepChunkDefault;
    s->blocks = sweep_grid_blocks(s->chunk);
    if (s->blocks < 0) return s->blocks;

    // the distinct shaped-value tables: a setting's coefficient set, or all zeros when its bits are off (tx.py:65-66)
    std::map<std::array<int16_t, 64>, int> table_of;
    std::vector<std::array<int16_t, 64>> sets;
    std::vector<std::vector<int>> members;
    for (int i = 0; i < nset; i++) {
        std::array<int16_t, 64> c{};
        if (settings[i].bit_en) std::memcpy(c.data(), settings[i].coeffs, sizeof c);
        auto it = table_of.find(c);
        if (it == table_of.end()) {
            it = table_of.emplace(c, (int)sets.size()).first;
            sets.push_back(c);
            members.emplace_back();
        }
        members[it->second].push_back(i);
        s->any_noise = s->any_noise || settings[i].noise_en;
    }
    // launches: the settings of one table, zero decision bounds first (those launches skip the threshold step), two per
    // packed lane operation, up to 2 kSweepMaxPairs per launch
    for (int t = 0; t < (int)sets.size(); t++) {
        std::vector<int> &m = members[t];
        std::stable_partition(m.begin(), m.end(), [&](int i) { return decision_bound(settings[i]) == 0; });
        for (size_t at = 0; at < m.size(); at += 2 * kSweepMaxPairs) {
            SweepGroup g{};
            g.table = t;
            const size_t cnt = std::min<size_t>(m.size() - at, 2 * kSweepMaxPairs);
            g.pairs = (int)((cnt + 1) / 2);
            for (int j = 0; j < 2 * kSweepMaxPairs; j++) g.idx[j] = -1;
            for (size_t j = 0; j < cnt; j++) {
                const int i = m[at + j];
                const bbb_tx_setting &st = settings[i];
                const int32_t tb = decision_bound(st);
                const unsigned k = (unsigned)j / 2, sh = 16u * ((unsigned)j & 1u);
                g.idx[j] = i;
                g.nv2[k] |= (uint32_t)(st.noise_en ? st.noise_var : 0) << sh;
                g.t0[k] |= sat16(-16 * tb) << sh;             // data bit 0: ~y < -16 t
                g.t1[k] |= sat16(16 * tb) << sh;              // data bit 1:  y < 16 t
                g.thr = g.thr || tb != 0;
            }
            s->groups.push_back(g);
        }
    }

    // scratch: the chunk's noise and data bits.  Sample n needs the shaper window, bits M-7 .. M with M = floor((n - 17) / 8);
    // a chunk needs at most chunk / 8 + 8 of them, and the window of its last thread reads 2 more
    if (s->any_noise) BBB_HIP(hipMalloc((void **)&s->noise, ((s->chunk + 15) & ~15ull) + 16));
    if (base->source == 0) {
        s->bits_words = (s->chunk / 8 + 16) / 64 + 2;
        BBB_HIP(hipMalloc((void **)&s->bits, s->bits_words * sizeof(uint64_t)));
    }
    BBB_HIP(hipMalloc((void **)&s->scratch, sweep_scratch_words(s->blocks) * sizeof(uint32_t)));
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

int bbb_tx_ber_sweep_run(bbb_tx_ber_sweep *s, uint64_t first_sample, uint64_t nsamples, uint64_t *counters_dev) {
    if (!s) return fail(BBB_EINVAL, "null sweep object");
    if (!counters_dev) return fail(BBB_EINVAL, "null counters_dev");
    if ((uintptr_t)counters_dev & 7) return fail(BBB_EINVAL, "misaligned device pointer");
    if (const int rc = tx_range_check(first_sample, nsamples)) return rc;
    if (nsamples == 0) return BBB_OK;
    if (s->any_noise && s->base.warmup + first_sample + nsamples < nsamples)
        return fail(BBB_EINVAL, "warmup + first_sample + nsamples overflows");
    BBB_HIP(hipSetDevice(s->device));
    int rc;
    for (uint64_t off = 0; off < nsamples;) {
        const uint64_t n = std::min(s->chunk, nsamples - off), first = first_sample + off;
        // 1. the noise, once for every setting: sample n's is the CLT value of state A^(warmup + n + 1) (tx.py:70-71)
        if (s->any_noise) {
            if ((rc = bbb_awgn_fill_i8(s->h, s->noise, n, s->base.warmup + first))) return rc;
            // 2. announce the next chunk, as bbb_tx_eye_run does: its start states are derived beside this chunk's kernels
            if (off + n < nsamples && (rc = bbb_awgn_prefetch(s->h, std::min(s->chunk, nsamples - off - n), s->base.warmup + first + n)))
                return rc;
        }
        hipStream_t st = lutopt_stream(s->h);     // the handle's stream, read per chunk like the fill itself does
        BBB_HIP(hipSetDevice(s->device));
        // 3. the data bits of the chunk's shaper windows (bits below 0 read as 0, the reset shift register); the Pulser's
        // are computed where they are needed
        SweepChunk c{};
        c.noise = s->noise && s->any_noise ? s->noise : nullptr;
        c.source = s->base.source;
        c.first = first;
        c.n = n;
        if (s->base.source == 0) {
            const int64_t lo = std::max<int64_t>(0, floor8((int64_t)first - 17) - 7);
            const int64_t hi = floor8((int64_t)(first + n - 1) - 17) + 2;
            c.bits = reinterpret_cast<const unsigned long long *>(s->bits);
            c.m0 = lo;
            c.navail = hi >= lo ? (uint64_t)(hi - lo + 1) : 0;
            if (c.navail > s->bits_words * 64) return fail(BBB_EINVAL, "internal: sweep bit buffer too small");
            if (c.navail && (rc = bbb_prbs_fill(s->base.prbs_k, s->base.prbs_state, (uint64_t)lo, c.navail, s->bits, s->device, st)))
                return rc;
        }
        // 4. one launch per group of settings; every one re-reads the chunk from the cache
        for (const SweepGroup &g : s->groups)
            if ((rc = sweep_launch(g, s->tables, c, s->scratch, s->blocks, counters_dev, st))) return rc;
        off += n;
    }
    return BBB_OK;
}

int bbb_tx_ber_sweep_close(bbb_tx_ber_sweep *s) {
    if (!s) return fail(BBB_EINVAL, "null sweep object");
    delete s;
    return BBB_OK;
}

}  // extern "C"
