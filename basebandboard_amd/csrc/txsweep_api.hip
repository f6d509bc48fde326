// txsweep_api.hip -- the extern "C" entry points of the BER sweep over transmitter settings (include/bbb.h).  Host logic
// only: argument checks, the grouping of the settings into launches, what a chunk of tx_chunks.hpp's loop does and its
// scratch.
#include "tx_chunks.hpp"

#include <memory>

using namespace bbb;

namespace {

constexpr uint64_t kSweepChunkDefault = 1ull << 26;   // 64 MiB of int8 noise: every launch of a chunk finds it in the Infinity Cache
constexpr uint64_t kSweepChunkMax = 1ull << 30;

// the decision x >= t of a setting (strict: x > threshold), t clamped to [-2048, 2048]: x is 12-bit, so nothing changes
int32_t decision_bound(const bbb_tx_setting &s) {
    int64_t t = (int64_t)s.threshold + (s.strict ? 1 : 0);
    return (int32_t)std::max<int64_t>(-2048, std::min<int64_t>(2048, t));
}

uint32_t sat16(int32_t v) { return (uint32_t)(uint16_t)(int16_t)std::max(-32768, std::min(32767, v)); }

}  // namespace

struct bbb_tx_ber_sweep {
    int blocks = 0;
    std::vector<SweepGroup> groups;
    DevBuf<uint32_t> scratch;        // per-block partial counts of one launch
    ShapedTables shaped;
    DevBuf<uint64_t> bits;           // the chunk's data bits
    DevBuf<int8_t> noise;            // the chunk's noise
    TxChunks tx;
};

extern "C" {

int bbb_tx_ber_sweep_open(bbb_lutopt *h, const bbb_tx_cfg *base, const bbb_tx_setting *settings, int nset, uint64_t chunk_samples,
                          bbb_tx_ber_sweep **out) {
    auto s = std::make_unique<bbb_tx_ber_sweep>();
    bool any_noise = false;
    int rc = tx_chunks_open(&s->tx, h, out, base, chunk_samples, kSweepChunkDefault, kSweepChunkMax,
                            [&] { return tx_settings_check(base, settings, nset, &any_noise); });
    if (rc) return rc;
    s->tx.cfg.noise_en = any_noise;
    s->blocks = sweep_grid_blocks(s->tx.chunk);
    if (s->blocks < 0) return s->blocks;

    // scratch: the chunk's noise and data bits
    if (any_noise && (rc = s->noise.grow(((s->tx.chunk + 15) & ~15ull) + 16))) return rc;
    if (base->source == 0 && (rc = s->bits.grow(sweep_bits_words(s->tx.chunk)))) return rc;
    if ((rc = s->scratch.grow(sweep_scratch_words(s->blocks))) || (rc = s->shaped.build(settings, nset, lutopt_stream(h)))) return rc;

    std::vector<std::vector<int>> members(s->shaped.ntab);
    for (int i = 0; i < nset; i++) members[s->shaped.of[i]].push_back(i);
    // launches: the settings of one table, zero decision bounds first (those launches skip the threshold step), two per
    // packed lane operation, up to 2 kSweepMaxPairs per launch
    for (int t = 0; t < s->shaped.ntab; t++) {
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
    *out = s.release();
    return BBB_OK;
}

int bbb_tx_ber_sweep_run(bbb_tx_ber_sweep *s, uint64_t first_sample, uint64_t nsamples, uint64_t *counters_dev) {
    if (!s) return fail(BBB_EINVAL, "null sweep object");
    if (!counters_dev) return fail(BBB_EINVAL, "null counters_dev");
    if ((uintptr_t)counters_dev & 7) return fail(BBB_EINVAL, "misaligned device pointer");
    if (const int rc = tx_range_check(first_sample, nsamples)) return rc;
    if (nsamples == 0) return BBB_OK;
    const bbb_tx_cfg &base = s->tx.cfg;
    if (base.noise_en && base.warmup + first_sample + nsamples < nsamples)
        return fail(BBB_EINVAL, "warmup + first_sample + nsamples overflows");
    return tx_chunks_walk(s->tx, s->noise.p, first_sample, nsamples, tx_same_range, [&](uint64_t first, uint64_t n, hipStream_t st) {
        // the data bits of the chunk's shaper windows; the Pulser's are computed where they are needed
        SweepChunk c{};
        c.noise = s->noise;
        c.source = base.source;
        c.first = first;
        c.n = n;
        if (base.source == 0) {
            TxBits b;
            if (const int rc = tx_chunk_bits(s->tx, sweep_bit_range(first, n), s->bits, s->bits.cap, st, &b)) return rc;
            c.bits = reinterpret_cast<const unsigned long long *>(s->bits.p);
            c.m0 = b.lo;
            c.navail = b.n;
        }
        // one launch per group of settings; every one re-reads the chunk from the cache
        for (const SweepGroup &g : s->groups)
            if (const int rc = sweep_launch(g, s->shaped.tables, c, s->scratch, s->blocks, counters_dev, st)) return rc;
        return BBB_OK;
    });
}

int bbb_tx_ber_sweep_close(bbb_tx_ber_sweep *s) {
    if (!s) return fail(BBB_EINVAL, "null sweep object");
    delete s;
    return BBB_OK;
}

}  // extern "C"
