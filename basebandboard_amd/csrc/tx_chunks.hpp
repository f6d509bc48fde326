// tx_chunks.hpp -- what the objects that walk the transmitter's waveform chunk by chunk share (bbb_tx_eye, bbb_tx_ber_sweep,
// bbb_tx_acf, bbb_link_sweep, bbb_tx_xcorr): the opening checks, the chunk loop, a chunk's data bits, and the settings and
// shaped-value tables of the two sweeps.  Host only: no kernel file includes it.  The objects use a handle only through
// public calls (bbb_tx_fill_i16, bbb_awgn_fill_i8, bbb_awgn_prefetch, bbb_prbs_fill) and the accessors of bbb_common.hpp, so
// bbb_api.hip's scheduler is compiled unchanged against a model of HIP (tests/sched_model/) -- and so are they.
#pragma once
#include "bbb_common.hpp"
#include "dev_buf.hpp"

#include <array>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace bbb {

// Declared LAST in its object: destroyed first, it selects the device for the frees of the DevBufs declared before it
// (which go in reverse order of declaration).
struct TxChunks {
    bbb_lutopt *h = nullptr;
    bbb_tx_cfg cfg{};                // the sweeps: the base cfg, noise_en standing for "some setting has its noise on"
    uint64_t chunk = 0;
    int device = -1;
    ~TxChunks() { if (device >= 0) (void)hipSetDevice(device); }
};

// The opening checks of every *_open, in their order; `own` makes the object's own argument checks (*cfg among them) where
// they have always stood: behind the two null checks, in front of chunk_samples.  chunk_max is a power of two.  Leaves the
// handle's device selected.
template <class Own>
int tx_chunks_open(TxChunks *t, bbb_lutopt *h, const void *out, const bbb_tx_cfg *cfg, uint64_t chunk_samples, uint64_t chunk_default,
                   uint64_t chunk_max, Own own) {
    if (!h) return fail(BBB_EINVAL, "null handle");
    if (!out) return fail(BBB_EINVAL, "null out");
    int rc = own();
    if (rc) return rc;
    if (chunk_samples > chunk_max) return fail(BBB_EINVAL, "chunk_samples must be <= 2^" + std::to_string(__builtin_ctzll(chunk_max)));
    const int device = lutopt_device(h);
    if (device < 0) return fail(BBB_ENODEV, "host-only handle (device -1) cannot generate samples");
    if ((rc = use_device(device))) return rc;
    t->h = h;
    t->cfg = *cfg;
    t->chunk = chunk_samples ? chunk_samples : chunk_default;
    t->device = device;
    return BBB_OK;
}

// the generator's samples that a chunk of an object's samples stands for
struct TxRange { uint64_t first, n; };
inline TxRange tx_same_range(uint64_t first, uint64_t n) { return {first, n}; }

// what a chunk fills: the waveform into an int16 buffer, or (the sweeps) the noise alone, sample j's being the CLT value of
// state A^(warmup + j + 1) (tx.py:70-71), once for every setting
inline int tx_chunk_fill(const TxChunks &t, int16_t *buf, TxRange r) { return bbb_tx_fill_i16(t.h, &t.cfg, buf, r.n, r.first); }
inline int tx_chunk_fill(const TxChunks &t, int8_t *noise, TxRange r) {
    return t.cfg.noise_en ? bbb_awgn_fill_i8(t.h, noise, r.n, t.cfg.warmup + r.first) : BBB_OK;
}

// The chunk loop of every *_run over samples [first_sample, first_sample + nsamples): fill range(first, n) into buf, announce
// the next chunk's fill as TX.generate does (its noise start states are derived beside this chunk's kernels), then
// body(first, n, stream) with the handle's stream, read per chunk like the fill itself does.
template <class T, class Range, class Body>
int tx_chunks_walk(const TxChunks &t, T *buf, uint64_t first_sample, uint64_t nsamples, Range range, Body body) {
    if (nsamples == 0) return BBB_OK;
    BBB_HIP(hipSetDevice(t.device));
    for (uint64_t off = 0; off < nsamples;) {
        const uint64_t n = std::min(t.chunk, nsamples - off), first = first_sample + off;
        int rc = tx_chunk_fill(t, buf, range(first, n));
        if (rc) return rc;
        if (t.cfg.noise_en && off + n < nsamples) {
            const TxRange next = range(first + n, std::min(t.chunk, nsamples - off - n));
            if ((rc = bbb_awgn_prefetch(t.h, next.n, t.cfg.warmup + next.first))) return rc;
        }
        hipStream_t st = lutopt_stream(t.h);
        BBB_HIP(hipSetDevice(t.device));
        if ((rc = body(first, n, st))) return rc;
        off += n;
    }
    return BBB_OK;
}

// A chunk's data bits r (clamped at bit 0: bits below it read as 0, the reset shift register) into bits[words]: the source's
// PRBS-k from prbs_state, or the Pulser's.  *got: the bits written, lo .. lo + n - 1 (n 0: the chunk needs none).
struct TxBits { int64_t lo; uint64_t n; };
inline int tx_chunk_bits(const TxChunks &t, BitRange r, uint64_t *bits, uint64_t words, hipStream_t st, TxBits *got) {
    got->lo = std::max<int64_t>(0, r.lo);
    got->n = r.hi >= got->lo ? (uint64_t)(r.hi - got->lo + 1) : 0;
    if (got->n == 0) return BBB_OK;
    if (got->n > words * 64) return fail(BBB_EHIP, "internal: the chunk's data bits do not fit their buffer");
    if (t.cfg.source == 1) return xcorr_pulser_bits_launch(bits, (uint64_t)got->lo, (got->n + 63) / 64, st);
    return bbb_prbs_fill(t.cfg.prbs_k, t.cfg.prbs_state, (uint64_t)got->lo, got->n, bits, t.device, st);
}

// ---- the two sweeps: their settings ... ----------------------------------------------------------------------------------
constexpr int kTxMaxSettings = 512;

// the argument checks of a sweep's settings; *any_noise: some setting has its noise on
inline int tx_settings_check(const bbb_tx_cfg *base, const bbb_tx_setting *settings, int nset, bool *any_noise) {
    if (!base) return fail(BBB_EINVAL, "null base cfg");
    if (!settings) return fail(BBB_EINVAL, "null settings");
    if (nset < 1 || nset > kTxMaxSettings)
        return fail(BBB_EINVAL, "nset must be 1.." + std::to_string(kTxMaxSettings) + " (got " + std::to_string(nset) + ")");
    *any_noise = false;
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
        *any_noise = *any_noise || st.noise_en;
    }
    return BBB_OK;
}

// ... and their distinct shaped-value tables: a setting's coefficient set, or all zeros when its bits are off (tx.py:65-66)
struct ShapedTables {
    DevBuf<uint16_t> tables;         // 8 x 256 u16 per distinct set
    DevBuf<int16_t> coeffs;          // the distinct sets
    std::vector<int> of;             // setting -> its table
    int ntab = 0;

    // builds the tables on the device and waits for them: run may be called on another stream the handle is bound to later
    int build(const bbb_tx_setting *settings, int nset, hipStream_t st) {
        std::map<std::array<int16_t, 64>, int> table_of;
        std::vector<std::array<int16_t, 64>> sets;
        for (int i = 0; i < nset; i++) {
            std::array<int16_t, 64> c{};
            if (settings[i].bit_en) std::memcpy(c.data(), settings[i].coeffs, sizeof c);
            const auto it = table_of.emplace(c, (int)sets.size()).first;
            if (it->second == (int)sets.size()) sets.push_back(c);
            of.push_back(it->second);
        }
        ntab = (int)sets.size();
        int rc;
        if ((rc = coeffs.grow((size_t)ntab * 64)) || (rc = tables.grow((size_t)ntab * 8 * 256))) return rc;
        BBB_HIP(hipMemcpy(coeffs, sets.data(), (size_t)ntab * 64 * sizeof(int16_t), hipMemcpyHostToDevice));
        if ((rc = sweep_tables_launch(coeffs, ntab, tables, st))) return rc;
        BBB_HIP(hipStreamSynchronize(st));
        return BBB_OK;
    }
};

}  // namespace bbb
