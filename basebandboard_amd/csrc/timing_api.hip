// timing_api.hip -- the extern "C" entry points of the symbol timing recovery (include/bbb.h, bbb_timing_*).  Host logic only:
// the checks of bbb_timing_cfg, the plan, the launch structure, the call's scratch and the serial host model.
#include "capture.hpp"
#include "timing_launch.hpp"

#include <algorithm>
#include <string>
#include <vector>

using namespace bbb;

namespace {

struct Resolved {
    uint32_t P, L, h, chunk;
};

// everything wrong with cfg that needs no device; soft: shift and out_bytes count
int cfg_check(const bbb_timing_cfg *c, bool soft, Resolved *r) {
    if (!c) return fail(BBB_EINVAL, "null timing cfg");
    int rc = fir_cfg_check(&c->ff, !soft);
    if (rc) return rc;
    if (c->ff.decim != 1 || c->ff.phase != 0) return fail(BBB_EINVAL, "ff.decim must be 1 and ff.phase 0: the tracker chooses the instants");
    if (c->spb < 3 || c->spb > 256) return fail(BBB_EINVAL, "spb must be 3..256 (got " + std::to_string(c->spb) + ")");
    r->P = c->spb;
    r->L = c->block_symbols ? c->block_symbols : kTimingBlockDefault;
    if (r->L < 8 || r->L > 1024 || (uint64_t)r->L * r->P > 65536)
        return fail(BBB_EINVAL, "block_symbols must be 8..1024 with block_symbols * spb <= 65536 (got " + std::to_string(r->L) + ")");
    r->h = c->hysteresis_shift ? c->hysteresis_shift : kTimingShiftDefault;
    if (r->h > 63) return fail(BBB_EINVAL, "hysteresis_shift must be 1..63 (got " + std::to_string(r->h) + ")");
    if (c->init_phase != BBB_TIMING_ACQUIRE && c->init_phase >= r->P)
        return fail(BBB_EINVAL, "init_phase must be < spb or BBB_TIMING_ACQUIRE (got " + std::to_string(c->init_phase) + ")");
    r->chunk = std::min(c->chunk_blocks ? c->chunk_blocks : kTimingChunkDefault, kTimingChunkMax);
    return BBB_OK;
}

// the filtered sample a(n), n in [-1, nin), of host memory
int64_t host_acc(const int16_t *in, uint32_t nbefore, const bbb_fir_cfg &ff, int64_t n) {
    int64_t v = 0;
    for (uint32_t i = 0; i < ff.ntaps && n - (int64_t)i >= -(int64_t)nbefore; ++i) v += (int64_t)ff.taps[i] * in[n - (int64_t)i];
    return v;
}

}  // namespace

extern "C" {

int bbb_timing_plan(const bbb_timing_cfg *cfg, uint64_t nin, int final, uint64_t *nblocks, uint64_t *nconsumed, uint64_t *max_bits,
                    uint64_t *nbefore_wanted) {
    Resolved r;
    int rc = cfg_check(cfg, false, &r);
    if (rc) return rc;
    if (nin > kFirSampleLimit) return fail(BBB_EINVAL, "nin must be <= 2^58");
    uint64_t nb, nc, mb;
    timing_plan(r.P, r.L, nin, final != 0, nb, nc, mb);
    if (nblocks) *nblocks = nb;
    if (nconsumed) *nconsumed = nc;
    if (max_bits) *max_bits = mb;
    if (nbefore_wanted) *nbefore_wanted = cfg->ff.ntaps;
    return BBB_OK;
}

int bbb_timing_model_host(const int16_t *in, uint64_t nin, uint32_t nbefore, int final, const bbb_timing_cfg *cfg, uint64_t *state,
                          uint64_t *bits_packed, void *soft, uint8_t *phase, uint64_t *stats, uint64_t *nbits_out) {
    Resolved r;
    int rc = cfg_check(cfg, soft != nullptr, &r);
    if (rc) return rc;
    if (nin && !in) return fail(BBB_EINVAL, "null in");
    if (!state) return fail(BBB_EINVAL, "null state");
    const bbb_fir_cfg &ff = cfg->ff;
    uint64_t nblocks, nconsumed, max_bits;
    timing_plan(r.P, r.L, nin, final != 0, nblocks, nconsumed, max_bits);
    if (nblocks && !bits_packed) return fail(BBB_EINVAL, "null bits_packed");
    nin = nconsumed;
    const uint64_t LP = (uint64_t)r.L * r.P;
    for (uint64_t w = 0; w < (max_bits + 63) / 64; ++w) bits_packed[w] = 0;
    bool locked = (state[0] >> 63) != 0;
    uint64_t phi = (state[0] & 0xFFFFFFFFull) % r.P, nbits = 0, moves = 0, ups = 0, downs = 0;
    std::vector<int64_t> E(r.P);
    for (uint64_t j = 0; j < nblocks; ++j) {
        for (uint32_t p = 0; p < r.P; ++p) {
            E[p] = 0;
            for (uint32_t i = 0; i < r.L; ++i) {
                const uint64_t t = j * LP + (uint64_t)i * r.P + p;
                if (t >= nin) break;
                const int64_t d = host_acc(in, nbefore, ff, (int64_t)t) - cfg->threshold;
                E[p] += d < 0 ? -d : d;
            }
        }
        int m = 0, w = 0;
        if (!locked) {
            phi = 0;
            if (cfg->init_phase < r.P) phi = cfg->init_phase;
            else
                for (uint32_t p = 1; p < r.P; ++p)
                    if (E[p] > E[phi]) phi = p;
            locked = true;
        } else {
            const int64_t cur = E[phi], up = E[(phi + 1) % r.P], dn = E[(phi + r.P - 1) % r.P], margin = cur >> r.h;
            if (up > cur + margin && up >= dn) m = 1;
            else if (dn > cur + margin) m = -1;
            phi = (phi + r.P + m) % r.P;
            if (m == 1 && phi == 0) w = 1;
            if (m == -1 && phi == r.P - 1) w = -1;
        }
        if (phase) phase[j] = (uint8_t)phi;
        moves += m != 0;
        ups += w > 0;
        downs += w < 0;
        for (int64_t i = w; i < (int64_t)r.L; ++i) {
            const int64_t t = (int64_t)(j * LP + phi) + i * (int64_t)r.P;
            if (t >= (int64_t)nin) break;
            const int64_t v = host_acc(in, nbefore, ff, t);
            const bool bit = cfg->strict ? v > cfg->threshold : v >= cfg->threshold;
            bits_packed[nbits >> 6] |= (uint64_t)bit << (nbits & 63);
            if (soft) {
                if (ff.out_bytes == 2) ((int16_t *)soft)[nbits] = (int16_t)std::min<int64_t>(std::max<int64_t>(v >> ff.shift, -32768), 32767);
                else ((int32_t *)soft)[nbits] = (int32_t)v;
            }
            ++nbits;
        }
    }
    if (nblocks) state[0] = kTimingLocked | phi;
    state[1] += nbits;
    if (stats) {
        stats[0] += nblocks;
        stats[1] += moves;
        stats[2] += ups;
        stats[3] += downs;
    }
    if (nbits_out) *nbits_out = nbits;
    return BBB_OK;
}

int bbb_timing_run(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, int final, const bbb_timing_cfg *cfg, uint64_t *state_dev,
                   uint64_t *bits_packed_dev, void *soft_dev, uint8_t *phase_dev, uint64_t *stats_dev, uint64_t *nbits_dev, int device,
                   void *hip_stream) {
    Resolved r;
    int rc = cfg_check(cfg, soft_dev != nullptr, &r);
    if (rc) return rc;
    if (nin > kFirSampleLimit) return fail(BBB_EINVAL, "nin must be <= 2^58");
    if (nin && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    if (!state_dev) return fail(BBB_EINVAL, "null state_dev");
    if (!nbits_dev) return fail(BBB_EINVAL, "null nbits_dev");
    const bbb_fir_cfg &ff = cfg->ff;
    uint64_t nblocks, nconsumed, max_bits;
    timing_plan(r.P, r.L, nin, final != 0, nblocks, nconsumed, max_bits);
    if (nblocks && !bits_packed_dev) return fail(BBB_EINVAL, "null bits_packed_dev");
    const unsigned soft_bytes = ff.out_bytes == 4 ? 4 : 2;
    if (((uintptr_t)in_dev & 1) || ((uintptr_t)bits_packed_dev & 7) || ((uintptr_t)soft_dev & (soft_bytes - 1)) ||
        ((uintptr_t)state_dev & 7) || ((uintptr_t)stats_dev & 7) || ((uintptr_t)nbits_dev & 7))
        return fail(BBB_EINVAL, "misaligned device pointer");
    // the samples read: nconsumed of them behind up to ntaps samples of history (one more than the filter's: the early instant)
    const uint32_t before = std::min<uint32_t>(nbefore, ff.ntaps);
    struct Out {
        const void *p;
        uint64_t bytes;
        const char *name;
    } outs[6] = {{bits_packed_dev, (max_bits + 63) / 64 * 8, "bits_packed_dev"}, {soft_dev, soft_dev ? max_bits * soft_bytes : 0, "soft_dev"},
                 {phase_dev, phase_dev ? nblocks : 0, "phase_dev"},           {stats_dev, stats_dev ? 32u : 0u, "stats_dev"},
                 {nbits_dev, 8, "nbits_dev"},                                 {state_dev, 16, "state_dev"}};
    for (int i = 0; i < 6; ++i) {
        if (nconsumed && overlap(in_dev - before, (nconsumed + before) * 2, outs[i].p, outs[i].bytes))
            return fail(BBB_EINVAL, std::string(outs[i].name) + " overlaps the samples");
        for (int k = 0; k < i; ++k)
            if (overlap(outs[k].p, outs[k].bytes, outs[i].p, outs[i].bytes))
                return fail(BBB_EINVAL, std::string(outs[i].name) + " overlaps " + outs[k].name);
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    TimingLaunch a{};
    a.g.P = r.P;
    a.g.L = r.L;
    a.g.h = r.h;
    a.g.chunk = r.chunk;
    a.g.LP = r.L * r.P;
    a.g.nin = nconsumed;
    a.g.nblocks = nblocks;
    a.g.nchunks = (nblocks + r.chunk - 1) / r.chunk;
    const TimingScratch lay = timing_scratch(nblocks, a.g.nchunks, r.P);
    CallScratch<uint64_t> scratch;
    if ((rc = scratch.alloc(lay.words, st))) return rc;
    a.in = in_dev;
    a.nbefore = before;
    a.ngroups = fir_pack_taps(&ff, a.taps);
    a.shift = soft_dev ? ff.shift : 0;
    a.in_vec = !((uintptr_t)in_dev & 15);
    a.split = timing_split(r.P, a.g.LP);
    a.threshold = cfg->threshold;
    a.strict = cfg->strict != 0;
    a.init_phase = cfg->init_phase;
    a.state = state_dev;
    a.bits = bits_packed_dev;
    a.soft = soft_dev;
    a.soft_bytes = soft_bytes;
    a.phase = phase_dev;
    a.stats = stats_dev;
    a.nbits = nbits_dev;
    uint64_t *base = scratch;
    a.hdr = base + lay.hdr;
    a.boff = base + lay.boff;
    a.coff = base + lay.coff;
    a.cbits = reinterpret_cast<uint32_t *>(base + lay.cbits);
    a.binfo = reinterpret_cast<uint16_t *>(base + lay.binfo);
    a.mv = reinterpret_cast<uint8_t *>(base + lay.mv);
    a.cmap = reinterpret_cast<uint8_t *>(base + lay.cmap);
    a.cstart = reinterpret_cast<uint8_t *>(base + lay.cstart);
    // the words that two waves or tiles share are ORed together; the bits from nbits on stay 0
    if (max_bits) BBB_HIP(hipMemsetAsync(bits_packed_dev, 0, (max_bits + 63) / 64 * 8, st));
    return timing_launch(a, cus, st);
}

}  // extern "C"
