// carrier_api.hip -- the extern "C" entry points of the carrier recovery (include/bbb.h, bbb_carrier_*).  Host logic only: the
// checks of bbb_carrier_cfg, the plan, the launch structure, the call's scratch and the serial host model.
#include "capture.hpp"
#include "carrier_launch.hpp"

#include <algorithm>
#include <string>

using namespace bbb;

namespace {

struct Resolved {
    uint32_t L, chunk;
};

// everything wrong with cfg that needs no device
int cfg_check(const bbb_carrier_cfg *c, Resolved *r) {
    if (!c) return fail(BBB_EINVAL, "null carrier cfg");
    r->L = c->block_pairs ? c->block_pairs : kCarrierBlockDefault;
    if (r->L < 8 || r->L > 1024 || r->L % 8)
        return fail(BBB_EINVAL, "block_pairs must be a multiple of 8 in 8..1024 (got " + std::to_string(r->L) + ")");
    if (c->init_phase > 65535) return fail(BBB_EINVAL, "init_phase must be < 65536 (got " + std::to_string(c->init_phase) + ")");
    r->chunk = std::min(c->chunk_blocks ? c->chunk_blocks : kCarrierChunkDefault, kCarrierChunkMax);
    return BBB_OK;
}

}  // namespace

extern "C" {

int bbb_carrier_plan(const bbb_carrier_cfg *cfg, uint64_t nin, int final, uint64_t *nblocks, uint64_t *nconsumed) {
    Resolved r;
    int rc = cfg_check(cfg, &r);
    if (rc) return rc;
    if (nin > kCarrierPairLimit) return fail(BBB_EINVAL, "nin must be <= 2^58");
    uint64_t nb, nc;
    carrier_plan(r.L, nin, final != 0, nb, nc);
    if (nblocks) *nblocks = nb;
    if (nconsumed) *nconsumed = nc;
    return BBB_OK;
}

int bbb_carrier_model_host(const int16_t *in, uint64_t nin, int final, const bbb_carrier_cfg *cfg, uint64_t *state, int16_t *iq,
                           uint64_t *bits_packed, int16_t *soft, uint16_t *phase, uint64_t *stats) {
    Resolved r;
    int rc = cfg_check(cfg, &r);
    if (rc) return rc;
    if (nin > kCarrierPairLimit) return fail(BBB_EINVAL, "nin must be <= 2^58");
    if (nin && !in) return fail(BBB_EINVAL, "null in");
    if (!state) return fail(BBB_EINVAL, "null state");
    if (!iq && !bits_packed && !soft && !phase) return fail(BBB_EINVAL, "no output given");
    int16_t rom[1024];
    bbb_nco_rom(rom);
    const uint64_t L = r.L;
    const uint64_t nblocks = final ? (nin + L - 1) / L : nin / L;
    nin = std::min(nin, nblocks * L);
    if (bits_packed)
        for (uint64_t w = 0; w < (nblocks * L + 63) / 64; ++w) bits_packed[w] = 0;
    uint32_t est = (state[0] >> 63) ? (uint32_t)(state[0] & 0xFFFF) : cfg->init_phase;
    uint64_t flips = 0, zeros = 0;
    int64_t steps = 0;
    for (uint64_t j = 0; j < nblocks; ++j) {
        const uint64_t lo = j * L, hi = std::min(nin, lo + L);
        int64_t sr = 0, siq = 0;
        for (uint64_t n = lo; n < hi; ++n) {
            const int64_t i = in[2 * n], q = in[2 * n + 1];
            sr += i * i - q * q;
            siq += i * q;
        }
        const int64_t si = 2 * siq;
        const uint64_t m = (uint64_t)std::max(sr < 0 ? -sr : sr, si < 0 ? -si : si);
        int bl = 0;
        while (bl < 64 && (m >> bl)) ++bl;
        const int s = std::max(0, bl - 15);
        uint32_t mag;
        int theta2;
        ddc_polar((int)(sr >> s), (int)(si >> s), mag, theta2);
        const uint32_t h = ((uint32_t)theta2 & 0xFFFF) >> 1;
        const uint32_t d = (h - est) & 0xFFFF;
        const uint32_t next = (d < 16384 || d >= 49152) ? h : (h + 32768) & 0xFFFF;
        flips += (next >> 15) != (est >> 15);
        zeros += sr == 0 && si == 0;
        steps += (int16_t)(uint16_t)(next - est);
        est = next;
        if (phase) phase[j] = (uint16_t)est;
        const uint32_t adr = est >> 6;
        const int c = rom[(adr + 256) & 1023], sn = rom[adr];
        for (uint64_t n = lo; n < hi; ++n) {
            const int i = in[2 * n], q = in[2 * n + 1];
            const int io = std::min(std::max((i * c + q * sn) >> 15, -32768), 32767);
            const int qo = std::min(std::max((q * c - i * sn) >> 15, -32768), 32767);
            if (iq) {
                iq[2 * n] = (int16_t)io;
                iq[2 * n + 1] = (int16_t)qo;
            }
            if (soft) soft[n] = (int16_t)io;
            const bool bit = cfg->strict ? io > cfg->threshold : io >= cfg->threshold;
            if (bits_packed) bits_packed[n >> 6] |= (uint64_t)bit << (n & 63);
        }
    }
    if (nblocks) state[0] = kCarrierStarted | est;
    state[1] += nin;
    if (stats) {
        stats[0] += nblocks;
        stats[1] += flips;
        stats[2] += zeros;
        stats[3] += (uint64_t)steps;
    }
    return BBB_OK;
}

int bbb_carrier_run(const int16_t *in_dev, uint64_t nin, int final, const bbb_carrier_cfg *cfg, uint64_t *state_dev, int16_t *iq_dev,
                    uint64_t *bits_packed_dev, int16_t *soft_dev, uint16_t *phase_dev, uint64_t *stats_dev, int device, void *hip_stream) {
    Resolved r;
    int rc = cfg_check(cfg, &r);
    if (rc) return rc;
    if (nin > kCarrierPairLimit) return fail(BBB_EINVAL, "nin must be <= 2^58");
    if (nin && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    if (!state_dev) return fail(BBB_EINVAL, "null state_dev");
    if (!iq_dev && !bits_packed_dev && !soft_dev && !phase_dev) return fail(BBB_EINVAL, "no output given: iq_dev, bits_packed_dev, soft_dev and phase_dev are all null");
    if (((uintptr_t)in_dev & 3) || ((uintptr_t)iq_dev & 3) || ((uintptr_t)bits_packed_dev & 7) || ((uintptr_t)soft_dev & 1) ||
        ((uintptr_t)phase_dev & 1) || ((uintptr_t)state_dev & 7) || ((uintptr_t)stats_dev & 7))
        return fail(BBB_EINVAL, "misaligned device pointer");
    uint64_t nblocks, nconsumed;
    carrier_plan(r.L, nin, final != 0, nblocks, nconsumed);
    struct Out {
        const void *p;
        uint64_t bytes;
        const char *name;
    } outs[6] = {{iq_dev, iq_dev ? nconsumed * 4 : 0, "iq_dev"},
                 {bits_packed_dev, bits_packed_dev ? carrier_bit_words(nblocks, r.L) * 8 : 0, "bits_packed_dev"},
                 {soft_dev, soft_dev ? nconsumed * 2 : 0, "soft_dev"},
                 {phase_dev, phase_dev ? nblocks * 2 : 0, "phase_dev"},
                 {stats_dev, stats_dev ? 32u : 0u, "stats_dev"},
                 {state_dev, 16, "state_dev"}};
    for (int i = 0; i < 6; ++i) {
        if (overlap(in_dev, nconsumed * 4, outs[i].p, outs[i].bytes)) return fail(BBB_EINVAL, std::string(outs[i].name) + " overlaps the pairs");
        for (int k = 0; k < i; ++k)
            if (overlap(outs[k].p, outs[k].bytes, outs[i].p, outs[i].bytes))
                return fail(BBB_EINVAL, std::string(outs[i].name) + " overlaps " + outs[k].name);
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    CarrierLaunch a{};
    a.g.L = r.L;
    a.g.chunk = r.chunk;
    a.g.nin = nconsumed;
    a.g.nblocks = nblocks;
    a.g.nchunks = (nblocks + r.chunk - 1) / r.chunk;
    a.nflag = (uint32_t)std::min<uint64_t>(a.g.nchunks, (uint64_t)std::max(1, cus) * kCarrierGridPerCu);
    const CarrierScratch lay = carrier_scratch(nblocks, a.g.nchunks, a.nflag);
    CallScratch<uint64_t> scratch;
    if ((rc = scratch.alloc(lay.words, st))) return rc;
    a.in = in_dev;
    a.in_vec = !((uintptr_t)in_dev & 15);
    a.init_phase = cfg->init_phase;
    a.threshold = cfg->threshold;
    a.strict = cfg->strict != 0;
    a.state = state_dev;
    a.iq = iq_dev;
    a.bits = bits_packed_dev;
    a.soft = soft_dev;
    a.phase = phase_dev;
    a.stats = stats_dev;
    a.iq_vec = !((uintptr_t)iq_dev & 15);
    a.soft_vec = !((uintptr_t)soft_dev & 15);
    uint64_t *base = scratch;
    a.h = reinterpret_cast<uint16_t *>(base + lay.h);
    a.e = reinterpret_cast<uint16_t *>(base + lay.e);
    a.cpar = reinterpret_cast<uint8_t *>(base + lay.cpar);
    a.cstart = reinterpret_cast<uint8_t *>(base + lay.cstart);
    a.wsum = base + lay.wsum;
    CarrierRom rom;
    bbb_nco_rom(rom.v);
    return carrier_launch(a, rom, cus, st);
}

}  // extern "C"
