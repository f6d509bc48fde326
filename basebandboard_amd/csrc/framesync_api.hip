// framesync_api.hip -- the extern "C" entry points of the frame synchroniser (include/bbb.h, bbb_framesync_* and bbb_frame_*).
// Host logic only: the checks of bbb_framesync_cfg and of the arguments, the plan, the launch structure and the three serial
// host loops, which take the stream one bit at a time and use nothing of framesync_common.hpp's core.
#include "capture.hpp"
#include "framesync_launch.hpp"

#include <string>
#include <vector>

using namespace bbb;

namespace {

std::string got(uint64_t v) { return " (got " + std::to_string(v) + ")"; }

int cfg_check(const bbb_framesync_cfg *c, FsCfg *k, FsRand *R) {
    if (!c) return fail(BBB_EINVAL, "null framesync cfg");
    if (c->marker_bits < 8 || c->marker_bits > 64) return fail(BBB_EINVAL, "marker_bits must be 8..64" + got(c->marker_bits));
    if (c->marker_bits < 64 && c->marker >> c->marker_bits) return fail(BBB_EINVAL, "marker has bits above marker_bits");
    if (c->frame_bits < c->marker_bits + 8 || c->frame_bits > (1u << 20))
        return fail(BBB_EINVAL, "frame_bits must be marker_bits + 8 .. 2^20" + got(c->frame_bits));
    if (c->tol_lock > c->marker_bits / 4) return fail(BBB_EINVAL, "tol_lock must be <= marker_bits / 4" + got(c->tol_lock));
    if (c->tol_search > c->tol_lock) return fail(BBB_EINVAL, "tol_search must be <= tol_lock" + got(c->tol_search));
    if (c->verify > 7) return fail(BBB_EINVAL, "verify must be 0..7" + got(c->verify));
    if (c->flywheel > 7) return fail(BBB_EINVAL, "flywheel must be 0..7" + got(c->flywheel));
    if (c->both_polarities > 1) return fail(BBB_EINVAL, "both_polarities must be 0 or 1" + got(c->both_polarities));
    if (c->reserved[0] || c->reserved[1] || c->reserved[2]) return fail(BBB_EINVAL, "reserved must be 0");
    if (!fs_rand_table(c->rand_poly, c->rand_seed, *R))
        return fail(BBB_EINVAL, "rand_poly must be 0 or 9 bits with the x^8 and x^0 terms set, rand_seed 1..255" + got(c->rand_poly));
    k->marker = c->marker;
    k->M = c->marker_bits;
    k->mask = k->M == 64 ? ~0ull : (1ull << k->M) - 1;
    k->F = c->frame_bits;
    k->tol_search = c->tol_search;
    k->tol_lock = c->tol_lock;
    k->v = c->verify;
    k->w = c->flywheel;
    k->both = c->both_polarities;
    k->payload_bytes = (k->F - k->M) % 8 ? 0 : (k->F - k->M) / 8;
    return BBB_OK;
}

int range_check(uint64_t nbits, uint64_t first_bit) {
    if (nbits > kFsMaxBits) return fail(BBB_EINVAL, "nbits must be <= 2^35" + got(nbits));
    if (first_bit > kFsMaxPos || nbits > kFsMaxPos - first_bit) return fail(BBB_EINVAL, "first_bit + nbits must be <= 2^48");
    return BBB_OK;
}

int whole_bytes_check(const FsCfg &k) {
    if (!k.payload_bytes) return fail(BBB_EINVAL, "frame_bits - marker_bits must be a multiple of 8");
    return BBB_OK;
}

struct Buf {
    const char *name;
    const void *p;
    uint64_t bytes, align;
};

// null (where bytes are wanted) and misaligned pointers, and every pair that overlaps; the first buffer is the input
int bufs_check(const std::vector<Buf> &b) {
    for (const Buf &x : b) {
        if (x.bytes && !x.p) return fail(BBB_EINVAL, std::string("null ") + x.name);
        if ((uintptr_t)x.p & (x.align - 1)) return fail(BBB_EINVAL, std::string("misaligned ") + x.name);
    }
    for (size_t i = 0; i < b.size(); ++i)
        for (size_t j = i + 1; j < b.size(); ++j)
            if (overlap(b[i].p, b[i].bytes, b[j].p, b[j].bytes))
                return fail(BBB_EINVAL, std::string(b[j].name) + " overlaps " + (i ? b[i].name : "the input"));
    return BBB_OK;
}

uint64_t scratch_bytes(uint64_t nbits) { return 8 * (fs_flag_words(nbits) + fs_words(nbits)); }

int run_check(const uint64_t *in, uint64_t nbits, uint64_t first_bit, const bbb_framesync_cfg *cfg, const uint64_t *state, const uint64_t *pos,
              const uint16_t *meta, uint64_t max_frames, const void *scratch, bool device, FsCfg *k, FsRand *R) {
    int rc = cfg_check(cfg, k, R);
    if (rc || (rc = range_check(nbits, first_bit))) return rc;
    if (max_frames > kFsMaxBits) return fail(BBB_EINVAL, "max_frames must be <= 2^35" + got(max_frames));
    std::vector<Buf> b{{"in_packed", in, 8 * fs_words(nbits), 8}, {"state", state, 8 * BBB_FRAMESYNC_NSTATE, 8}, {"pos", pos, 8 * max_frames, 8},
                       {"meta", meta, 2 * max_frames, 2}};
    if (device) b.push_back({"scratch", scratch, scratch_bytes(nbits), 8});
    return bufs_check(b);
}

int extract_check(const uint64_t *in, uint64_t nbits, uint64_t first_bit, const uint64_t *pos, const uint16_t *meta, const uint64_t *state,
                  uint64_t max_frames, const bbb_framesync_cfg *cfg, const uint8_t *out, uint64_t out_align, FsCfg *k, FsRand *R) {
    int rc = cfg_check(cfg, k, R);
    if (rc || (rc = whole_bytes_check(*k)) || (rc = range_check(nbits, first_bit))) return rc;
    if (max_frames > kFsMaxOut / k->payload_bytes) return fail(BBB_EINVAL, "max_frames * payload bytes must be <= 2^40");
    return bufs_check({{"in_packed", in, 8 * fs_words(nbits), 8}, {"state", state, 8 * BBB_FRAMESYNC_NSTATE, 8}, {"pos", pos, 8 * max_frames, 8},
                       {"meta", meta, 2 * max_frames, 2}, {"out", out, max_frames * k->payload_bytes, out_align}});
}

int attach_check(const uint8_t *payload, uint64_t nframes, const bbb_framesync_cfg *cfg, const uint64_t *out, FsCfg *k, FsRand *R) {
    int rc = cfg_check(cfg, k, R);
    if (rc || (rc = whole_bytes_check(*k))) return rc;
    if (nframes > kFsMaxOut / k->F) return fail(BBB_EINVAL, "nframes * frame_bits must be <= 2^40");
    return bufs_check({{"payload", payload, nframes * k->payload_bytes, 1}, {"out_packed", out, 8 * fs_words(nframes * k->F), 8}});
}

// ---- the definition's own arithmetic: one bit at a time -----------------------------------------------------------------------
inline uint32_t bit_of(const uint64_t *w, uint64_t r) { return (uint32_t)(w[r / 64] >> (r % 64) & 1); }

// the randomiser's byte for payload byte j, by running the register from the seed (no table)
struct Lfsr {
    uint32_t poly, seed, s;
    void restart() { s = seed; }
    uint32_t byte() {
        uint32_t v = 0;
        for (int i = 0; i < 8; ++i) {
            v = v << 1 | (s & 1);
            uint32_t fb = 0;
            for (int b = 0; b < 8; ++b) fb ^= (s >> b & 1) & (poly >> b & 1);
            s = s >> 1 | fb << 7;
        }
        return poly ? v : 0;
    }
};

}  // namespace

extern "C" {

int bbb_framesync_plan(uint64_t nbits, const bbb_framesync_cfg *cfg, bbb_framesync_plan_out *out) {
    FsCfg k;
    FsRand R;
    int rc = cfg_check(cfg, &k, &R);
    if (rc || (rc = range_check(nbits, 0))) return rc;
    if (!out) return fail(BBB_EINVAL, "null out");
    out->scratch_bytes = scratch_bytes(nbits);
    out->holdback_bits = ((uint64_t)std::max(k.v, 1u) * k.F + k.M + 63) / 64 * 64;
    out->tile_bits = kFsTileBits;
    return BBB_OK;
}

int bbb_framesync_model_host(const uint64_t *in, uint64_t nbits, uint64_t first_bit, int final, const bbb_framesync_cfg *cfg, uint64_t *state,
                             uint64_t *pos, uint16_t *meta, uint64_t max_frames) {
    FsCfg k;
    FsRand R;
    int rc = run_check(in, nbits, first_bit, cfg, state, pos, meta, max_frames, nullptr, false, &k, &R);
    if (rc) return rc;
    if (state[1] < first_bit) {
        state[0] |= BBB_FRAMESYNC_ERROR;
        return BBB_OK;
    }
    const uint64_t N = first_bit + nbits, M = cfg->marker_bits, F = cfg->frame_bits;
    auto dist = [&](uint64_t p, uint32_t pol) -> uint32_t {
        if (p + M > N) return (uint32_t)M + 1;
        uint32_t d = 0;
        for (uint64_t i = 0; i < M; ++i) d += bit_of(in, p - first_bit + i) != ((uint32_t)(cfg->marker >> i & 1) ^ pol);
        return d;
    };
    uint64_t mode = state[0] & 0xFF, pol = state[0] >> 8 & 1, fresh = state[0] >> 9 & 1, misses = state[0] >> 16 & 0xFF;
    uint64_t flags = state[0] & (BBB_FRAMESYNC_ERROR | BBB_FRAMESYNC_OVERFLOW), P = state[1], emitted = 0;
    auto emit = [&](uint32_t d, bool fly) {
        if (emitted < max_frames) {
            pos[emitted] = P;
            meta[emitted] = (uint16_t)(d | pol << 8 | (uint64_t)fly << 9 | fresh << 10);
        } else {
            flags |= BBB_FRAMESYNC_OVERFLOW;
        }
        fresh = 0;
        ++emitted;
        ++state[2];
    };
    for (;;) {
        if (mode == 0) {
            bool stop = false;
            for (;; ++P) {
                if (P + M > N) {
                    stop = true;
                    break;
                }
                int pl = -1;
                for (uint32_t q = 0; q <= cfg->both_polarities && pl < 0; ++q)
                    if (dist(P, q) <= cfg->tol_search) pl = (int)q;
                if (pl < 0) continue;
                if (!final && P + cfg->verify * F + M > N) {
                    stop = true;
                    break;
                }
                bool ok = true;
                for (uint32_t j = 1; j <= cfg->verify && ok; ++j) ok = dist(P + j * F, (uint32_t)pl) <= cfg->tol_lock;
                if (!ok) {
                    ++state[6];
                    continue;
                }
                mode = 1;
                pol = (uint64_t)pl;
                misses = 0;
                fresh = 1;
                ++state[4];
                break;
            }
            if (stop) break;
        } else {
            if (P + F > N) break;
            const uint32_t d = dist(P, (uint32_t)pol);
            if (d <= cfg->tol_lock) {
                misses = 0;
                emit(d, false);
                state[7] += d;
            } else {
                ++misses;
                if (misses > cfg->flywheel) {
                    mode = 0;
                    misses = 0;
                    ++state[5];
                    continue;
                }
                emit(d, true);
                ++state[3];
            }
            P += F;
        }
    }
    state[0] = mode | pol << 8 | fresh << 9 | misses << 16 | flags | emitted << 32;
    state[1] = P;
    return BBB_OK;
}

int bbb_frame_extract_host(const uint64_t *in, uint64_t nbits, uint64_t first_bit, const uint64_t *pos, const uint16_t *meta, const uint64_t *state,
                           uint64_t max_frames, const bbb_framesync_cfg *cfg, uint8_t *out) {
    FsCfg k;
    FsRand R;
    int rc = extract_check(in, nbits, first_bit, pos, meta, state, max_frames, cfg, out, 1, &k, &R);
    if (rc) return rc;
    const uint64_t count = std::min<uint64_t>(state[0] >> 32, max_frames), PB = k.payload_bytes;
    Lfsr reg{cfg->rand_poly, cfg->rand_seed, 0};
    for (uint64_t f = 0; f < count; ++f) {
        const bool inside = pos[f] >= first_bit && pos[f] - first_bit + cfg->frame_bits <= nbits;
        reg.restart();
        for (uint64_t j = 0; j < PB; ++j) {
            uint32_t v = 0;
            for (uint32_t b = 0; b < 8 && inside; ++b)
                v |= (bit_of(in, pos[f] - first_bit + cfg->marker_bits + 8 * j + b) ^ (uint32_t)(meta[f] >> 8 & 1)) << b;
            const uint32_t rb = reg.byte();
            out[f * PB + j] = (uint8_t)(inside ? v ^ rb : 0);
        }
    }
    return BBB_OK;
}

int bbb_frame_attach_host(const uint8_t *payload, uint64_t nframes, const bbb_framesync_cfg *cfg, uint64_t *out) {
    FsCfg k;
    FsRand R;
    int rc = attach_check(payload, nframes, cfg, out, &k, &R);
    if (rc) return rc;
    const uint64_t F = cfg->frame_bits, M = cfg->marker_bits, PB = k.payload_bytes;
    for (uint64_t i = 0; i < fs_words(nframes * F); ++i) out[i] = 0;
    Lfsr reg{cfg->rand_poly, cfg->rand_seed, 0};
    for (uint64_t f = 0; f < nframes; ++f) {
        auto put = [&](uint64_t o, uint64_t b) { out[(f * F + o) / 64] |= b << ((f * F + o) % 64); };
        for (uint64_t i = 0; i < M; ++i) put(i, cfg->marker >> i & 1);
        reg.restart();
        for (uint64_t j = 0; j < PB; ++j) {
            const uint32_t v = payload[f * PB + j] ^ reg.byte();
            for (uint32_t b = 0; b < 8; ++b) put(M + 8 * j + b, v >> b & 1);
        }
    }
    return BBB_OK;
}

int bbb_framesync_run(const uint64_t *in_packed_dev, uint64_t nbits, uint64_t first_bit, int final, const bbb_framesync_cfg *cfg,
                      uint64_t *state_dev, uint64_t *pos_dev, uint16_t *meta_dev, uint64_t max_frames, void *scratch_dev, int device,
                      void *hip_stream) {
    FsLaunch a{};
    int rc = run_check(in_packed_dev, nbits, first_bit, cfg, state_dev, pos_dev, meta_dev, max_frames, scratch_dev, true, &a.c, &a.rnd);
    if (rc) return rc;
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    a.in = in_packed_dev;
    a.nbits = nbits;
    a.first_bit = first_bit;
    a.final = final != 0;
    a.state = state_dev;
    a.pos = pos_dev;
    a.meta = meta_dev;
    a.max_frames = max_frames;
    a.flags = (uint64_t *)scratch_dev;
    a.plane = a.flags + fs_flag_words(nbits);
    return fs_run_launch(a, cus, (hipStream_t)hip_stream);
}

int bbb_frame_extract(const uint64_t *in_packed_dev, uint64_t nbits, uint64_t first_bit, const uint64_t *pos_dev, const uint16_t *meta_dev,
                      const uint64_t *state_dev, uint64_t max_frames, const bbb_framesync_cfg *cfg, uint8_t *out_dev, int device,
                      void *hip_stream) {
    FsLaunch a{};
    int rc = extract_check(in_packed_dev, nbits, first_bit, pos_dev, meta_dev, state_dev, max_frames, cfg, out_dev, 8, &a.c, &a.rnd);
    if (rc) return rc;
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    if (!max_frames) return BBB_OK;                // nothing can be extracted: nothing is written
    a.in = in_packed_dev;
    a.nbits = nbits;
    a.first_bit = first_bit;
    a.state = const_cast<uint64_t *>(state_dev);
    a.pos = const_cast<uint64_t *>(pos_dev);
    a.meta = const_cast<uint16_t *>(meta_dev);
    a.max_frames = max_frames;
    a.out_bytes = out_dev;
    return fs_extract_launch(a, cus, (hipStream_t)hip_stream);
}

int bbb_frame_attach(const uint8_t *payload_dev, uint64_t nframes, const bbb_framesync_cfg *cfg, uint64_t *out_packed_dev, int device,
                     void *hip_stream) {
    FsLaunch a{};
    int rc = attach_check(payload_dev, nframes, cfg, out_packed_dev, &a.c, &a.rnd);
    if (rc) return rc;
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    if (!nframes) return BBB_OK;                   // nothing is attached: nothing is written
    a.payload = payload_dev;
    a.nframes = nframes;
    a.out_words = out_packed_dev;
    return fs_attach_launch(a, cus, (hipStream_t)hip_stream);
}

}  // extern "C"
