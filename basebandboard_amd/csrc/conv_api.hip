// conv_api.hip -- the extern "C" entry points of the convolutional codec (include/bbb.h, bbb_conv_*).  Host logic only: the
// checks of bbb_conv_cfg, the sizes of a call, the launch structures and the two serial host models.
#include "capture.hpp"
#include "conv_launch.hpp"

#include <algorithm>
#include <string>
#include <vector>

using namespace bbb;

namespace {

// everything wrong with cfg that needs no device
int cfg_check(const bbb_conv_cfg *c, MlseGeom *geom, ConvPunct *punct) {
    if (!c) return fail(BBB_EINVAL, "null conv cfg");
    if (c->K < kConvMinK || c->K > kConvMaxK) return fail(BBB_EINVAL, "K must be 3..7 (got " + std::to_string(c->K) + ")");
    if (c->n < 2 || c->n > kConvMaxN) return fail(BBB_EINVAL, "n must be 2..3 (got " + std::to_string(c->n) + ")");
    for (uint32_t i = 0; i < c->n; ++i)
        if (!c->gen[i] || c->gen[i] >> c->K)
            return fail(BBB_EINVAL, "gen[" + std::to_string(i) + "] must be nonzero and below 2^K (got " + std::to_string(c->gen[i]) + ")");
    if (c->period < 1 || c->period > kConvMaxPeriod) return fail(BBB_EINVAL, "period must be 1..16 (got " + std::to_string(c->period) + ")");
    if (!conv_punct(c->n, c->period, c->keep, *punct))
        return fail(BBB_EINVAL, "keep must lie below 2^period and every step of the period must keep a bit");
    if (!conv_geom(c->block_steps, c->warmup_steps, c->lookahead_steps, *geom))
        return fail(BBB_EINVAL, "warmup_steps and lookahead_steps must be <= 128 and block + warmup + lookahead <= 512 (got " +
                                    std::to_string(geom->B) + ", " + std::to_string(geom->W) + ", " + std::to_string(geom->D) + ")");
    return BBB_OK;
}

// the sizes of a decoder call, from sizes alone
int sizes(const MlseGeom &geom, const ConvPunct &P, uint64_t nin, uint64_t first, int final, uint64_t *nsteps, uint64_t *ndecided) {
    if (nin > kConvValueLimit) return fail(BBB_EINVAL, "nin must be <= 2^60");
    if (first > kConvStepLimit) return fail(BBB_EINVAL, "first_step + nsteps must be <= 2^58");
    *nsteps = conv_steps_below(P, conv_idx(P, first) + nin) - first;
    if (*nsteps > kConvStepLimit - first) return fail(BBB_EINVAL, "first_step + nsteps must be <= 2^58");
    *ndecided = mlse_ndecided(geom, first, *nsteps, final != 0);
    return BBB_OK;
}

uint64_t nbefore_wanted(const MlseGeom &geom, const ConvPunct &P, uint64_t first) {
    return conv_idx(P, first) - conv_idx(P, mlse_window(geom, first / geom.B, first, 0, 0).a_lo);
}

// the bytes of the buffer that hold the values [lo, hi) counted from its base
void value_bytes(const void *in, int format, uint64_t lo, uint64_t hi, const void **p, uint64_t *bytes) {
    if (format == BBB_CONV_HARD) {
        *p = static_cast<const unsigned char *>(in) + lo / 64 * 8;
        *bytes = hi > lo ? ((hi + 63) / 64 - lo / 64) * 8 : 0;
    } else {
        *p = static_cast<const unsigned char *>(in) + lo * 2;
        *bytes = (hi - lo) * 2;
    }
}

int encode_sizes(const bbb_conv_cfg *cfg, ConvPunct *P, uint64_t nsteps, uint64_t first, uint64_t *nout) {
    MlseGeom geom;
    int rc = cfg_check(cfg, &geom, P);
    if (rc) return rc;
    if (first > kConvStepLimit || nsteps > kConvStepLimit - first) return fail(BBB_EINVAL, "first_step + nsteps must be <= 2^58");
    *nout = conv_idx(*P, first + nsteps) - conv_idx(*P, first);
    return BBB_OK;
}

}  // namespace

extern "C" {

int bbb_conv_plan(const bbb_conv_cfg *cfg, uint64_t nin, uint64_t first_step, int final, uint64_t *nsteps, uint64_t *ndecided,
                  uint64_t *nbefore_wanted_out) {
    MlseGeom geom;
    ConvPunct P;
    int rc = cfg_check(cfg, &geom, &P);
    if (rc) return rc;
    uint64_t ns, nd;
    if ((rc = sizes(geom, P, nin, first_step, final, &ns, &nd))) return rc;
    if (nsteps) *nsteps = ns;
    if (ndecided) *ndecided = nd;
    if (nbefore_wanted_out) *nbefore_wanted_out = nbefore_wanted(geom, P, first_step);
    return BBB_OK;
}

// The encoder's definition, step by step, with nothing of conv_common.hpp's core in it.
int bbb_conv_encode_host(const uint64_t *bits, uint64_t nsteps, uint64_t first_step, const bbb_conv_cfg *cfg, uint32_t *state,
                         uint64_t *out, uint64_t *nout_out) {
    ConvPunct P;
    uint64_t nout;
    int rc = encode_sizes(cfg, &P, nsteps, first_step, &nout);
    if (rc) return rc;
    if (nsteps && !bits) return fail(BBB_EINVAL, "null bits");
    if (nout && !out) return fail(BBB_EINVAL, "null out");
    if (nout_out) *nout_out = nout;
    if (!nsteps) return BBB_OK;
    const uint32_t K = cfg->K, mask = (1u << (K - 1)) - 1;
    uint32_t h = (state ? *state : cfg->init_state) & mask;
    for (uint64_t w = 0; w < (nout + 63) / 64; ++w) out[w] = 0;
    uint64_t pos = 0;
    for (uint64_t k = 0; k < nsteps; ++k) {
        const uint32_t b = (uint32_t)(bits[k >> 6] >> (k & 63)) & 1u, r = (h << 1) | b;
        const uint32_t place = (uint32_t)((first_step + k) % cfg->period);
        for (uint32_t i = 0; i < cfg->n; ++i) {
            uint32_t c = 0;
            for (uint32_t j = 0; j < K; ++j)
                if (cfg->gen[i] >> (K - 1 - j) & 1) c ^= r >> j & 1;
            if (cfg->keep[i] >> place & 1) {
                out[pos >> 6] |= (uint64_t)c << (pos & 63);
                ++pos;
            }
        }
        h = r & mask;
    }
    if (state) *state = h;
    return BBB_OK;
}

int bbb_conv_encode(const uint64_t *bits_dev, uint64_t nsteps, uint64_t first_step, const bbb_conv_cfg *cfg, uint32_t *state_dev,
                    uint64_t *out_dev, uint64_t *nout_out, int device, void *hip_stream) {
    ConvEncodeLaunch a{};
    uint64_t nout;
    int rc = encode_sizes(cfg, &a.punct, nsteps, first_step, &nout);
    if (rc) return rc;
    if (nsteps && !bits_dev) return fail(BBB_EINVAL, "null bits_dev");
    if (nout && !out_dev) return fail(BBB_EINVAL, "null out_dev");
    if (((uintptr_t)bits_dev & 7) || ((uintptr_t)out_dev & 7) || ((uintptr_t)state_dev & 3)) return fail(BBB_EINVAL, "misaligned device pointer");
    const uint64_t ibytes = (nsteps + 63) / 64 * 8, obytes = (nout + 63) / 64 * 8, sbytes = state_dev && nsteps ? 4 : 0;
    if (overlap(bits_dev, ibytes, out_dev, obytes)) return fail(BBB_EINVAL, "out_dev overlaps the input bits");
    if (overlap(bits_dev, ibytes, state_dev, sbytes)) return fail(BBB_EINVAL, "state_dev overlaps the input bits");
    if (overlap(out_dev, obytes, state_dev, sbytes)) return fail(BBB_EINVAL, "state_dev overlaps out_dev");
    if (nout_out) *nout_out = nout;
    if ((rc = use_device(device))) return rc;
    if (!nsteps) return BBB_OK;                    // nothing is encoded: nothing is written
    a.bits = bits_dev;
    a.first = first_step;
    a.nsteps = nsteps;
    a.idx_first = conv_idx(a.punct, first_step);
    a.nout = nout;
    a.K = cfg->K;
    a.n = cfg->n;
    for (uint32_t i = 0; i < cfg->n; ++i) a.gen[i] = cfg->gen[i];
    a.init_state = cfg->init_state & ((1u << (cfg->K - 1)) - 1);
    a.state = state_dev;
    a.out = out_dev;
    return conv_encode_launch(a, (hipStream_t)hip_stream);
}

// The decoder's definition, step by step and window by window, with nothing of conv_common.hpp's core in it.
int bbb_conv_model_host(const void *in, uint64_t in_first, uint64_t nin, uint64_t nbefore, uint64_t first_step, int final, int format,
                        const bbb_conv_cfg *cfg, uint64_t *bits_packed, uint64_t *ndecided_out) {
    MlseGeom geom;
    ConvPunct P;
    int rc = cfg_check(cfg, &geom, &P);
    if (rc) return rc;
    if (format != BBB_CONV_SOFT16 && format != BBB_CONV_HARD) return fail(BBB_EINVAL, "format must be BBB_CONV_SOFT16 or BBB_CONV_HARD");
    uint64_t nsteps, nd;
    if ((rc = sizes(geom, P, nin, first_step, final, &nsteps, &nd))) return rc;
    if (nbefore > in_first) return fail(BBB_EINVAL, "nbefore must be <= in_first");
    if (nin && !in) return fail(BBB_EINVAL, "null in");
    if (nd && !bits_packed) return fail(BBB_EINVAL, "null bits_packed");
    if (ndecided_out) *ndecided_out = nd;
    const int K = (int)cfg->K, NS = 1 << (K - 1), n = (int)cfg->n;
    const int64_t B = geom.B, W = geom.W, D = geom.D, first = (int64_t)first_step, end = first + (int64_t)nsteps, p = cfg->period;
    // the transmitted bits in front of step t, counted
    auto idx = [&](int64_t t) {
        int64_t per = 0, part = 0;
        for (int64_t s = 0; s < p; ++s)
            for (int i = 0; i < n; ++i) {
                per += cfg->keep[i] >> s & 1;
                if (s < t % p) part += cfg->keep[i] >> s & 1;
            }
        return t / p * per + part;
    };
    const int64_t idx_first = idx(first);
    // received value number x of the record (x counted over the whole stream): 0 outside the history and the call
    auto value = [&](int64_t x) -> int64_t {
        const int64_t rel = x - idx_first;
        if (rel < -(int64_t)nbefore || rel >= (int64_t)nin) return 0;
        const uint64_t e = (uint64_t)((int64_t)in_first + rel);
        if (format == BBB_CONV_HARD) return (static_cast<const uint64_t *>(in)[e >> 6] >> (e & 63) & 1) ? 1 : -1;
        return static_cast<const int16_t *>(in)[e];
    };
    for (uint64_t w = 0; w < (nd + 63) / 64; ++w) bits_packed[w] = 0;
    if (!nd) return BBB_OK;
    std::vector<uint64_t> choice(kMlseMaxWindow);
    for (int64_t j = first / B; j * B < first + (int64_t)nd; ++j) {
        const int64_t lo = std::max<int64_t>(0, j * B - W), hi = std::min(end, (j + 1) * B + D);
        int64_t m[64], next[64];
        for (int h = 0; h < NS; ++h) m[h] = lo == 0 && h != (int)(cfg->init_state & (uint32_t)(NS - 1)) ? -(1ll << 30) : 0;
        int64_t x = idx(lo);
        for (int64_t T = lo; T < hi; ++T) {
            int64_t r[3] = {0, 0, 0};
            for (int i = 0; i < n; ++i)
                if (cfg->keep[i] >> (T % p) & 1) r[i] = value(x++);
            uint64_t ch = 0;
            for (int hp = 0; hp < NS; ++hp) {
                int64_t cand[2];
                for (int c = 0; c < 2; ++c) {
                    const int h = (hp >> 1) | (c << (K - 2)), reg = (h << 1) | (hp & 1);
                    int64_t gain = 0;
                    for (int i = 0; i < n; ++i) {
                        int par = 0;
                        for (int q = 0; q < K; ++q) par ^= (reg >> q & 1) & (int)(cfg->gen[i] >> (K - 1 - q) & 1);
                        gain += par ? r[i] : -r[i];
                    }
                    cand[c] = m[h] + gain;
                }
                const int c = cand[1] > cand[0];
                next[hp] = cand[c];
                ch |= (uint64_t)c << hp;
            }
            for (int h = 0; h < NS; ++h) m[h] = next[h];
            choice[(size_t)(T - lo)] = ch;
        }
        int s = 0;
        for (int h = 1; h < NS; ++h)
            if (m[h] > m[s]) s = h;
        if (cfg->terminated && final && hi == end) s = 0;
        for (int64_t T = hi - 1; T >= lo; --T) {
            if (T >= j * B && T < (j + 1) * B && T >= first && T < first + (int64_t)nd)
                bits_packed[(T - first) >> 6] |= (uint64_t)(s & 1) << ((T - first) & 63);
            s = (s >> 1) | ((int)(choice[(size_t)(T - lo)] >> s & 1) << (K - 2));
        }
    }
    return BBB_OK;
}

int bbb_conv_decode(const void *in_dev, uint64_t in_first, uint64_t nin, uint64_t nbefore, uint64_t first_step, int final, int format,
                    const bbb_conv_cfg *cfg, uint64_t *bits_packed_dev, uint64_t *stats_dev, uint64_t *ndecided_out, int device,
                    void *hip_stream) {
    ConvLaunch a{};
    int rc = cfg_check(cfg, &a.geom, &a.punct);
    if (rc) return rc;
    if (format != BBB_CONV_SOFT16 && format != BBB_CONV_HARD) return fail(BBB_EINVAL, "format must be BBB_CONV_SOFT16 or BBB_CONV_HARD");
    uint64_t nsteps, nd;
    if ((rc = sizes(a.geom, a.punct, nin, first_step, final, &nsteps, &nd))) return rc;
    if (nbefore > in_first) return fail(BBB_EINVAL, "nbefore must be <= in_first");
    if (in_first > (1ull << 62)) return fail(BBB_EINVAL, "in_first must be <= 2^62");
    if (nin && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    if (nd && !bits_packed_dev) return fail(BBB_EINVAL, "null bits_packed_dev");
    if (((uintptr_t)in_dev & (format == BBB_CONV_HARD ? 7 : 1)) || ((uintptr_t)bits_packed_dev & 7) || ((uintptr_t)stats_dev & 7))
        return fail(BBB_EINVAL, "misaligned device pointer");
    // the history the kernel reads: what the first window reaches, and no more than the caller says is there; the values it
    // reads behind in_first: those of the call's whole steps
    const uint64_t before = std::min<uint64_t>(nbefore, nbefore_wanted(a.geom, a.punct, first_step));
    const uint64_t nused = conv_idx(a.punct, first_step + nsteps) - conv_idx(a.punct, first_step);
    const void *rd;
    uint64_t rbytes;
    value_bytes(in_dev, format, in_first - before, in_first + nused, &rd, &rbytes);
    const uint64_t bbytes = (nd + 63) / 64 * 8;
    if (overlap(rd, rbytes, bits_packed_dev, bbytes)) return fail(BBB_EINVAL, "bits_packed_dev overlaps the received values");
    if (overlap(rd, rbytes, stats_dev, stats_dev ? 16 : 0)) return fail(BBB_EINVAL, "stats_dev overlaps the received values");
    if (overlap(bits_packed_dev, bbytes, stats_dev, stats_dev ? 16 : 0)) return fail(BBB_EINVAL, "stats_dev overlaps bits_packed_dev");
    if (ndecided_out) *ndecided_out = nd;
    const hipStream_t st = (hipStream_t)hip_stream;
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    if (!nd) return BBB_OK;                        // nothing is decided: nothing is written
    a.in = in_dev;
    a.hard = format == BBB_CONV_HARD;
    a.in_first = in_first;
    a.rel_lo = -(int64_t)before;
    a.rel_hi = (int64_t)nused;
    a.idx_first = conv_idx(a.punct, first_step);
    a.K = cfg->K;
    a.n = cfg->n;
    for (uint32_t i = 0; i < cfg->n; ++i) a.gen[i] = cfg->gen[i];
    a.init_state = cfg->init_state & ((1u << (cfg->K - 1)) - 1);
    a.forced_end = cfg->terminated && final;
    a.first = first_step;
    a.nsteps = nsteps;
    a.ndecided = nd;
    a.j0 = first_step / a.geom.B;
    a.nblocks = (first_step + nd - 1) / a.geom.B - a.j0 + 1;
    a.bits = bits_packed_dev;
    a.stats = stats_dev;
    // the words that two blocks share are ORed together
    BBB_HIP(hipMemsetAsync(bits_packed_dev, 0, bbytes, st));
    return conv_decode_launch(a, cus, st);
}

}  // extern "C"
