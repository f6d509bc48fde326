// rs_api.hip -- the extern "C" entry points of the Reed-Solomon codec (include/bbb.h, bbb_rs_*).  Host logic only: the checks
// of bbb_rs_cfg, the sizes of a call, the launch structure and the two serial host loops.
#include "capture.hpp"
#include "rs_launch.hpp"

#include <string>
#include <vector>

using namespace bbb;

namespace {

std::string got(uint32_t v) { return " (got " + std::to_string(v) + ")"; }

// everything wrong with cfg that needs no device; the field's tables and the code come out of it
int cfg_check(const bbb_rs_cfg *c, RsField *F, RsCode *code) {
    if (!c) return fail(BBB_EINVAL, "null rs cfg");
    if (c->prim_poly >> 9 || !(c->prim_poly >> 8)) return fail(BBB_EINVAL, "prim_poly must have 9 bits with bit 8 set" + got(c->prim_poly));
    if (!rs_field(c->prim_poly, *F)) return fail(BBB_EINVAL, "prim_poly is not primitive: x must have order 255" + got(c->prim_poly));
    if (c->fcr > 254) return fail(BBB_EINVAL, "fcr must be 0..254" + got(c->fcr));
    if (c->prim < 1 || c->prim > 254 || rs_gcd(c->prim, 255) != 1) return fail(BBB_EINVAL, "prim must be 1..254 with gcd(prim, 255) = 1" + got(c->prim));
    if (c->nroots < 2 || c->nroots > kRsMaxRoots || (c->nroots & 1)) return fail(BBB_EINVAL, "nroots must be even, 2..32" + got(c->nroots));
    if (c->n <= c->nroots || c->n > kRsMaxN) return fail(BBB_EINVAL, "n must be nroots + 1 .. 255" + got(c->n));
    if (c->depth < 1 || c->depth > kRsMaxDepth) return fail(BBB_EINVAL, "depth must be 1..8" + got(c->depth));
    if (c->reserved[0] || c->reserved[1]) return fail(BBB_EINVAL, "reserved must be 0");
    rs_code(*F, c->fcr, c->prim, c->nroots, c->n, c->depth, *code);
    return BBB_OK;
}

int size_check(const RsCode &code, uint64_t nframes) {
    if (nframes > kRsByteLimit / ((uint64_t)code.depth * code.n)) return fail(BBB_EINVAL, "nframes * depth * n must be <= 2^40");
    return BBB_OK;
}

// ---- the definition's own arithmetic: no tables, nothing of rs_common.hpp's core ------------------------------------------------
struct Gf {
    uint32_t poly;
    uint32_t mul(uint32_t a, uint32_t b) const {
        uint32_t r = 0;
        for (; b; b >>= 1) {
            if (b & 1) r ^= a;
            a <<= 1;
            if (a & 0x100) a ^= poly;
        }
        return r;
    }
    uint32_t pow(uint32_t a, uint32_t e) const {
        uint32_t r = 1;
        for (; e; e >>= 1) {
            if (e & 1) r = mul(r, a);
            a = mul(a, a);
        }
        return r;
    }
    uint32_t inv(uint32_t a) const { return pow(a, 254); }
};

// g[j]: the coefficient of x^j, g[nroots] = 1
std::vector<uint32_t> generator(const Gf &gf, const bbb_rs_cfg *c) {
    std::vector<uint32_t> g{1};
    for (uint32_t i = 0; i < c->nroots; ++i) {
        const uint32_t root = gf.pow(2, c->prim * (c->fcr + i));
        std::vector<uint32_t> h(g.size() + 1, 0);
        for (size_t j = 0; j < g.size(); ++j) {
            h[j + 1] ^= g[j];
            h[j] ^= gf.mul(g[j], root);
        }
        g = h;
    }
    return g;
}

// One received word r[0 .. n-1] (symbol 0 first) decoded in place by bounded distance: the number of symbols changed, or
// BBB_RS_FAILED with r untouched.  *bits: the popcount of the changes.
uint32_t decode_word(const Gf &gf, const bbb_rs_cfg *c, std::vector<uint32_t> &r, uint32_t *bits) {
    const uint32_t nroots = c->nroots, n = c->n, t = nroots / 2;
    const uint32_t beta = gf.pow(2, c->prim);
    *bits = 0;
    std::vector<uint32_t> S(nroots);
    bool clean = true;
    for (uint32_t i = 0; i < nroots; ++i) {
        const uint32_t x = gf.pow(beta, c->fcr + i);
        uint32_t v = 0;
        for (uint32_t s = 0; s < n; ++s) v = gf.mul(v, x) ^ r[s];               // Horner from x^(n-1) down
        S[i] = v;
        clean = clean && !v;
    }
    if (clean) return 0;
    // Berlekamp-Massey as in the books: C the connection polynomial, B the one before the last change of length
    std::vector<uint32_t> Cp(nroots + 2, 0), Bp(nroots + 2, 0);
    Cp[0] = Bp[0] = 1;
    uint32_t L = 0, m = 1, b = 1;
    for (uint32_t k = 0; k < nroots; ++k) {
        uint32_t d = S[k];
        for (uint32_t i = 1; i <= L; ++i) d ^= gf.mul(Cp[i], S[k - i]);
        if (!d) {
            ++m;
            continue;
        }
        const std::vector<uint32_t> T = Cp;
        const uint32_t f = gf.mul(d, gf.inv(b));
        for (uint32_t i = 0; i + m < Cp.size(); ++i) Cp[i + m] ^= gf.mul(f, Bp[i]);
        if (2 * L <= k) {
            L = k + 1 - L;
            Bp = T;
            b = d;
            m = 1;
        } else {
            ++m;
        }
    }
    if (L > t) return BBB_RS_FAILED;
    // the roots among the stored positions, by trying every one
    std::vector<uint32_t> pos;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t z = gf.inv(gf.pow(beta, n - 1 - s));
        uint32_t v = 0;
        for (uint32_t i = L + 1; i-- > 0;) v = gf.mul(v, z) ^ Cp[i];
        if (!v) pos.push_back(s);
    }
    if (pos.size() != L) return BBB_RS_FAILED;
    // Forney: Omega = S C mod x^nroots; e = Omega(z) z^fcr / (z C'(z))
    std::vector<uint32_t> Om(nroots, 0);
    for (uint32_t j = 0; j < nroots; ++j)
        for (uint32_t i = 0; i <= L && i <= j; ++i) Om[j] ^= gf.mul(Cp[i], S[j - i]);
    for (uint32_t s : pos) {
        const uint32_t z = gf.inv(gf.pow(beta, n - 1 - s));
        uint32_t num = 0, den = 0;
        for (uint32_t j = nroots; j-- > 0;) num = gf.mul(num, z) ^ Om[j];
        for (uint32_t i = 1; i <= L; i += 2) den ^= gf.mul(Cp[i], gf.pow(z, i));
        const uint32_t e = gf.mul(gf.mul(num, gf.pow(z, c->fcr)), gf.inv(den));
        r[s] ^= e;
        *bits += (uint32_t)__builtin_popcount(e);
    }
    return L;
}

}  // namespace

extern "C" {

int bbb_rs_encode_host(const uint8_t *data, uint64_t nframes, const bbb_rs_cfg *cfg, uint8_t *out) {
    RsField F;
    RsCode code;
    int rc = cfg_check(cfg, &F, &code);
    if (rc || (rc = size_check(code, nframes))) return rc;
    if (nframes && !data) return fail(BBB_EINVAL, "null data");
    if (nframes && !out) return fail(BBB_EINVAL, "null out");
    const Gf gf{cfg->prim_poly};
    const std::vector<uint32_t> g = generator(gf, cfg);
    const uint32_t I = cfg->depth, n = cfg->n, nroots = cfg->nroots, k = n - nroots;
    std::vector<uint32_t> rem(nroots);
    for (uint64_t f = 0; f < nframes; ++f)
        for (uint32_t c = 0; c < I; ++c) {
            // the remainder of data(x) x^nroots by g(x), one data symbol at a time; rem[j] is the coefficient of x^j
            std::fill(rem.begin(), rem.end(), 0u);
            for (uint32_t s = 0; s < k; ++s) {
                const uint32_t d = data[f * I * k + (uint64_t)s * I + c];
                out[f * I * n + (uint64_t)s * I + c] = (uint8_t)d;
                const uint32_t fb = d ^ rem[nroots - 1];
                for (uint32_t j = nroots - 1; j > 0; --j) rem[j] = rem[j - 1] ^ gf.mul(fb, g[j]);
                rem[0] = gf.mul(fb, g[0]);
            }
            for (uint32_t j = 0; j < nroots; ++j) out[f * I * n + (uint64_t)(k + j) * I + c] = (uint8_t)rem[nroots - 1 - j];
        }
    return BBB_OK;
}

int bbb_rs_model_host(const uint8_t *in, uint64_t nframes, const bbb_rs_cfg *cfg, uint8_t *data, uint8_t *nerr, uint64_t *stats) {
    RsField F;
    RsCode code;
    int rc = cfg_check(cfg, &F, &code);
    if (rc || (rc = size_check(code, nframes))) return rc;
    if (nframes && !in) return fail(BBB_EINVAL, "null in");
    if (nframes && !data) return fail(BBB_EINVAL, "null data");
    const Gf gf{cfg->prim_poly};
    const uint32_t I = cfg->depth, n = cfg->n, k = n - cfg->nroots;
    std::vector<uint32_t> r(n);
    for (uint64_t f = 0; f < nframes; ++f)
        for (uint32_t c = 0; c < I; ++c) {
            for (uint32_t s = 0; s < n; ++s) r[s] = in[f * I * n + (uint64_t)s * I + c];
            uint32_t bits;
            const uint32_t ne = decode_word(gf, cfg, r, &bits);
            for (uint32_t s = 0; s < k; ++s) data[f * I * k + (uint64_t)s * I + c] = (uint8_t)r[s];
            if (nerr) nerr[f * I + c] = (uint8_t)ne;
            if (stats) {
                stats[0] += 1;
                stats[1] += ne == 0;
                stats[2] += ne == BBB_RS_FAILED;
                if (ne != BBB_RS_FAILED) {
                    stats[3] += ne;
                    stats[4] += bits;
                }
            }
        }
    return BBB_OK;
}

int bbb_rs_encode(const uint8_t *data_dev, uint64_t nframes, const bbb_rs_cfg *cfg, uint8_t *out_dev, int device, void *hip_stream) {
    RsLaunch a{};
    int rc = cfg_check(cfg, &a.field, &a.code);
    if (rc || (rc = size_check(a.code, nframes))) return rc;
    if (nframes && !data_dev) return fail(BBB_EINVAL, "null data_dev");
    if (nframes && !out_dev) return fail(BBB_EINVAL, "null out_dev");
    const uint64_t dbytes = nframes * a.code.depth * a.code.k, cbytes = nframes * a.code.depth * a.code.n;
    if (overlap(data_dev, dbytes, out_dev, cbytes)) return fail(BBB_EINVAL, "out_dev overlaps the data");
    if ((rc = use_device(device))) return rc;
    if (!nframes) return BBB_OK;                   // nothing is encoded: nothing is written
    a.in = data_dev;
    a.out = out_dev;
    a.nframes = nframes;
    return rs_encode_launch(a, (hipStream_t)hip_stream);
}

int bbb_rs_decode(const uint8_t *in_dev, uint64_t nframes, const bbb_rs_cfg *cfg, uint8_t *data_dev, uint8_t *nerr_dev, uint64_t *stats_dev,
                  int device, void *hip_stream) {
    RsLaunch a{};
    int rc = cfg_check(cfg, &a.field, &a.code);
    if (rc || (rc = size_check(a.code, nframes))) return rc;
    if (nframes && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    if (nframes && !data_dev) return fail(BBB_EINVAL, "null data_dev");
    if ((uintptr_t)stats_dev & 7) return fail(BBB_EINVAL, "misaligned stats_dev");
    const uint64_t dbytes = nframes * a.code.depth * a.code.k, cbytes = nframes * a.code.depth * a.code.n;
    const uint64_t ebytes = nerr_dev ? nframes * a.code.depth : 0, sbytes = stats_dev && nframes ? 8 * BBB_RS_NSTATS : 0;
    if (overlap(in_dev, cbytes, data_dev, dbytes)) return fail(BBB_EINVAL, "data_dev overlaps the input");
    if (overlap(in_dev, cbytes, nerr_dev, ebytes)) return fail(BBB_EINVAL, "nerr_dev overlaps the input");
    if (overlap(in_dev, cbytes, stats_dev, sbytes)) return fail(BBB_EINVAL, "stats_dev overlaps the input");
    if (overlap(data_dev, dbytes, nerr_dev, ebytes)) return fail(BBB_EINVAL, "nerr_dev overlaps data_dev");
    if (overlap(data_dev, dbytes, stats_dev, sbytes)) return fail(BBB_EINVAL, "stats_dev overlaps data_dev");
    if (overlap(nerr_dev, ebytes, stats_dev, sbytes)) return fail(BBB_EINVAL, "stats_dev overlaps nerr_dev");
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    if (!nframes) return BBB_OK;                   // nothing is decoded: nothing is written
    a.in = in_dev;
    a.out = data_dev;
    a.nerr = nerr_dev;
    a.stats = stats_dev;
    a.nframes = nframes;
    return rs_decode_launch(a, cus, (hipStream_t)hip_stream);
}

}  // extern "C"
