// ldpc_api.hip -- the extern "C" entry points of the LDPC codec (include/bbb.h, bbb_ldpc_*).  Host logic only: the checks of
// bbb_ldpc_cfg, the sizes of a call, the launch structure and the two serial host loops.
#include "capture.hpp"
#include "ldpc_launch.hpp"

#include <string>
#include <vector>

using namespace bbb;

namespace {

std::string got(int64_t v) { return " (got " + std::to_string(v) + ")"; }

// everything wrong with cfg that needs no device; the edge list and the settings come out of it
int cfg_check(const bbb_ldpc_cfg *c, LdpcCode *code) {
    if (!c) return fail(BBB_EINVAL, "null ldpc cfg");
    if (c->Z < 2 || c->Z > kLdpcMaxZ) return fail(BBB_EINVAL, "Z must be 2..512" + got(c->Z));
    if (c->J < 1 || c->J > kLdpcMaxJ) return fail(BBB_EINVAL, "J must be 1..32" + got(c->J));
    if (c->K <= c->J || c->K > kLdpcMaxK) return fail(BBB_EINVAL, "K must be J + 1 .. 64" + got(c->K));
    if (c->K * c->Z > kLdpcMaxN) return fail(BBB_EINVAL, "n = K Z must be <= 16384" + got(c->K * c->Z));
    if (c->J * c->Z > kLdpcMaxM) return fail(BBB_EINVAL, "m = J Z must be <= 8192" + got(c->J * c->Z));
    if (c->max_iter < 1 || c->max_iter > 64) return fail(BBB_EINVAL, "max_iter must be 1..64" + got(c->max_iter));
    if (c->norm > 16) return fail(BBB_EINVAL, "norm must be 1..16, or 0 for 12" + got(c->norm));
    if (c->hard_mag > 32767) return fail(BBB_EINVAL, "hard_mag must be 1..32767, or 0 for 32" + got(c->hard_mag));
    if (c->reserved[0] || c->reserved[1]) return fail(BBB_EINVAL, "reserved must be 0");
    std::vector<uint32_t> in_col(c->K, 0);
    for (uint32_t j = 0; j < c->J; ++j) {
        uint32_t d = 0;
        for (uint32_t k = 0; k < c->K; ++k) {
            const int32_t s = c->base[j * c->K + k];
            if (s < -1 || s >= (int32_t)c->Z) return fail(BBB_EINVAL, "base entries must lie in -1 .. Z-1" + got(s));
            d += s >= 0;
            in_col[k] += s >= 0;
        }
        if (d < 2 || d > kLdpcMaxDeg) return fail(BBB_EINVAL, "every block row must hold 2..32 entries >= 0 (row " + std::to_string(j) + ":" + got(d) + ")");
    }
    for (uint32_t k = 0; k < c->K; ++k)
        if (!in_col[k]) return fail(BBB_EINVAL, "every block column must hold an entry >= 0 (column " + std::to_string(k) + ")");
    if (!ldpc_code(c->Z, c->J, c->K, c->base, *code)) return fail(BBB_EINVAL, "bad base matrix");
    code->max_iter = c->max_iter;
    code->norm = c->norm ? c->norm : 12;
    code->hard_mag = c->hard_mag ? c->hard_mag : 32;
    return BBB_OK;
}

int triangular_check(const LdpcCode &code) {
    for (uint32_t j = 0; j < code.J; ++j)
        if (ldpc_diag(code, j) == kLdpcMaxDeg) return fail(BBB_EINVAL, "parity part not triangular (block row " + std::to_string(j) + ")");
    return BBB_OK;
}

int size_check(const LdpcCode &code, uint64_t ncodewords) {
    if (ncodewords > kLdpcValueLimit / code.n) return fail(BBB_EINVAL, "ncodewords * n must be <= 2^40");
    return BBB_OK;
}

int format_check(int format, const void *in, uint64_t in_first) {
    if (format != BBB_CONV_SOFT16 && format != BBB_CONV_HARD) return fail(BBB_EINVAL, "unknown format" + got(format));
    if (in_first > kLdpcFirstLimit) return fail(BBB_EINVAL, "in_first must be <= 2^62");
    if ((uintptr_t)in & (format == BBB_CONV_HARD ? 7u : 1u)) return fail(BBB_EINVAL, "misaligned input");
    return BBB_OK;
}

// the bytes of the received values that a call reads
void in_range(const void *in, uint64_t in_first, uint64_t nvals, int format, const void **lo, uint64_t *bytes) {
    if (format == BBB_CONV_HARD) {
        *lo = (const uint8_t *)in + 8 * (in_first / 64);
        *bytes = nvals ? 8 * ((in_first + nvals + 63) / 64 - in_first / 64) : 0;
    } else {
        *lo = (const uint8_t *)in + 2 * in_first;
        *bytes = 2 * nvals;
    }
}

inline uint32_t get_bit(const uint64_t *p, uint64_t b) { return (uint32_t)(p[b >> 6] >> (b & 63u) & 1u); }

inline int32_t clamp15(int32_t v) { return v > 32767 ? 32767 : (v < -32767 ? -32767 : v); }

}  // namespace

extern "C" {

int bbb_ldpc_encode_host(const uint64_t *bits, uint64_t ncodewords, const bbb_ldpc_cfg *cfg, uint64_t *out) {
    LdpcCode code;
    int rc = cfg_check(cfg, &code);
    if (rc || (rc = triangular_check(code)) || (rc = size_check(code, ncodewords))) return rc;
    if (ncodewords && !bits) return fail(BBB_EINVAL, "null bits");
    if (ncodewords && !out) return fail(BBB_EINVAL, "null out");
    const uint32_t Z = cfg->Z, J = cfg->J, K = cfg->K, n = K * Z, k = (K - J) * Z;
    for (uint64_t w = 0; w < (ncodewords * n + 63) / 64; ++w) out[w] = 0;
    std::vector<uint8_t> x(n);
    for (uint64_t w = 0; w < ncodewords; ++w) {
        for (uint32_t i = 0; i < k; ++i) x[i] = (uint8_t)get_bit(bits, w * k + i);
        for (uint32_t j = J; j-- > 0;) {
            const uint32_t sjj = (uint32_t)cfg->base[j * K + K - J + j];
            for (uint32_t r = 0; r < Z; ++r) {
                uint32_t t = 0;
                for (uint32_t c = 0; c < K; ++c) {
                    const int32_t s = cfg->base[j * K + c];
                    if (s >= 0 && c != K - J + j) t ^= x[c * Z + (r + (uint32_t)s) % Z];
                }
                x[(K - J + j) * Z + (r + sjj) % Z] = (uint8_t)t;
            }
        }
        for (uint32_t i = 0; i < n; ++i) out[(w * n + i) >> 6] |= (uint64_t)x[i] << ((w * n + i) & 63u);
    }
    return BBB_OK;
}

int bbb_ldpc_model_host(const void *in, uint64_t in_first, uint64_t ncodewords, int format, const bbb_ldpc_cfg *cfg, uint64_t *bits_packed,
                        uint8_t *iters, uint64_t *stats) {
    LdpcCode code;
    int rc = cfg_check(cfg, &code);
    if (rc || (rc = size_check(code, ncodewords)) || (rc = format_check(format, in, in_first))) return rc;
    if (ncodewords && !in) return fail(BBB_EINVAL, "null in");
    if (ncodewords && !bits_packed) return fail(BBB_EINVAL, "null bits_packed");
    const uint32_t Z = cfg->Z, J = cfg->J, K = cfg->K, n = K * Z, k = (K - J) * Z;
    const int32_t norm = cfg->norm ? (int32_t)cfg->norm : 12, mag = cfg->hard_mag ? (int32_t)cfg->hard_mag : 32;
    for (uint64_t w = 0; w < (ncodewords * k + 63) / 64; ++w) bits_packed[w] = 0;
    std::vector<int32_t> P(n), R((size_t)J * Z * K), Q(K);
    std::vector<uint8_t> first(n);
    // every check of the hard decisions satisfied?
    auto satisfied = [&]() {
        for (uint32_t j = 0; j < J; ++j)
            for (uint32_t r = 0; r < Z; ++r) {
                uint32_t x = 0;
                for (uint32_t c = 0; c < K; ++c) {
                    const int32_t s = cfg->base[j * K + c];
                    if (s >= 0) x ^= (uint32_t)(P[c * Z + (r + (uint32_t)s) % Z] > 0);
                }
                if (x) return false;
            }
        return true;
    };
    for (uint64_t w = 0; w < ncodewords; ++w) {
        for (uint32_t v = 0; v < n; ++v) {
            const uint64_t at = in_first + w * n + v;
            P[v] = format == BBB_CONV_HARD ? (get_bit((const uint64_t *)in, at) ? mag : -mag) : clamp15(((const int16_t *)in)[at]);
            first[v] = P[v] > 0;
        }
        std::fill(R.begin(), R.end(), 0);
        uint32_t it_out = 0;
        if (!satisfied()) {
            it_out = BBB_LDPC_FAILED;
            for (uint32_t it = 0; it < cfg->max_iter && it_out == BBB_LDPC_FAILED; ++it) {
                for (uint32_t j = 0; j < J; ++j)
                    for (uint32_t r = 0; r < Z; ++r) {
                        int32_t *Rc = &R[((size_t)j * Z + r) * K];          // R per edge, at the edge's block column
                        int32_t m1 = INT32_MAX, m2 = INT32_MAX, i1 = -1;
                        uint32_t S = 0;
                        for (uint32_t c = 0; c < K; ++c) {
                            const int32_t s = cfg->base[j * K + c];
                            if (s < 0) continue;
                            Q[c] = clamp15(P[c * Z + (r + (uint32_t)s) % Z] - Rc[c]);
                            S ^= (uint32_t)(Q[c] > 0);
                            const int32_t a = Q[c] < 0 ? -Q[c] : Q[c];
                            if (a < m1) {
                                m2 = m1;
                                m1 = a;
                                i1 = (int32_t)c;
                            } else if (a < m2) {
                                m2 = a;
                            }
                        }
                        for (uint32_t c = 0; c < K; ++c) {
                            const int32_t s = cfg->base[j * K + c];
                            if (s < 0) continue;
                            const int32_t a = (((int32_t)c == i1 ? m2 : m1) * norm) >> 4;
                            Rc[c] = (S ^ (uint32_t)(Q[c] > 0)) ? a : -a;
                            P[c * Z + (r + (uint32_t)s) % Z] = clamp15(Q[c] + Rc[c]);
                        }
                    }
                if (satisfied()) it_out = it + 1;
            }
        }
        uint32_t changed = 0;
        for (uint32_t v = 0; v < n; ++v) changed += first[v] != (uint8_t)(P[v] > 0);
        for (uint32_t i = 0; i < k; ++i) bits_packed[(w * k + i) >> 6] |= (uint64_t)(P[i] > 0) << ((w * k + i) & 63u);
        if (iters) iters[w] = (uint8_t)it_out;
        if (stats) {
            stats[0] += 1;
            stats[1] += it_out == 0;
            stats[2] += it_out == BBB_LDPC_FAILED;
            if (it_out != BBB_LDPC_FAILED) {
                stats[3] += it_out;
                stats[4] += changed;
            }
        }
    }
    return BBB_OK;
}

int bbb_ldpc_encode(const uint64_t *bits_dev, uint64_t ncodewords, const bbb_ldpc_cfg *cfg, uint64_t *out_dev, int device, void *hip_stream) {
    LdpcLaunch a{};
    int rc = cfg_check(cfg, &a.code);
    if (rc || (rc = triangular_check(a.code)) || (rc = size_check(a.code, ncodewords))) return rc;
    if (ncodewords && !bits_dev) return fail(BBB_EINVAL, "null bits_dev");
    if (ncodewords && !out_dev) return fail(BBB_EINVAL, "null out_dev");
    if ((uintptr_t)bits_dev & 7) return fail(BBB_EINVAL, "misaligned bits_dev");
    if ((uintptr_t)out_dev & 7) return fail(BBB_EINVAL, "misaligned out_dev");
    const uint64_t dbytes = 8 * ((ncodewords * a.code.k + 63) / 64), cbytes = 8 * ((ncodewords * a.code.n + 63) / 64);
    if (overlap(bits_dev, dbytes, out_dev, cbytes)) return fail(BBB_EINVAL, "out_dev overlaps the data");
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    if (!ncodewords) return BBB_OK;                // nothing is encoded: nothing is written
    a.in = bits_dev;
    a.out = out_dev;
    a.ncodewords = ncodewords;
    return ldpc_encode_launch(a, cus, (hipStream_t)hip_stream);
}

int bbb_ldpc_decode(const void *in_dev, uint64_t in_first, uint64_t ncodewords, int format, const bbb_ldpc_cfg *cfg, uint64_t *bits_packed_dev,
                    uint8_t *iters_dev, uint64_t *stats_dev, int device, void *hip_stream) {
    LdpcLaunch a{};
    int rc = cfg_check(cfg, &a.code);
    if (rc || (rc = size_check(a.code, ncodewords)) || (rc = format_check(format, in_dev, in_first))) return rc;
    if (ncodewords && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    if (ncodewords && !bits_packed_dev) return fail(BBB_EINVAL, "null bits_packed_dev");
    if ((uintptr_t)bits_packed_dev & 7) return fail(BBB_EINVAL, "misaligned bits_packed_dev");
    if ((uintptr_t)stats_dev & 7) return fail(BBB_EINVAL, "misaligned stats_dev");
    const void *in_lo;
    uint64_t cbytes;
    in_range(in_dev, in_first, ncodewords * a.code.n, format, &in_lo, &cbytes);
    const uint64_t dbytes = 8 * ((ncodewords * a.code.k + 63) / 64), ebytes = iters_dev ? ncodewords : 0;
    const uint64_t sbytes = stats_dev && ncodewords ? 8 * BBB_LDPC_NSTATS : 0;
    if (overlap(in_lo, cbytes, bits_packed_dev, dbytes)) return fail(BBB_EINVAL, "bits_packed_dev overlaps the input");
    if (overlap(in_lo, cbytes, iters_dev, ebytes)) return fail(BBB_EINVAL, "iters_dev overlaps the input");
    if (overlap(in_lo, cbytes, stats_dev, sbytes)) return fail(BBB_EINVAL, "stats_dev overlaps the input");
    if (overlap(bits_packed_dev, dbytes, iters_dev, ebytes)) return fail(BBB_EINVAL, "iters_dev overlaps bits_packed_dev");
    if (overlap(bits_packed_dev, dbytes, stats_dev, sbytes)) return fail(BBB_EINVAL, "stats_dev overlaps bits_packed_dev");
    if (overlap(iters_dev, ebytes, stats_dev, sbytes)) return fail(BBB_EINVAL, "stats_dev overlaps iters_dev");
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
    if (!ncodewords) return BBB_OK;                // nothing is decoded: nothing is written
    a.in = in_dev;
    a.in_first = in_first;
    a.out = bits_packed_dev;
    a.iters = iters_dev;
    a.stats = stats_dev;
    a.ncodewords = ncodewords;
    a.format = format;
    return ldpc_decode_launch(a, cus, (hipStream_t)hip_stream);
}

}  // extern "C"
