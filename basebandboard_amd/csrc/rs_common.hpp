// rs_common.hpp -- the per-lane core of the Reed-Solomon codec (include/bbb.h, bbb_rs_*), the field's tables and the code's
// generator, for the device and for the host: tests/rs_host.cpp restates the kernel's walk and calls these functions from it.
// bbb_rs_model_host and bbb_rs_encode_host are NOT built from this file: they are independent serial loops without tables.
//
// Symbol s of a codeword is the coefficient of x^p, p = n-1-s.  With beta = alpha^prim:
//   S_i = r(beta^(fcr+i)) = sum_s r_s beta^((fcr+i) p)                        i < nroots, in log form one add and wrap a step
//   errors e_k at p_k, X_k = beta^(p_k):  S_i = sum_k (e_k X_k^fcr) X_k^i, so Berlekamp-Massey over S gives
//   Lambda(x) = prod_k (1 - X_k x), Omega = S Lambda mod x^nroots, and at z = 1 / X_k
//   e_k = Omega(z) z^fcr / Lodd(z),  Lodd(z) = sum over odd i of Lambda_i z^i = z Lambda'(z)       (characteristic 2)
// A wave owns a codeword: lane l holds symbols 4l .. 4l+3 and, in Berlekamp-Massey, coefficient l of Lambda and of the
// auxiliary polynomial (kept multiplied by x^m: one move up a lane per step).  What crosses lanes -- the XOR reductions, the
// move, the ballots -- is the caller's; syndromes, Lambda and Omega lie in a few bytes that every lane of the wave can read.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#define RS_UNROLL _Pragma("unroll")
#else
#define RS_HD inline
#define RS_UNROLL
#endif

namespace bbb {

constexpr uint32_t kRsMaxRoots = 32, kRsMaxDepth = 8, kRsMaxN = 255;
constexpr uint32_t kRsNoLog = 255;                 // the "logarithm" of a zero coefficient
constexpr uint64_t kRsByteLimit = 1ull << 40;      // nframes * depth * n

// ex[i] = alpha^i for i < 512 (the sum of two logarithms needs no wrap), lg[ex[i]] = i for i < 255, lg[0] = 0 and unused
struct RsField {
    uint8_t ex[512];
    uint8_t lg[256];
};

// false: not 9 bits with bit 8 set, or x does not have order 255
RS_HD bool rs_field(uint32_t prim_poly, RsField &F) {
    if (prim_poly >> 9 || !(prim_poly >> 8)) return false;
    uint32_t x = 1;
    for (uint32_t i = 0; i < 512; ++i) F.ex[i] = 0;
    for (uint32_t i = 0; i < 256; ++i) F.lg[i] = 0;
    for (uint32_t i = 0; i < 255; ++i) {
        if (x == 0 || (i && x == 1)) return false;
        F.ex[i] = (uint8_t)x;
        F.lg[x] = (uint8_t)i;
        x <<= 1;
        if (x & 0x100) x ^= prim_poly;
    }
    if (x != 1) return false;
    for (uint32_t i = 255; i < 512; ++i) F.ex[i] = F.ex[i - 255];
    return true;
}

RS_HD uint32_t rs_mul(const uint8_t *ex, const uint8_t *lg, uint32_t a, uint32_t b) { return a && b ? ex[lg[a] + lg[b]] : 0u; }
RS_HD uint32_t rs_div(const uint8_t *ex, const uint8_t *lg, uint32_t a, uint32_t b) { return a ? ex[lg[a] + 255u - lg[b]] : 0u; }   // b != 0

// gq[j]: the logarithm of g's coefficient of x^(nroots-1-j), j < nroots (kRsNoLog: the coefficient is 0, as from nroots on):
// the order in which the dividing register meets them
struct RsCode {
    uint32_t nroots, n, k, depth, fcr, prim;
    uint8_t gq[kRsMaxRoots];
};

RS_HD uint32_t rs_gcd(uint32_t a, uint32_t b) {
    while (b) {
        const uint32_t r = a % b;
        a = b;
        b = r;
    }
    return a;
}

// the code of checked parameters: g(x) = prod_{i < nroots} (x - alpha^(prim (fcr + i)))
RS_HD void rs_code(const RsField &F, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n, uint32_t depth, RsCode &c) {
    c.nroots = nroots;
    c.n = n;
    c.k = n - nroots;
    c.depth = depth;
    c.fcr = fcr;
    c.prim = prim;
    uint8_t g[kRsMaxRoots + 1];                    // g[j]: the coefficient of x^j
    for (uint32_t j = 0; j <= kRsMaxRoots; ++j) g[j] = 0;
    g[0] = 1;
    for (uint32_t i = 0; i < nroots; ++i) {
        const uint32_t root = F.ex[prim * (fcr + i) % 255];
        for (uint32_t j = i + 1; j-- > 0;) g[j] = (uint8_t)((j ? g[j - 1] : 0u) ^ rs_mul(F.ex, F.lg, g[j], root));
        g[i + 1] = 1;                              // (written as its own term: g was of degree i and monic)
    }
    for (uint32_t j = 0; j < kRsMaxRoots; ++j) c.gq[j] = j < nroots && g[nroots - 1 - j] ? F.lg[g[nroots - 1 - j]] : (uint8_t)kRsNoLog;
}

// ---- the encoder: one codeword per lane --------------------------------------------------------------------------------------
// One step of the division by g: par[0] is the coefficient of x^(nroots-1) of the remainder so far, the first parity symbol;
// beyond nroots the register stays 0, so the walk is the same for every nroots.
RS_HD void rs_lfsr_step(const uint8_t *ex, const uint8_t *lg, const uint8_t *gq, uint8_t (&par)[kRsMaxRoots], uint32_t d) {
    const uint32_t fb = d ^ par[0], lf = lg[fb];
    RS_UNROLL
    for (uint32_t j = 0; j < kRsMaxRoots; ++j) {
        const uint32_t up = j + 1 < kRsMaxRoots ? par[j + 1] : 0u, q = gq[j];
        par[j] = (uint8_t)(up ^ (fb && q != kRsNoLog ? ex[lf + q] : 0u));
    }
}

// ---- the decoder: one codeword per wave --------------------------------------------------------------------------------------
// the place of a coded byte in its frame
RS_HD uint32_t rs_byte_of(const RsCode &c, uint32_t cw, uint32_t s) { return s * c.depth + cw; }

// What the lane's four symbols (symbol 4 lane + q in byte q of sym, 0 from n on) add to the syndromes, packed four to a word:
// S_i in byte i % 4 of out[i / 4].  The XOR of out over the wave's lanes is the syndromes.
RS_HD void rs_lane_syndromes(const uint8_t *ex, const uint8_t *lg, const RsCode &c, uint32_t sym, uint32_t lane, uint32_t (&out)[kRsMaxRoots / 4]) {
    RS_UNROLL
    for (uint32_t d = 0; d < kRsMaxRoots / 4; ++d) out[d] = 0;
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t v = sym >> (8 * q) & 255u, s = 4 * lane + q;
        if (!v || s >= c.n) continue;
        const uint32_t step = c.prim * (c.n - 1 - s) % 255u;
        uint32_t e = lg[v] + step * c.fcr % 255u;
        if (e >= 255u) e -= 255u;
        RS_UNROLL
        for (uint32_t d = 0; d < kRsMaxRoots / 4; ++d) {
            RS_UNROLL
            for (uint32_t b = 0; b < 4; ++b)
                if (4 * d + b < c.nroots) {
                    out[d] ^= (uint32_t)ex[e] << (8 * b);
                    e += step;
                    if (e >= 255u) e -= 255u;
                }
        }
    }
}

// Berlekamp-Massey, step r: what lane `lane` adds to the discrepancy (the XOR over the lanes is d) ...
RS_HD uint32_t rs_bm_term(const uint8_t *ex, const uint8_t *lg, uint32_t lam, const uint8_t *S, uint32_t r, uint32_t lane) {
    return lane <= r && lam ? rs_mul(ex, lg, lam, S[r - lane]) : 0u;
}
// ... and the lane's update: lam its coefficient of Lambda, bs that of x^m B (already moved up a lane for this step); b and the
// length L are the same in every lane
RS_HD void rs_bm_update(const uint8_t *ex, const uint8_t *lg, uint32_t d, uint32_t r, uint32_t &b, uint32_t &L, uint32_t &lam, uint32_t &bs) {
    if (!d) return;
    const uint32_t nl = lam ^ rs_mul(ex, lg, rs_div(ex, lg, d, b), bs);
    if (2 * L <= r) {
        bs = lam;
        b = d;
        L = r + 1 - L;
    }
    lam = nl;
}

// coefficient j of Omega = S Lambda mod x^nroots, from the L + 1 coefficients of Lambda
RS_HD uint32_t rs_omega(const uint8_t *ex, const uint8_t *lg, const uint8_t *lam, uint32_t L, const uint8_t *S, uint32_t j) {
    uint32_t o = 0;
    for (uint32_t i = 0; i <= L && i <= j; ++i) o ^= rs_mul(ex, lg, lam[i], S[j - i]);
    return o;
}

// the logarithm of z = 1 / X for symbol s < n
RS_HD uint32_t rs_zlog(const RsCode &c, uint32_t s) { return (255u - c.prim * (c.n - 1 - s) % 255u) % 255u; }

// Sum of coef[i] z^i over i = first, first + stride, ... < ncoef at the lane's FOUR positions at once, z = alpha^zl[q]: a
// coefficient and its logarithm are read once, and the four chains of look-ups do not wait for one another.
RS_HD void rs_eval4(const uint8_t *ex, const uint8_t *lg, const uint8_t *coef, uint32_t ncoef, const uint32_t (&zl)[4], uint32_t first,
                    uint32_t stride, uint32_t (&out)[4]) {
    uint32_t e[4], inc[4];
    RS_UNROLL
    for (uint32_t q = 0; q < 4; ++q) {
        inc[q] = stride * zl[q] % 255u;
        e[q] = first * zl[q] % 255u;
        out[q] = 0;
    }
    for (uint32_t i = first; i < ncoef; i += stride) {
        const uint32_t v = coef[i];
        if (v) {
            const uint32_t l = lg[v];
            RS_UNROLL
            for (uint32_t q = 0; q < 4; ++q) out[q] ^= ex[l + e[q]];
        }
        RS_UNROLL
        for (uint32_t q = 0; q < 4; ++q) {
            e[q] += inc[q];
            if (e[q] >= 255u) e[q] -= 255u;
        }
    }
}

// the error value at a root z = alpha^zl of Lambda from num = Omega(z) and den = the odd part of Lambda at z
RS_HD uint32_t rs_value(const uint8_t *ex, const uint8_t *lg, const RsCode &c, uint32_t num, uint32_t den, uint32_t zl) {
    return den ? rs_mul(ex, lg, rs_div(ex, lg, num, den), ex[c.fcr * zl % 255u]) : 0u;
}

}  // namespace bbb
