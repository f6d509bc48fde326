// ldpc_common.hpp -- the per-check core of the LDPC codec (include/bbb.h, bbb_ldpc_*), the code's edge list, and the group, LDS
// and bit-packing arithmetic, for the device and for the host: tests/ldpc_host.cpp restates the kernel's walk and calls these
// functions from it.  bbb_ldpc_model_host and bbb_ldpc_encode_host are NOT built from this file: they are independent serial
// loops that keep R per edge.
//
// A check of layer j, row r has the edges e < deg[j] of block row j by ascending column: variable col[j][e] Z + (r + shift[j][e])
// mod Z.  Its messages R_e are kept COMPRESSED: a1 = (m1 norm) >> 4 and a2 = (m2 norm) >> 4 (15 bits each) in one word, the
// bits S ^ b_e in a second word, and i1 in a byte: |R_e| = a2 for e = i1 and a1 otherwise, R_e > 0 where its bit is set.  That is
// 67 bits, so a record is 9 bytes and not 8: two words and a byte, in two arrays.
//
// The group rule: a workgroup of kLdpcThreads lanes takes G = max(1, min(kLdpcMaxGroup, kLdpcThreads / Z)) codewords at a time,
// so that G Z <= kLdpcThreads where Z allows it: the G Z checks of a layer (of all the group's codewords) are spread over the
// lanes, check q = lane + kLdpcThreads * round being row q % Z of codeword q / Z.  Z > kLdpcThreads takes two rounds.
// G n <= 16384 and G m <= 8192 follow from the bounds of the ABI for every Z, so the LDS of a group never exceeds that of the
// largest single codeword.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LDPC_HD __host__ __device__ __forceinline__
#define LDPC_UNROLL _Pragma("unroll")
#else
#define LDPC_HD inline
#define LDPC_UNROLL
#endif

namespace bbb {

constexpr uint32_t kLdpcMaxJ = 32, kLdpcMaxK = 64, kLdpcMaxDeg = 32, kLdpcMaxZ = 512, kLdpcMaxN = 16384, kLdpcMaxM = 8192;
constexpr uint32_t kLdpcThreads = 256, kLdpcMaxGroup = 16, kLdpcRounds = kLdpcMaxZ / kLdpcThreads;
constexpr uint64_t kLdpcValueLimit = 1ull << 40;   // ncodewords * n
constexpr uint64_t kLdpcFirstLimit = 1ull << 62;   // in_first
constexpr uint32_t kLdpcFailed = 255;
constexpr int32_t kLdpcRunning = -1;               // a codeword's entry of the iteration table while it is still decoded

// The code as the kernels want it: the edges of every block row, the sizes, the decoder's settings with the defaults filled in.
struct LdpcCode {
    uint32_t Z, J, K, n, m, k;
    uint32_t max_iter, norm, hard_mag;
    uint32_t group;                                // G
    uint8_t deg[kLdpcMaxJ];
    uint8_t col[kLdpcMaxJ][kLdpcMaxDeg];
    uint16_t shift[kLdpcMaxJ][kLdpcMaxDeg];
};

LDPC_HD uint32_t ldpc_group(uint32_t Z) {
    const uint32_t g = kLdpcThreads / Z;
    return g < 1 ? 1u : (g > kLdpcMaxGroup ? kLdpcMaxGroup : g);
}

// Fills `code` from a base matrix (row-major J x K, the sizes checked by the caller): false where a block row holds fewer than
// 2 or more than 32 entries, a block column none, or an entry lies outside -1 .. Z-1.
LDPC_HD bool ldpc_code(uint32_t Z, uint32_t J, uint32_t K, const int16_t *base, LdpcCode &code) {
    code.Z = Z;
    code.J = J;
    code.K = K;
    code.n = K * Z;
    code.m = J * Z;
    code.k = (K - J) * Z;
    code.group = ldpc_group(Z);
    uint64_t seen = 0;
    for (uint32_t j = 0; j < kLdpcMaxJ; ++j) {
        code.deg[j] = 0;
        for (uint32_t e = 0; e < kLdpcMaxDeg; ++e) {
            code.col[j][e] = 0;
            code.shift[j][e] = 0;
        }
    }
    for (uint32_t j = 0; j < J; ++j) {
        uint32_t d = 0;
        for (uint32_t c = 0; c < K; ++c) {
            const int32_t s = base[j * K + c];
            if (s < -1 || s >= (int32_t)Z) return false;
            if (s < 0) continue;
            if (d == kLdpcMaxDeg) return false;
            code.col[j][d] = (uint8_t)c;
            code.shift[j][d] = (uint16_t)s;
            ++d;
            seen |= 1ull << c;
        }
        if (d < 2) return false;
        code.deg[j] = (uint8_t)d;
    }
    return seen == (K == 64 ? ~0ull : (1ull << K) - 1);
}

// the edge of row j that is its diagonal parity block (column K - J + j), or kLdpcMaxDeg where the parity part is not block
// upper triangular at row j
LDPC_HD uint32_t ldpc_diag(const LdpcCode &c, uint32_t j) {
    uint32_t at = kLdpcMaxDeg;
    for (uint32_t e = 0; e < c.deg[j]; ++e) {
        const uint32_t col = c.col[j][e];
        if (col >= c.K - c.J && col < c.K - c.J + j) return kLdpcMaxDeg;
        if (col == c.K - c.J + j) at = e;
    }
    return at;
}

// ---- the LDS of a group: byte offsets from a 16-byte aligned base -----------------------------------------------------------------
// P: int16, 8 halfwords of slack in front (the stage starts at the same offset into 16 bytes as the memory does), G n values
// rec: two words per check, G m of them; i1: a byte per check; orig, fin: the flat bit arrays of the G n first and last hard
// decisions, in u64 words; tab: per codeword of the group the iteration table (int32) and the syndrome flag (int32)
struct LdpcLds {
    uint32_t P, rec, i1, orig, fin, tab, bytes;
};

LDPC_HD LdpcLds ldpc_lds(const LdpcCode &c) {
    LdpcLds l;
    const uint32_t vals = c.group * c.n, checks = c.group * c.m, words = (vals + 63) / 64;
    l.P = 0;
    l.rec = (2 * (8 + vals) + 15) & ~15u;
    l.i1 = l.rec + 8 * checks;
    l.orig = (l.i1 + checks + 15) & ~15u;
    l.fin = l.orig + 8 * words;
    l.tab = l.fin + 8 * words;
    l.bytes = l.tab + 8 * kLdpcMaxGroup;
    return l;
}

// ---- the per-check core ---------------------------------------------------------------------------------------------------------------
LDPC_HD int32_t ldpc_clamp(int32_t v) { return v > 32767 ? 32767 : (v < -32767 ? -32767 : v); }

LDPC_HD uint32_t ldpc_var(const LdpcCode &c, uint32_t j, uint32_t e, uint32_t r) {
    uint32_t x = r + c.shift[j][e];
    if (x >= c.Z) x -= c.Z;
    return c.col[j][e] * c.Z + x;
}

// the message a compressed record holds for edge e
LDPC_HD int32_t ldpc_message(uint32_t w0, uint32_t mask, uint32_t i1, uint32_t e) {
    const int32_t mag = (int32_t)(e == i1 ? w0 >> 16 : w0 & 0xFFFFu);
    return (mask >> e & 1u) ? mag : -mag;
}

// One check of layer j, row r, on the posteriors P of its codeword: gather, two-minimum scan, new record, update.  fresh: the
// record holds nothing yet (R = 0).  The Q_e stay in registers between the two loops: every index below is a constant once
// the loops are unrolled, and deg[j] is the same in every lane.
LDPC_HD void ldpc_check(const LdpcCode &c, uint32_t j, uint32_t r, bool fresh, int16_t *P, uint32_t &w0, uint32_t &mask, uint32_t &i1) {
    const uint32_t deg = c.deg[j];
    int32_t q[kLdpcMaxDeg];
    uint32_t m1 = 0xFFFFFFFFu, m2 = 0xFFFFFFFFu, idx = 0, bm = 0;
    LDPC_UNROLL
    for (uint32_t e = 0; e < kLdpcMaxDeg; ++e) {
        q[e] = 0;
        if (e < deg) {
            const int32_t R = fresh ? 0 : ldpc_message(w0, mask, i1, e);
            const int32_t Q = ldpc_clamp((int32_t)P[ldpc_var(c, j, e, r)] - R);
            q[e] = Q;
            bm |= (uint32_t)(Q > 0) << e;
            const uint32_t a = (uint32_t)(Q < 0 ? -Q : Q);
            if (a < m1) {
                m2 = m1;
                m1 = a;
                idx = e;
            } else if (a < m2) {
                m2 = a;
            }
        }
    }
    const uint32_t S = (uint32_t)__builtin_popcount(bm) & 1u;
    const uint32_t a1 = (m1 * c.norm) >> 4, a2 = (m2 * c.norm) >> 4;
    w0 = a1 | a2 << 16;
    mask = S ? ~bm : bm;
    i1 = idx;
    LDPC_UNROLL
    for (uint32_t e = 0; e < kLdpcMaxDeg; ++e)
        if (e < deg) P[ldpc_var(c, j, e, r)] = (int16_t)ldpc_clamp(q[e] + ldpc_message(w0, mask, i1, e));
}

// the parity of a check over the hard decisions: 1 where it is not satisfied
LDPC_HD uint32_t ldpc_parity(const LdpcCode &c, uint32_t j, uint32_t r, const int16_t *P) {
    const uint32_t deg = c.deg[j];
    uint32_t x = 0;
    for (uint32_t e = 0; e < deg; ++e) x ^= (uint32_t)(P[ldpc_var(c, j, e, r)] > 0);
    return x;
}

// ---- flat bit arrays -------------------------------------------------------------------------------------------------------------------
// bits pos .. pos + len - 1 of a (LSB first in u64 words), len 1..64; reads no word the bits do not lie in
LDPC_HD uint64_t ldpc_get_bits(const uint64_t *a, uint64_t pos, uint32_t len) {
    const uint64_t w = pos >> 6;
    const uint32_t o = (uint32_t)(pos & 63u);
    uint64_t v = a[w] >> o;
    if (o + len > 64) v |= a[w + 1] << (64 - o);
    return len < 64 ? v & ((1ull << len) - 1) : v;
}

// Word W of a contiguously packed output in which item w occupies the bits [w per, (w + 1) per): the part of it that lies in
// [b0, b1), the bits of the items item0 .. that a group owns.  flat holds bit i of item w at (w - item0) stride + i.
LDPC_HD uint64_t ldpc_out_word(const uint64_t *flat, uint64_t W, uint64_t b0, uint64_t b1, uint64_t item0, uint32_t per, uint32_t stride) {
    uint64_t b = 64 * W > b0 ? 64 * W : b0;
    const uint64_t hi = 64 * W + 64 < b1 ? 64 * W + 64 : b1;
    uint64_t v = 0;
    while (b < hi) {
        const uint64_t w = b / per;
        const uint32_t i = (uint32_t)(b - w * per);
        const uint32_t len = (uint32_t)(per - i < hi - b ? per - i : hi - b);
        v |= ldpc_get_bits(flat, (w - item0) * stride + i, len) << (b - 64 * W);
        b += len;
    }
    return v;
}

// whether word W lies wholly inside [b0, b1): it is stored as it is; a word shared with a neighbour is OR-ed into zeroed memory
LDPC_HD bool ldpc_word_inside(uint64_t W, uint64_t b0, uint64_t b1) { return 64 * W >= b0 && 64 * W + 64 <= b1; }

// the bits of x = orig ^ fin, word w of a group's flat arrays of `total` bits, that belong to codewords which converged after at
// least one iteration
LDPC_HD uint32_t ldpc_corrected(uint64_t x, uint32_t w, uint32_t n, uint32_t total, const int32_t *iters) {
    uint32_t b = 64 * w, cnt = 0;
    const uint32_t hi = b + 64 < total ? b + 64 : total;
    while (b < hi) {
        const uint32_t g = b / n, len = (g + 1) * n - b < hi - b ? (g + 1) * n - b : hi - b;
        const uint64_t part = (x >> (b - 64 * w)) & (len < 64 ? (1ull << len) - 1 : ~0ull);
        if (iters[g] > 0 && iters[g] != (int32_t)kLdpcFailed) cnt += (uint32_t)__builtin_popcountll(part);
        b += len;
    }
    return cnt;
}

}  // namespace bbb
