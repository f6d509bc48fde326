// framesync_common.hpp -- the per-lane core of the frame synchroniser (include/bbb.h, bbb_framesync_* and bbb_frame_*), for the
// device and for the host: tests/framesync_host.cpp restates the kernels' walks and calls these functions from them.
// bbb_framesync_model_host, bbb_frame_extract_host and bbb_frame_attach_host are NOT built from this file: they are independent
// serial loops, one bit at a time.
//
// Everything here works on positions RELATIVE to the call's data: bit r of the data is bit r % 64 of word r / 64.
//   window distance      one funnel shift over two words, an XOR with the marker, a mask and a population count
//   candidate            within tol_search in an allowed polarity; dist(p, 1) = M - dist(p, 0)
//   run of misses        the LOCK rule on a bit mask of misses, one bit per frame of a batch: the run that ends at frame j, the
//                        misses carried into the batch counted as frames -1, -2, ... in front of it
//   decidability         what a call that is not final may decide
//   randomiser           the byte table of the Fibonacci register and its period in bytes
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FS_HD __host__ __device__ __forceinline__
#else
#define FS_HD inline
#endif

namespace bbb {

constexpr uint32_t kFsThreads = 256;
constexpr uint32_t kFsTileWords = kFsThreads;          // the search pass: a word of 64 positions a lane
constexpr uint64_t kFsTileBits = 64ull * kFsTileWords;
constexpr uint32_t kFsBatch = 4 * kFsThreads;          // the chain pass in LOCK: four frames a lane and round
constexpr uint32_t kFsMaskWords = kFsBatch / 64;
constexpr uint64_t kFsMaxBits = 1ull << 35, kFsMaxPos = 1ull << 48, kFsMaxOut = 1ull << 40;
constexpr uint32_t kFsModeSearch = 0, kFsModeLock = 1;

struct FsCfg {
    uint64_t marker, mask;                         // mask: the low M bits
    uint32_t M, F, tol_search, tol_lock, v, w, both;
    uint32_t payload_bytes;                        // (F - M) / 8 where that is whole, else 0
};

// period 0: no randomiser
struct FsRand {
    uint8_t tab[256];
    uint32_t period;
};

// word 0 of the state
struct FsWord0 {
    uint32_t mode, pol, fresh, misses, overflow, error;
};
FS_HD FsWord0 fs_unpack(uint64_t w) {
    return {(uint32_t)(w & 0xFF), (uint32_t)(w >> 8 & 1), (uint32_t)(w >> 9 & 1), (uint32_t)(w >> 16 & 0xFF), (uint32_t)(w >> 24 & 1),
            (uint32_t)(w >> 25 & 1)};
}
FS_HD uint64_t fs_pack(const FsWord0 &s, uint64_t emitted) {
    return (uint64_t)s.mode | (uint64_t)s.pol << 8 | (uint64_t)s.fresh << 9 | (uint64_t)s.misses << 16 | (uint64_t)s.overflow << 24 |
           (uint64_t)s.error << 25 | emitted << 32;
}

// nb bits (1..64) of the data from bit r on, in the low bits of the result; what lies above them is not defined.  Reads the
// second word only where the bits reach into it, so bits r .. r + nb - 1 inside the data means every read is.
FS_HD uint64_t fs_gather(const uint64_t *w, uint64_t r, uint32_t nb) {
    const uint64_t j = r >> 6;
    const uint32_t sh = (uint32_t)r & 63u;
    uint64_t x = w[j] >> sh;
    if (sh + nb > 64u) x |= w[j + 1] << (64u - sh);
    return x;
}

// dist(r, 0) of a position whose marker lies inside the data
FS_HD uint32_t fs_dist0(const uint64_t *w, uint64_t r, const FsCfg &c) {
    return (uint32_t)__builtin_popcountll((fs_gather(w, r, c.M) ^ c.marker) & c.mask);
}
FS_HD uint32_t fs_dist(const uint64_t *w, uint64_t r, uint32_t pol, const FsCfg &c) {
    const uint32_t d = fs_dist0(w, r, c);
    return pol ? c.M - d : d;
}

// 0: no candidate; 1 + pol: a candidate in that polarity (one at most, as tol_search <= M / 4)
FS_HD uint32_t fs_candidate(uint32_t d0, const FsCfg &c) {
    if (d0 <= c.tol_search) return 1;
    return c.both && c.M - d0 <= c.tol_search ? 2u : 0u;
}

// The 64 candidate bits of the positions 64 j .. 64 j + 63 from the data's words j (w0) and j + 1 (w1): every window is a
// funnel shift of the two.  Markers of up to 32 bits need the low half of it only.
FS_HD uint64_t fs_candidate_word(uint64_t w0, uint64_t w1, const FsCfg &c) {
    uint64_t cand = 0;
    if (c.M <= 32) {
        const uint32_t m = (uint32_t)c.marker, k = (uint32_t)c.mask;
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t i = 0; i < 64; ++i) {
            const uint32_t x = (uint32_t)(i ? w0 >> i | w1 << (64 - i) : w0);
            const uint32_t d = (uint32_t)__builtin_popcount((x ^ m) & k);
            cand |= (uint64_t)(fs_candidate(d, c) != 0) << i;
        }
    } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t i = 0; i < 64; ++i) {
            const uint64_t x = i ? w0 >> i | w1 << (64 - i) : w0;
            const uint32_t d = (uint32_t)__builtin_popcountll((x ^ c.marker) & c.mask);
            cand |= (uint64_t)(fs_candidate(d, c) != 0) << i;
        }
    }
    return cand;
}

// the positions of word j whose marker lies inside n bits of data: those with 64 j + i + M <= n
FS_HD uint64_t fs_valid_mask(uint64_t j, uint64_t n, uint32_t M) {
    if (n < M || 64 * j > n - M) return 0;
    const uint64_t lim = n - M - 64 * j;           // the last valid i
    return lim >= 63 ? ~0ull : (2ull << lim) - 1;
}

// the positions of word j at or behind s
FS_HD uint64_t fs_from_mask(uint64_t j, uint64_t s) {
    if (64 * j >= s) return ~0ull;
    return s - 64 * j >= 64 ? 0ull : ~0ull << (s - 64 * j);
}

// ---- decidability ---------------------------------------------------------------------------------------------------------------
// a SEARCH position needs its marker inside the data, final or not
FS_HD bool fs_search_open(uint64_t p, uint64_t n, const FsCfg &c) { return p + c.M <= n; }
// a candidate of a call that is not final needs all its confirmations inside the data
FS_HD bool fs_candidate_open(uint64_t p, uint64_t n, const FsCfg &c) { return p + (uint64_t)c.v * c.F + c.M <= n; }
// the LOCK steps the data allow from e
FS_HD uint64_t fs_lock_steps(uint64_t e, uint64_t n, const FsCfg &c) { return e + c.F <= n ? (n - e) / c.F : 0; }

// The confirmations of candidate p in polarity pol: what lies beyond the data is no hit.
FS_HD bool fs_confirm(const uint64_t *w, uint64_t p, uint32_t pol, uint64_t n, const FsCfg &c) {
    for (uint32_t j = 1; j <= c.v; ++j) {
        const uint64_t q = p + (uint64_t)j * c.F;
        if (q + c.M > n || fs_dist(w, q, pol, c) > c.tol_lock) return false;
    }
    return true;
}

// ---- the run of misses ----------------------------------------------------------------------------------------------------------
// frame i of a batch missed; i < 0: the frames in front of the batch, of which the last m0 missed
FS_HD bool fs_miss_at(const uint64_t *mm, int32_t i, uint32_t m0) {
    return i >= 0 ? (mm[i >> 6] >> (i & 63) & 1) != 0 : (uint32_t)(-i) <= m0;
}
// the misses in a row that end at frame j, counted up to w + 1: w + 1 means that the lock is lost at j or before
FS_HD uint32_t fs_miss_run(const uint64_t *mm, int32_t j, uint32_t m0, uint32_t w) {
    uint32_t n = 0;
    while (n <= w && fs_miss_at(mm, j - (int32_t)n, m0)) ++n;
    return n;
}

FS_HD uint16_t fs_meta(uint32_t d, uint32_t pol, bool fly, bool first) {
    return (uint16_t)(d | pol << 8 | (uint32_t)fly << 9 | (uint32_t)first << 10);
}

// ---- the randomiser -------------------------------------------------------------------------------------------------------------
// false: rand_poly is not 9 bits with the x^8 and x^0 terms set, or the seed is not 1..255
FS_HD bool fs_rand_table(uint32_t poly, uint32_t seed, FsRand &R) {
    for (uint32_t i = 0; i < 256; ++i) R.tab[i] = 0;
    R.period = 0;
    if (!poly) return true;
    if (poly >> 9 || !(poly >> 8) || !(poly & 1) || seed < 1 || seed > 255) return false;
    // the x^0 term makes the step invertible, so the register comes back to the seed: after pb <= 255 steps
    uint32_t s = seed, pb = 0;
    do {
        s = s >> 1 | (uint32_t)(__builtin_popcount(s & poly & 0xFF) & 1) << 7;
        ++pb;
    } while (s != seed);
    uint32_t g = pb;                               // bytes repeat after pb / gcd(pb, 8)
    for (uint32_t e = 8; e;) {
        const uint32_t r = g % e;
        g = e;
        e = r;
    }
    R.period = pb / g;
    s = seed;
    for (uint32_t i = 0; i < 8 * R.period; ++i) {
        R.tab[i >> 3] = (uint8_t)(R.tab[i >> 3] | (s & 1) << (7 - (i & 7)));
        s = s >> 1 | (uint32_t)(__builtin_popcount(s & poly & 0xFF) & 1) << 7;
    }
    return true;
}

// ---- extract: payload bytes off .. off + 7 of the frame at relative position p as one word ------------------------------------
FS_HD uint64_t fs_payload_word(const uint64_t *w, uint64_t p, uint32_t off, uint32_t nbytes, uint32_t pol, const FsCfg &c, const uint8_t *tab,
                               uint32_t period) {
    uint64_t x = fs_gather(w, p + c.M + 8ull * off, 8 * nbytes);
    if (pol) x = ~x;
    if (period) {
        uint32_t k = off % period;
        for (uint32_t b = 0; b < nbytes; ++b) {
            x ^= (uint64_t)tab[k] << (8 * b);
            if (++k == period) k = 0;
        }
    }
    return nbytes == 8 ? x : x & ((1ull << (8 * nbytes)) - 1);
}

// ---- attach: `take` bits (1..64, o + take <= F) of frame fi from its bit o on ---------------------------------------------------
FS_HD uint64_t fs_frame_bits(const uint8_t *payload, uint64_t fi, uint32_t o, uint32_t take, const FsCfg &c, const uint8_t *tab, uint32_t period) {
    uint64_t x = 0;
    uint32_t got = 0;
    if (o < c.M) {
        const uint32_t nm = take < c.M - o ? take : c.M - o;
        x = c.marker >> o & (nm == 64 ? ~0ull : (1ull << nm) - 1);
        got = nm;
        o += nm;
    }
    while (got < take) {
        const uint32_t k = o - c.M, idx = k >> 3, bit = k & 7;
        uint32_t by = payload[fi * c.payload_bytes + idx];
        if (period) by ^= tab[idx % period];
        const uint32_t nb = 8 - bit < take - got ? 8 - bit : take - got;
        x |= (uint64_t)(by >> bit & ((1u << nb) - 1)) << got;
        got += nb;
        o += nb;
    }
    return x;
}

}  // namespace bbb
