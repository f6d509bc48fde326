// timing_common.hpp -- the per-block core of the symbol timing recovery (include/bbb.h, bbb_timing_run) and the geometry of
// its three passes, for the device and for the host: tests/timing_host.cpp restates the passes and calls these functions.
//
// A block is L symbols of P samples.  Its metric E[p] = sum_i |a(j L P + i P + p) - threshold| ranks the P sampling phases;
// the tracker moves its phase by at most one per block, towards the larger neighbour when that beats the current phase by
// more than cur >> h.  The move depends on the block's metric and on the phase the block is entered in and on nothing else,
// so a block IS a map of P phases onto P phases (one byte per phase: the move + 1), and so is any run of blocks.  Maps
// compose associatively: a chunk of blocks is walked from every start phase at once, the chunks' maps are chained by one
// workgroup, and every chunk is walked once more from its true start.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TIM_HD __host__ __device__ __forceinline__
#else
#define TIM_HD inline
#endif

namespace bbb {

constexpr uint32_t kTimingAcquire = 0xFFFFFFFFu;   // BBB_TIMING_ACQUIRE
constexpr int kTimingThreads = 256;
constexpr uint32_t kTimingTile = 2048;             // = kFirTile: the inputs a workgroup stages at once
constexpr uint32_t kTimingBlockDefault = 64, kTimingShiftDefault = 4;
constexpr uint32_t kTimingChunkDefault = 1024, kTimingChunkMax = 65536;   // blocks of a chunk
constexpr uint32_t kTimingStage = 16384;           // bytes of move maps a chunk walk holds in LDS at once
constexpr uint32_t kTimingChainSlots = 4096;       // shares * P of the chain kernel
constexpr uint64_t kTimingLocked = 1ull << 63;

struct TimingGeom {
    uint32_t P, L, h, chunk;                       // chunk: blocks of a chunk, 1 .. kTimingChunkMax
    uint32_t LP;                                   // samples of a block, <= 65536
    uint64_t nin;                                  // the samples that count: nconsumed of a call that is not final
    uint64_t nblocks, nchunks;
};

// ---- the plan -----------------------------------------------------------------------------------------------------------------
TIM_HD void timing_plan(uint32_t P, uint32_t L, uint64_t nin, bool final, uint64_t &nblocks, uint64_t &nconsumed, uint64_t &max_bits) {
    const uint64_t LP = (uint64_t)L * P;
    nblocks = final ? (nin + LP - 1) / LP : nin / LP;
    nconsumed = nblocks * LP < nin ? nblocks * LP : nin;
    max_bits = nblocks * (L + 1);
}

// ---- the block's rule -----------------------------------------------------------------------------------------------------------
// one term of the metric; below 2^32 for every int32 a and threshold that bbb_fir_cfg allows
TIM_HD uint32_t timing_term(int32_t a, int32_t threshold) {
    const int64_t d = (int64_t)a - threshold;
    return (uint32_t)(d < 0 ? -d : d);
}

TIM_HD int timing_move(uint64_t cur, uint64_t up, uint64_t dn, uint32_t h) {
    const uint64_t lim = cur + (cur >> h);
    if (up > lim && up >= dn) return 1;
    if (dn > lim) return -1;
    return 0;
}

// the move of a block entered in phase phi, from its P metrics
TIM_HD int timing_move_at(const uint64_t *E, uint32_t P, uint32_t phi, uint32_t h) {
    return timing_move(E[phi], E[phi + 1 == P ? 0 : phi + 1], E[phi == 0 ? P - 1 : phi - 1], h);
}

// the arg-max of a first block: the lowest p on a tie
TIM_HD uint32_t timing_argmax(const uint64_t *E, uint32_t P) {
    uint32_t best = 0;
    for (uint32_t p = 1; p < P; ++p)
        if (E[p] > E[best]) best = p;
    return best;
}

// phi moves by m (-1, 0, 1); returns the wrap
TIM_HD int timing_step(uint32_t &phi, int m, uint32_t P) {
    if (m > 0) {
        phi = phi + 1 == P ? 0 : phi + 1;
        return phi == 0 ? 1 : 0;
    }
    if (m < 0) {
        phi = phi == 0 ? P - 1 : phi - 1;
        return phi == P - 1 ? -1 : 0;
    }
    return 0;
}

// Block j in phase phi emits the instants j L P + phi + i P for i in [w, imax): imax is what the record's end leaves of L.
TIM_HD uint32_t timing_imax(const TimingGeom &g, uint64_t j, uint32_t phi) {
    if ((j + 1) * g.LP <= g.nin) return g.L;       // a whole block: every block but a final call's last (no division on the walks)
    const uint64_t first = j * g.LP + phi;
    if (first >= g.nin) return 0;
    const uint64_t n = (g.nin - first + g.P - 1) / g.P;
    return n < g.L ? (uint32_t)n : g.L;
}
TIM_HD uint32_t timing_count(const TimingGeom &g, uint64_t j, uint32_t phi, int w) {
    const int n = (int)timing_imax(g, j, phi) - w;
    return n > 0 ? (uint32_t)n : 0u;
}

// One block of a walk: `code` is the block's map entry for phi (move + 1); a first block after reset goes to `first_phi`
// whatever phi was and neither moves nor wraps.  Returns the bits the block emits.
TIM_HD uint32_t timing_walk_block(const TimingGeom &g, uint64_t j, bool first, uint32_t first_phi, uint32_t code, uint32_t &phi, int &m, int &w) {
    if (first) {
        phi = first_phi;
        m = w = 0;
    } else {
        m = (int)code - 1;
        w = timing_step(phi, m, g.P);
    }
    return timing_count(g, j, phi, w);
}

// what block records hold for the gather pass
TIM_HD uint16_t timing_info(uint32_t phi, int w) { return (uint16_t)(phi | (uint32_t)(w + 1) << 8); }
TIM_HD uint32_t timing_info_phi(uint16_t info) { return info & 0xFFu; }
TIM_HD int timing_info_wrap(uint16_t info) { return (int)(info >> 8) - 1; }

// ---- tiles ------------------------------------------------------------------------------------------------------------------------
// The metric and gather passes stage kTimingTile samples at a time.  A block of at most a tile: a tile holds G whole blocks
// from its first sample on.  A longer block: it is cut into tiles of its own from its first sample on.
TIM_HD uint32_t timing_blocks_per_tile(uint32_t LP) { return LP <= kTimingTile ? kTimingTile / LP : 1; }
TIM_HD uint32_t timing_tiles_per_block(uint32_t LP) { return LP <= kTimingTile ? 1 : (LP + kTimingTile - 1) / kTimingTile; }
// groups: what one workgroup step of the metric pass owns, one tile of several blocks or the tiles of one block
TIM_HD uint64_t timing_ngroups(const TimingGeom &g) {
    const uint32_t G = timing_blocks_per_tile(g.LP);
    return (g.nblocks + G - 1) / G;
}
TIM_HD uint64_t timing_ntiles(const TimingGeom &g) { return timing_ngroups(g) * timing_tiles_per_block(g.LP); }

struct TimingTile {
    uint64_t j0;                                   // the first block
    uint32_t nblk;                                 // blocks in it (a longer block: 1)
    uint32_t off;                                  // the tile's first sample counted from block j0's first
    uint32_t len;                                  // samples of the tile that belong to its blocks
    uint64_t base;                                 // the tile's first sample
};
TIM_HD TimingTile timing_tile(const TimingGeom &g, uint64_t tile) {
    TimingTile t;
    const uint32_t G = timing_blocks_per_tile(g.LP), T = timing_tiles_per_block(g.LP);
    if (T == 1) {
        t.j0 = tile * G;
        const uint64_t left = g.nblocks - t.j0;
        t.nblk = left < G ? (uint32_t)left : G;
        t.off = 0;
        t.len = t.nblk * g.LP;
    } else {
        t.j0 = tile / T;
        t.nblk = 1;
        t.off = (uint32_t)(tile % T) * kTimingTile;
        t.len = g.LP - t.off < kTimingTile ? g.LP - t.off : kTimingTile;
    }
    t.base = t.j0 * g.LP + t.off;
    return t;
}

// The metric fold: a (block, phase) pair of a tile is summed by `split` threads (a power of two, so that they are lanes of
// one wave); thread s takes the pair's samples s, s + split, ...  pairs * split <= kTimingThreads.
TIM_HD uint32_t timing_split(uint32_t P, uint32_t LP) {
    const uint32_t pairs = timing_blocks_per_tile(LP) * P;
    uint32_t s = 1;
    while (2 * s * pairs <= (uint32_t)kTimingThreads && 2 * s <= 64) s *= 2;
    return s;
}
// the tile-relative index of the pair's first sample, and the end of its samples in the tile
TIM_HD void timing_pair_span(const TimingGeom &g, const TimingTile &t, uint32_t jb, uint32_t p, uint32_t &k0, uint32_t &kend) {
    if (t.off == 0) {
        k0 = jb * g.LP + p;
        kend = jb * g.LP + (g.LP < kTimingTile ? g.LP : kTimingTile);
    } else {
        const uint32_t r = t.off % g.P;            // the phase of the tile's first sample
        k0 = p >= r ? p - r : p + g.P - r;
        kend = t.len;
    }
}

// The gather pass: the instants of block j (phase phi, wrap w) that tile t holds are i in [ilo, ihi); the sample one in front
// of a block belongs to the block's first tile.
TIM_HD void timing_tile_instants(const TimingGeom &g, const TimingTile &t, uint64_t j, uint32_t phi, int w, int &ilo, int &ihi) {
    const int imax = (int)timing_imax(g, j, phi);
    ilo = w;
    ihi = imax;
    if (timing_tiles_per_block(g.LP) > 1) {
        if (t.off) {
            const int lo = (int)((t.off - phi + g.P - 1) / g.P);
            if (lo > ilo) ilo = lo;
        }
        const int hi = (int)((t.off + kTimingTile - phi + g.P - 1) / g.P);
        if (hi < ihi) ihi = hi;
    }
    if (ihi < ilo) ihi = ilo;
}

// ---- the chain ----------------------------------------------------------------------------------------------------------------------
// kTimingChainSlots / P threads (at most kTimingThreads) own a share of consecutive chunks each.
TIM_HD uint32_t timing_chain_threads(uint32_t P) {
    const uint32_t t = kTimingChainSlots / P;
    return t < (uint32_t)kTimingThreads ? t : (uint32_t)kTimingThreads;
}
TIM_HD uint64_t timing_chain_share(uint64_t nchunks, uint32_t P) {
    const uint32_t t = timing_chain_threads(P);
    return (nchunks + t - 1) / t;
}
// f first, then g, for one start phase: maps are bytes, bits add up along the way
TIM_HD void timing_compose(const uint8_t *map, const uint32_t *bits, uint64_t c, uint32_t P, uint32_t &phi, uint64_t &nbits) {
    nbits += bits[c * P + phi];
    phi = map[c * P + phi];
}

// the phase of a state word: the low 32 bits, folded into [0, P)
TIM_HD uint32_t timing_state_phi(uint64_t s, uint32_t P) { return (uint32_t)(s & 0xFFFFFFFFull) % P; }

}  // namespace bbb
