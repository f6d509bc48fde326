// carrier_common.hpp -- the per-pair and per-block core of the carrier recovery (include/bbb.h, bbb_carrier_run) and the
// geometry of its passes, for the device and for the host: tests/carrier_host.cpp restates the passes and calls these functions.
//
// A block is L pairs (I, Q).  Squaring a BPSK pair doubles its angle and so removes the data: the block's sums
// SR = sum(I I - Q Q), SI = 2 sum(I Q) point at twice the carrier's phase, the CORDIC of ddc_common.hpp gives that angle and
// half of it is h_j, the phase modulo half a turn.  The serial part is the unwrap, est_j = h_j or h_j + half a turn, whichever
// lies within a quarter turn of est_(j-1).  With est_j = h_j + 32768 b_j that is b_j = b_(j-1) XOR f_j, where f_j depends on
// h_j and h_(j-1) alone: the state is ONE BIT and the scan a prefix XOR.  Also est_j - est_(j-1) = h_j - h_(j-1) + 32768 f_j
// modulo 2^16, so no counter of stats_dev needs b either.
#pragma once
#include <cstdint>

#include "ddc_common.hpp"

#if defined(__HIPCC__)
#define CAR_HD __host__ __device__ __forceinline__
#else
#define CAR_HD inline
#endif

namespace bbb {

constexpr int kCarrierThreads = 256;
constexpr uint32_t kCarrierPairsPerThread = 8;
constexpr uint32_t kCarrierTileMax = kCarrierThreads * kCarrierPairsPerThread;       // 2048 pairs
constexpr uint32_t kCarrierBlockDefault = 32;
constexpr uint32_t kCarrierChunkDefault = 1024, kCarrierChunkMax = 65536;             // blocks of a chunk
constexpr uint32_t kCarrierFlagPer = 8, kCarrierFlagTurn = kCarrierThreads * kCarrierFlagPer;     // blocks of a thread and of a turn of the flag pass
constexpr int kCarrierGridPerCu = 8;               // workgroups per compute unit of the sum, flag and rotate kernels
constexpr uint64_t kCarrierStarted = 1ull << 63;
constexpr uint64_t kCarrierPairLimit = 1ull << 58;

struct CarrierGeom {
    uint32_t L, chunk;                             // pairs of a block (a multiple of 8); blocks of a chunk
    uint64_t nin;                                  // the pairs that count: nconsumed of a call that is not final
    uint64_t nblocks, nchunks;
};

// ---- the plan -----------------------------------------------------------------------------------------------------------------
CAR_HD void carrier_plan(uint32_t L, uint64_t nin, bool final, uint64_t &nblocks, uint64_t &nconsumed) {
    nblocks = final ? (nin + L - 1) / L : nin / L;
    nconsumed = nblocks * L < nin ? nblocks * L : nin;
}
CAR_HD uint64_t carrier_bit_words(uint64_t nblocks, uint32_t L) { return (nblocks * L + 63) / 64; }

// ---- the pair's and the block's rule ------------------------------------------------------------------------------------------
// I I - Q Q and I Q of one pair, added to int64 sums; either lies within 2^30, the sums of 1024 of them within 2^40
CAR_HD void carrier_square(int i, int q, int64_t &sr, int64_t &siq) {
    sr += (int64_t)(i * i - q * q);
    siq += (int64_t)(i * q);
}

CAR_HD int carrier_bitlength(uint64_t m) {
    if (m == 0) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
    return 64 - __clzll((long long)m);
#else
    return 64 - __builtin_clzll(m);
#endif
}

// h of a block from SR and sum(I Q): the doubled angle's CORDIC phase, halved; *zero: both sums are 0
CAR_HD uint32_t carrier_h(int64_t sr, int64_t siq, bool *zero) {
    const int64_t si = 2 * siq;
    const uint64_t ar = (uint64_t)(sr < 0 ? -sr : sr), ai = (uint64_t)(si < 0 ? -si : si), m = ar > ai ? ar : ai;
    const int bl = carrier_bitlength(m), s = bl > 15 ? bl - 15 : 0;
    uint32_t mag;
    int theta2;
    ddc_polar((int)(sr >> s), (int)(si >> s), mag, theta2);
    *zero = m == 0;
    return ((uint32_t)theta2 & 0xFFFFu) >> 1;
}

CAR_HD bool carrier_near(uint32_t d) {
    d &= 0xFFFFu;
    return d < 16384u || d >= 49152u;
}
// f_j from h_j and h_(j-1)
CAR_HD uint32_t carrier_flip(uint32_t h, uint32_t hprev) { return carrier_near(h - hprev) ? 0u : 1u; }
// wrap16(est_j - est_(j-1)) from the same and f_j
CAR_HD int carrier_step(uint32_t h, uint32_t hprev, uint32_t f) { return (int)(int16_t)(uint16_t)(h - hprev + 32768u * f); }

// est_(-1) of a call from the state word and init_phase
CAR_HD uint32_t carrier_state_est(uint64_t s0, uint32_t init_phase) { return (s0 & kCarrierStarted) ? (uint32_t)(s0 & 0xFFFFu) : init_phase & 0xFFFFu; }

CAR_HD int carrier_sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
// the ROM addresses of an estimate, and the pair turned back by it
CAR_HD uint32_t carrier_adr_sin(uint32_t est) { return (est & 0xFFFFu) >> 6; }
CAR_HD uint32_t carrier_adr_cos(uint32_t est) { return (carrier_adr_sin(est) + 256u) & 1023u; }
CAR_HD void carrier_rotate(int i, int q, int c, int s, int &io, int &qo) {
    io = carrier_sat16((i * c + q * s) >> 15);
    qo = carrier_sat16((q * c - i * s) >> 15);
}
CAR_HD bool carrier_decide(int io, int threshold, bool strict) { return strict ? io > threshold : io >= threshold; }

// ---- tiles ------------------------------------------------------------------------------------------------------------------------
// A workgroup stages floor(2048 / L) whole blocks at a time; a thread owns 8 consecutive pairs, which lie in one block
// because L is a multiple of 8, and L / 8 consecutive threads own a block.
CAR_HD uint32_t carrier_blocks_per_tile(uint32_t L) { return kCarrierTileMax / L; }
CAR_HD uint32_t carrier_tile_pairs(uint32_t L) { return carrier_blocks_per_tile(L) * L; }
CAR_HD uint64_t carrier_ntiles(const CarrierGeom &g) {
    const uint32_t G = carrier_blocks_per_tile(g.L);
    return (g.nblocks + G - 1) / G;
}
// The threads of a block join their sums in two steps: `fold` lanes (the largest power of two that divides L / 8, at most
// 64: such a group never straddles a block or a wave) by shuffles, then the block's (L / 8) / fold groups through LDS.
CAR_HD uint32_t carrier_fold(uint32_t L) {
    uint32_t f = 1;
    while (f < 64 && (L / 8) % (2 * f) == 0) f *= 2;
    return f;
}

// ---- the chain ----------------------------------------------------------------------------------------------------------------------
// kCarrierThreads threads own a share of consecutive chunks each
CAR_HD uint64_t carrier_chain_share(uint64_t nchunks) { return (nchunks + kCarrierThreads - 1) / kCarrierThreads; }

}  // namespace bbb
