// dfe_common.hpp -- the per-symbol core of the decision-feedback equalizer (include/bbb.h, bbb_dfe_run) and the rules of its
// regions, for the device and for the host: tests/dfe_host.cpp restates the kernels' walk and calls these functions from it.
//
//   v[k] = a[k] - sum_{i < nfb} fb[i] d[k - 1 - i]      bit[k] = v[k] >= threshold (strict: >)      d = +1 / -1
// The loop's memory is the nfb last decisions: a state h, bit i = the decision of symbol k - 1 - i, one of NS = 2^nfb.  One
// symbol takes h to ((h << 1) | bit) & (NS - 1), and its bit depends on h through F[h] = sum fb[i] d_i(h) alone.  So a
// symbol IS a map of NS states onto NS states: NS nibbles of one 64-bit word, nibble h = the state that h goes to (the
// nibbles from NS on are 0).  Maps compose associatively, compose(f, g) = f first, then g, so a run of symbols can be
// reduced in any grouping that keeps their order: a wave scans them, a workgroup chains the waves' totals, a region's
// total is one word, and a chain of regions is again a chain of words.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DFE_HD __host__ __device__ __forceinline__
#else
#define DFE_HD inline
#endif

namespace bbb {

constexpr int kDfeMaxFb = 4;
constexpr int kDfeThreads = 256;                   // one symbol per thread and round; a wave's 64 symbols are k & ~63 .. + 63
constexpr int kDfeStepSamples = 2048;              // = kFirTile: the inputs a workgroup stages at once
constexpr uint32_t kDfeRegionDefault = 4096;       // symbols of a region
constexpr uint32_t kDfeWarmupDefault = 64;         // symbols run in front of a region to find its start
constexpr uint32_t kDfeChainThreads = 256;
constexpr uint64_t kDfeMaxRegions = 1ull << 26;

struct DfeRule {
    int32_t fb[kDfeMaxFb];                         // 0 from nfb on
    int32_t F[1 << kDfeMaxFb];                     // F[h] = sum_i fb[i] * (bit i of h ? 1 : -1)
    int32_t threshold;
    int32_t strict;
};

DFE_HD void dfe_rule(DfeRule &r, const int32_t *fb, uint32_t nfb, int32_t threshold, int strict) {
    for (int i = 0; i < kDfeMaxFb; ++i) r.fb[i] = (uint32_t)i < nfb ? fb[i] : 0;
    for (int h = 0; h < (1 << kDfeMaxFb); ++h) {
        int64_t f = 0;
        for (int i = 0; i < kDfeMaxFb; ++i) f += (h >> i & 1) ? (int64_t)r.fb[i] : -(int64_t)r.fb[i];
        r.F[h] = (int32_t)f;                       // |f| <= sum |fb| < 2^31
    }
    r.threshold = threshold;
    r.strict = strict != 0;
}

template <int NS>
DFE_HD constexpr uint64_t dfe_identity() {
    uint64_t m = 0;
    for (int h = 0; h < NS; ++h) m |= (uint64_t)h << (4 * h);
    return m;
}

// v of a symbol whose feed-forward sum is a, after state s.  Exact in int32 by the bound on sum |h| and sum |fb|.
DFE_HD int32_t dfe_v(int32_t a, const DfeRule &r, uint32_t s) {
    int32_t f = 0;
#pragma unroll
    for (int i = 0; i < kDfeMaxFb; ++i) f += (s >> i & 1) ? r.fb[i] : -r.fb[i];
    return a - f;
}

// D: bit h = the symbol's decision after state h
template <int NS>
DFE_HD uint32_t dfe_decisions(int32_t a, const DfeRule &r) {
    uint32_t D = 0;
#pragma unroll
    for (int h = 0; h < NS; ++h) {
        const int32_t v = a - r.F[h];
        D |= (uint32_t)(r.strict ? v > r.threshold : v >= r.threshold) << h;
    }
    return D;
}

template <int NS>
DFE_HD uint64_t dfe_map(uint32_t D) {
    uint64_t m = 0;
#pragma unroll
    for (int h = 0; h < NS; ++h) m |= (uint64_t)(((h << 1) | (D >> h & 1)) & (NS - 1)) << (4 * h);
    return m;
}

DFE_HD uint32_t dfe_apply(uint64_t m, uint32_t s) { return (uint32_t)(m >> (4 * s)) & 15u; }

// byte i of the result is byte (selector byte i) of the eight bytes hi:lo, selector bytes 0..7: v_perm_b32
DFE_HD uint32_t dfe_perm8(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t t = (uint64_t)hi << 32 | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= (uint32_t)(t >> (8 * (sel >> (8 * i) & 7)) & 0xFF) << (8 * i);
    return r;
#endif
}

// f first, then g.  Up to four states nibble by nibble.  Eight and sixteen states four nibbles at a time: g's even and odd
// nibbles are spread to one per byte (two tables of eight bytes), four nibbles of f, one per byte, select bytes of both
// tables with bits 3..1 and between the two with bit 0.
template <int NS>
DFE_HD uint64_t dfe_compose(uint64_t f, uint64_t g) {
    if constexpr (NS <= 4) {
        uint64_t m = 0;
#pragma unroll
        for (int h = 0; h < NS; ++h) m |= (uint64_t)dfe_apply(g, dfe_apply(f, (uint32_t)h)) << (4 * h);
        return m;
    } else {
        constexpr uint64_t low = 0x0F0F0F0F0F0F0F0Full;
        const uint64_t ge = g & low, go = (g >> 4) & low, fe = f & low, fo = (f >> 4) & low;
        const uint32_t ge0 = (uint32_t)ge, ge1 = (uint32_t)(ge >> 32), go0 = (uint32_t)go, go1 = (uint32_t)(go >> 32);
        auto look = [&](uint32_t x) {
            const uint32_t sel = (x >> 1) & 0x07070707u, odd = (x & 0x01010101u) * 0xFFu;
            return (dfe_perm8(ge1, ge0, sel) & ~odd) | (dfe_perm8(go1, go0, sel) & odd);
        };
        uint64_t re = look((uint32_t)fe), ro = look((uint32_t)fo);
        if constexpr (NS > 8) {
            re |= (uint64_t)look((uint32_t)(fe >> 32)) << 32;
            ro |= (uint64_t)look((uint32_t)(fo >> 32)) << 32;
        }
        return re | ro << 4;
    }
}

// every state goes to the same one: what came before no longer matters
template <int NS>
DFE_HD bool dfe_constant(uint64_t m) {
    return m == (m & 15u) * (0x1111111111111111ull >> (64 - 4 * NS));
}

// ---- the geometry of a walk --------------------------------------------------------------------------------------------------
// Symbol k sits at input phase + k * decim.  A step is the kDfeStepSamples inputs from `base` on; of the symbols [k_lo, k_hi)
// it holds [q_lo, q_hi).  A step is walked in rounds of kDfeThreads symbols from q_lo & ~63 on, thread t of a round taking
// symbol rb + t, so that a wave's 64 lanes are the 64 bits of one output word.
DFE_HD void dfe_step_symbols(uint64_t base, uint32_t decim, uint32_t phase, uint64_t k_lo, uint64_t k_hi, uint64_t &q_lo, uint64_t &q_hi) {
    const uint64_t end = base + kDfeStepSamples;
    const uint64_t lo = base <= phase ? 0 : (base - phase + decim - 1) / decim;
    const uint64_t hi = end <= phase ? 0 : (end - phase + decim - 1) / decim;
    q_lo = lo > k_lo ? lo : k_lo;
    q_hi = hi < k_hi ? hi : k_hi;
    if (q_hi < q_lo) q_hi = q_lo;
}

// ---- the rules of the regions ------------------------------------------------------------------------------------------------
// Region r is the symbols [r R, min((r + 1) R, nsym)).  Region 0 starts from the call's state word.  Every other region
// runs the W symbols in front of it (fewer where the record starts) into the map Mw: where Mw is constant its value IS the
// region's start, otherwise the region speculates Mw(0).  It leaves two words, its own map and dfe_info(start, proven).
template <int NS>
DFE_HD uint32_t dfe_start(uint64_t mw, bool &proven) {
    proven = dfe_constant<NS>(mw);
    return dfe_apply(mw, 0);
}
DFE_HD uint64_t dfe_info(uint32_t start, bool proven) { return start | (uint64_t)proven << 8; }
DFE_HD uint32_t dfe_info_start(uint64_t info) { return (uint32_t)info & 15u; }
DFE_HD bool dfe_info_proven(uint64_t info) { return (info >> 8 & 1) != 0; }

// The chain: kDfeChainThreads threads, thread t owns the regions [t per, min((t + 1) per, nreg)), per = ceil(nreg / threads).
// It composes their maps, takes the state in front of its share from the totals of the threads before it, and replays its
// share: wrong(r, s) for every region whose start was not s; returns the state behind its share.
DFE_HD uint64_t dfe_chain_share(uint64_t nreg) { return (nreg + kDfeChainThreads - 1) / kDfeChainThreads; }

template <int NS>
DFE_HD uint64_t dfe_chain_total(const uint64_t *rec, uint64_t lo, uint64_t hi) {
    uint64_t m = dfe_identity<NS>();
    for (uint64_t r = lo; r < hi; ++r) m = dfe_compose<NS>(m, rec[2 * r]);
    return m;
}

template <class Wrong>
DFE_HD uint32_t dfe_chain_replay(const uint64_t *rec, uint64_t lo, uint64_t hi, uint32_t s, uint32_t &unproven, Wrong wrong) {
    for (uint64_t r = lo; r < hi; ++r) {
        const uint64_t info = rec[2 * r + 1];
        if (!dfe_info_proven(info)) ++unproven;
        if (dfe_info_start(info) != s) wrong(r, s);
        s = dfe_apply(rec[2 * r], s);
    }
    return s;
}

// a flagged region and its true start, as the repair kernel reads them
DFE_HD uint64_t dfe_flag(uint64_t r, uint32_t s) { return r | (uint64_t)s << 32; }

}  // namespace bbb
