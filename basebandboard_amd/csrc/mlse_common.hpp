// mlse_common.hpp -- the per-window core of the Viterbi sequence detector (include/bbb.h, bbb_mlse_run) and the arithmetic of
// its blocks and windows, for the device and for the host: tests/mlse_host.cpp restates the kernel's walk and calls these
// functions from it.  bbb_mlse_model_host is NOT built from this file: it is an independent serial loop.
//
//   s(h, b)    = g[0] d(b) + sum_{i = 1..L} g[i] d(bit i - 1 of h)        d(1) = +1, d(0) = -1
//   gain(h, b) = 2 y s(h, b) - s(h, b)^2                                   h' = ((h << 1) | b) & (NS - 1)
// State h' is entered from h = (h' >> 1) | (c << (L - 1)), c = 0 or 1, with the bit b = h' & 1: the two transitions INTO a
// state are constants of that state.  So one state is one lane: MlseLane holds 2 s and s^2 of its two transitions, an ACS
// step takes the two predecessors' metrics (cross-lane moves on the device, an array on the host) and leaves the new metric
// and the survivor bit c; the NS survivor bits of a window's symbol are NS bits of a 64-bit word that holds 64 / NS windows
// (the device makes it with a ballot).
//
// Range: sum |g| <= 2^20 and |y| <= 2^15 give |s| <= 2^20, |2 y s| <= 2^36, s^2 <= 2^40, so |gain| < 2^41; a window is at
// most 512 symbols, so every path metric of an allowed state stays below 2^50 in magnitude: plain int64 is exact, and no
// common value is ever subtracted.  A barred state starts at -2^62: whatever it gains, it stays below -2^61, so it loses
// every comparison with an allowed path and never overflows.  (Two barred paths may compare otherwise than two minus
// infinities would, but a barred path is never on the traceback: the end state is an allowed one, and the survivor of an
// allowed state is an allowed state.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MLSE_HD __host__ __device__ __forceinline__
#else
#define MLSE_HD inline
#endif

namespace bbb {

constexpr int kMlseMaxMem = 4;
constexpr uint32_t kMlseBlockDefault = 192, kMlseWarmupDefault = 32, kMlseLookaheadDefault = 32;
constexpr uint32_t kMlseMaxEdge = 128;             // the most warm-up and the most lookahead
constexpr uint32_t kMlseMaxWindow = 512;           // B + W + D
constexpr int64_t kMlseGBound = 1 << 20;           // sum |g|
constexpr int64_t kMlseBarred = -(1ll << 62);
constexpr uint64_t kMlseSymbolLimit = 1ull << 58;  // first_symbol + nsym

struct MlseGeom { uint32_t B, W, D; };

// the three geometry fields of bbb_mlse_cfg with their defaults put in; false: outside the limits
MLSE_HD bool mlse_geom(uint32_t block, uint32_t warmup, uint32_t lookahead, MlseGeom &g) {
    g.B = block ? block : kMlseBlockDefault;
    g.W = warmup ? warmup : kMlseWarmupDefault;
    g.D = lookahead ? lookahead : kMlseLookaheadDefault;
    return g.W <= kMlseMaxEdge && g.D <= kMlseMaxEdge && g.B <= kMlseMaxWindow && g.B + g.W + g.D <= kMlseMaxWindow;
}

// ---- what a call decides -----------------------------------------------------------------------------------------------------
// The call holds the symbols [first, first + nsym).  final: all of them.  Otherwise the symbols below the largest block
// boundary E with E + D <= first + nsym: the whole blocks whose unclipped window lies inside the call.
MLSE_HD uint64_t mlse_ndecided(const MlseGeom &g, uint64_t first, uint64_t nsym, bool final) {
    if (final) return nsym;
    const uint64_t end = first + nsym;
    if (end < g.D) return 0;
    const uint64_t E = (end - g.D) / g.B * g.B;
    return E > first ? E - first : 0;
}

// The window of block j.  lo: its unclipped first symbol j B - W, which may lie before symbol 0; [a_lo, a_hi): the symbols
// the Viterbi run walks; [e_lo, e_hi): the symbols whose decisions the call emits; from_zero: the window starts at absolute
// symbol 0, where only init_state is allowed.
struct MlseWindow {
    int64_t lo;
    uint64_t a_lo, a_hi, e_lo, e_hi;
    bool from_zero;
};
MLSE_HD MlseWindow mlse_window(const MlseGeom &g, uint64_t j, uint64_t first, uint64_t nsym, uint64_t ndecided) {
    MlseWindow w;
    const uint64_t b_lo = j * g.B, b_hi = b_lo + g.B, end = first + nsym, dec = first + ndecided;
    w.lo = (int64_t)b_lo - (int64_t)g.W;
    w.from_zero = w.lo <= 0;
    w.a_lo = w.from_zero ? 0 : (uint64_t)w.lo;
    w.a_hi = b_hi + g.D < end ? b_hi + g.D : end;
    w.e_lo = b_lo > first ? b_lo : first;
    w.e_hi = b_hi < dec ? b_hi : dec;
    return w;
}

// the history in samples that keeps the first window of a call that starts at `first` from being zero-filled: its first
// symbol sits (first - a_lo) symbols before the call's, the taps reach ntaps - 1 samples further, `phase` samples of that
// lie inside the call.  At a block boundary this is min(first, W) * decim + ntaps - 1 - phase.
MLSE_HD uint64_t mlse_nbefore_wanted(const MlseGeom &g, uint64_t first, uint32_t decim, uint32_t ntaps, uint32_t phase) {
    const MlseWindow w = mlse_window(g, first / g.B, first, 0, 0);
    const uint64_t reach = (first - w.a_lo) * decim + ntaps - 1;
    return reach > phase ? reach - phase : 0;
}

// ceil(v / d) for signed v and d > 0
MLSE_HD int64_t mlse_ceil_div(int64_t v, int64_t d) { return v >= 0 ? (v + d - 1) / d : -((-v) / d); }

// ---- one state ---------------------------------------------------------------------------------------------------------------
MLSE_HD int32_t mlse_s(const int32_t *g, int L, uint32_t h, uint32_t b) {
    int32_t s = b ? g[0] : -g[0];                  // |s| <= sum |g| <= 2^20
    for (int i = 1; i <= L; ++i) s += (h >> (i - 1) & 1) ? g[i] : -g[i];
    return s;
}

MLSE_HD constexpr uint32_t mlse_pred(uint32_t hp, uint32_t c, int L) { return (hp >> 1) | (c << (L - 1)); }

struct MlseLane {
    int32_t a0, a1;                                // 2 s of the transition from predecessor c = 0, c = 1
    int64_t q0, q1;                                // s^2 of the same
};
MLSE_HD MlseLane mlse_lane(const int32_t *g, int L, uint32_t hp) {
    MlseLane r;
    const int32_t s0 = mlse_s(g, L, mlse_pred(hp, 0, L), hp & 1), s1 = mlse_s(g, L, mlse_pred(hp, 1, L), hp & 1);
    r.a0 = 2 * s0;
    r.a1 = 2 * s1;
    r.q0 = (int64_t)s0 * s0;
    r.q1 = (int64_t)s1 * s1;
    return r;
}

// the metric a window's state starts with
MLSE_HD int64_t mlse_start(bool from_zero, uint32_t h, uint32_t init_state) {
    return from_zero && h != init_state ? kMlseBarred : 0;
}

// add-compare-select: m0, m1 the metrics of the predecessors c = 0, c = 1.  The larger candidate survives; a tie goes to c = 0.
MLSE_HD int64_t mlse_acs(const MlseLane &r, int32_t y, int64_t m0, int64_t m1, uint32_t &c) {
    const int64_t c0 = m0 + (int64_t)y * r.a0 - r.q0, c1 = m1 + (int64_t)y * r.a1 - r.q1;
    c = c1 > c0;
    return c ? c1 : c0;
}

// the end state: (ma, ia) is kept against (mb, ib) when it is larger, or equal at the lower index
MLSE_HD bool mlse_keeps(int64_t ma, uint32_t ia, int64_t mb, uint32_t ib) { return ma > mb || (ma == mb && ia < ib); }

// one step of the traceback: the path is in state s behind the symbol whose survivor word is `word` (the window's NS bits
// start at bit `base`); `bit` is that symbol's decision, the result the state behind the symbol before it
MLSE_HD uint32_t mlse_back(uint64_t word, uint32_t base, uint32_t s, int L, uint32_t &bit) {
    bit = s & 1;
    return mlse_pred(s, (uint32_t)(word >> (base + s)) & 1u, L);
}

}  // namespace bbb
