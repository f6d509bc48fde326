// conv_common.hpp -- the per-lane core of the convolutional codec (include/bbb.h, bbb_conv_*), its puncture tables and the
// position arithmetic, for the device and for the host: tests/conv_host.cpp restates the kernel's walk and calls these
// functions from it.  bbb_conv_model_host and bbb_conv_encode_host are NOT built from this file: they are independent serial
// loops.  The blocks and windows are mlse_common.hpp's (MlseGeom, mlse_ndecided, mlse_window) under this codec's defaults.
//
//   r = (h << 1) | b,  c_i = parity of the bits j of r with bit K-1-j of gen[i] set,  h' = r & (NS - 1)
//   gain = sum_i r_i d(c_i)                                    d(1) = +1, d(0) = -1
// State h' is entered from h = (h' >> 1) | (c << (K-2)), c = 0 or 1, with the bit b = h' & 1: the coded bits of the two
// transitions INTO a state are constants of that state.  So one state is one lane: ConvLane holds d(c_i) of its two
// transitions, an ACS step takes the two predecessors' metrics and leaves the new metric and the survivor bit c; the NS
// survivor bits of a window's step are NS bits of a 64-bit word that holds 64 / NS windows (the device makes it with a ballot).
//
// Range: |r_i| <= 32768 and n <= 3 give |gain| <= 3 * 32768 < 2^17; a window is at most 512 steps, so every path metric of an
// allowed state stays below 2^26 in magnitude: plain int32 is exact, and no common value is ever subtracted.  A barred state
// starts at -2^30: whatever it gains it stays within [-2^30 - 2^26, -2^30 + 2^26], so it loses every comparison with an
// allowed path and never overflows.  Barred paths compare among themselves as the integers they are, which the definition
// says too (a terminated window shorter than K-1 steps may end on one).
#pragma once
#include "mlse_common.hpp"

#define CONV_HD MLSE_HD

namespace bbb {

constexpr uint32_t kConvMinK = 3, kConvMaxK = 7, kConvMaxN = 3, kConvMaxPeriod = 16;
constexpr uint32_t kConvBlockDefault = 192, kConvWarmupDefault = 64, kConvLookaheadDefault = 64;
constexpr int32_t kConvBarred = -(1 << 30);
constexpr uint64_t kConvStepLimit = 1ull << 58;    // first_step + nsteps
constexpr uint64_t kConvValueLimit = 1ull << 60;   // nin

// the three geometry fields of bbb_conv_cfg with their defaults put in; false: outside the limits (MlseGeom's own)
CONV_HD bool conv_geom(uint32_t block, uint32_t warmup, uint32_t lookahead, MlseGeom &g) {
    g.B = block ? block : kConvBlockDefault;
    g.W = warmup ? warmup : kConvWarmupDefault;
    g.D = lookahead ? lookahead : kConvLookaheadDefault;
    return g.W <= kMlseMaxEdge && g.D <= kMlseMaxEdge && g.B <= kMlseMaxWindow && g.B + g.W + g.D <= kMlseMaxWindow;
}

// ---- puncturing ----------------------------------------------------------------------------------------------------------------
// cum[r]: the bits the steps 0 .. r - 1 of a period transmit (cum[p] = ptot); inv_step / inv_bit: the step of the period and
// the coded bit behind transmitted bit number x < ptot of a period; recip = ceil(2^32 / p), with which x / p is a multiply
// for every x < 2^28 (x recip / 2^32 = x / p + x e / (p 2^32) with e < p <= 16: the excess stays below 1 / p).
struct ConvPunct {
    uint32_t n, p, ptot;
    uint64_t recip;                                // (2^32 itself at p = 1)
    uint16_t keep[kConvMaxN];
    uint8_t cum[kConvMaxPeriod + 1];
    uint8_t inv_step[kConvMaxN * kConvMaxPeriod], inv_bit[kConvMaxN * kConvMaxPeriod];
};

// false: a period outside 1..16, a mask with bits beyond the period, a step that transmits nothing
CONV_HD bool conv_punct(uint32_t n, uint32_t period, const uint32_t *keep, ConvPunct &P) {
    if (n < 2 || n > kConvMaxN || period < 1 || period > kConvMaxPeriod) return false;
    P.n = n;
    P.p = period;
    P.recip = ((1ull << 32) + period - 1) / period;
    for (uint32_t i = 0; i < kConvMaxN; ++i) {
        if (i < n && (keep[i] >> period)) return false;
        P.keep[i] = i < n ? (uint16_t)keep[i] : 0;
    }
    uint32_t tot = 0;
    for (uint32_t r = 0; r < period; ++r) {
        P.cum[r] = (uint8_t)tot;
        const uint32_t was = tot;
        for (uint32_t i = 0; i < n; ++i)
            if (P.keep[i] >> r & 1) {
                P.inv_step[tot] = (uint8_t)r;
                P.inv_bit[tot] = (uint8_t)i;
                ++tot;
            }
        if (tot == was) return false;
    }
    for (uint32_t r = period; r <= kConvMaxPeriod; ++r) P.cum[r] = (uint8_t)tot;
    P.ptot = tot;
    return true;
}

// the transmitted bits in front of step t
CONV_HD uint64_t conv_idx(const ConvPunct &P, uint64_t t) { return t / P.p * P.ptot + P.cum[t % P.p]; }

// the largest t with idx(t) <= x (cum rises strictly: every step transmits)
CONV_HD uint64_t conv_steps_below(const ConvPunct &P, uint64_t x) {
    const uint32_t rem = (uint32_t)(x % P.ptot);
    uint32_t r = 0;
    while (r + 1 < P.p && P.cum[r + 1] <= rem) ++r;
    return x / P.ptot * P.p + r;
}

// The step i steps behind a step whose place in its period is r0 and whose first value is number `base`: its place r in the
// period and the number of its first value.  i + r0 < 2^28.
CONV_HD int64_t conv_value_of_step(const ConvPunct &P, int64_t base, uint32_t r0, uint32_t i, uint32_t &r) {
    const uint32_t x = r0 + i, q = (uint32_t)((x * P.recip) >> 32);
    r = x - q * P.p;
    return base + (int64_t)q * P.ptot + (int64_t)P.cum[r] - (int64_t)P.cum[r0];
}

// received value number e of the buffer: an int16, or a packed bit as +1 / -1
CONV_HD int32_t conv_value(const void *in, bool hard, uint64_t e) {
    if (hard) return (static_cast<const uint64_t *>(in)[e >> 6] >> (e & 63) & 1) ? 1 : -1;
    return static_cast<const int16_t *>(in)[e];
}

// The n values of a step at place r of its period whose first value is number `rel` counted from the call's first (element
// in_first of the buffer): 0 where the bit is punctured and outside [rel_lo, rel_hi), the history and the call's values.
CONV_HD void conv_step_values(const ConvPunct &P, const void *in, bool hard, uint64_t in_first, int64_t rel, int64_t rel_lo, int64_t rel_hi,
                              uint32_t r, int16_t v[kConvMaxN]) {
    for (uint32_t i = 0; i < kConvMaxN; ++i) {
        v[i] = 0;
        if (i < P.n && (P.keep[i] >> r & 1)) {
            if (rel >= rel_lo && rel < rel_hi) v[i] = (int16_t)conv_value(in, hard, (uint64_t)((int64_t)in_first + rel));
            ++rel;
        }
    }
}

// ---- one state -----------------------------------------------------------------------------------------------------------------
// coded bit of generator gen for the input bit b entering state h: with the window w = r read oldest bit first, bit m of w the
// input bit K-1-m steps back, the rule of bbb.h is the parity of w & gen -- the conventional notation is this window's
CONV_HD uint32_t conv_code_bit(uint32_t gen, int K, uint32_t h, uint32_t b) {
    const uint32_t r = (h << 1) | b;
    uint32_t par = 0;
    for (int j = 0; j < K; ++j) par ^= (r >> j) & (gen >> (K - 1 - j));
    return par & 1;
}

CONV_HD constexpr uint32_t conv_pred(uint32_t hp, uint32_t c, int K) { return (hp >> 1) | (c << (K - 2)); }

struct ConvLane {
    int32_t d[2][kConvMaxN];                       // d(c_i) of the transition from predecessor c; 0 from n on
};
CONV_HD ConvLane conv_lane(const uint32_t *gen, uint32_t n, int K, uint32_t hp) {
    ConvLane r;
    for (uint32_t c = 0; c < 2; ++c)
        for (uint32_t i = 0; i < kConvMaxN; ++i) r.d[c][i] = i < n ? (conv_code_bit(gen[i], K, conv_pred(hp, c, K), hp & 1) ? 1 : -1) : 0;
    return r;
}

// the metric a window's state starts with
CONV_HD int32_t conv_start(bool from_zero, uint32_t h, uint32_t init_state) { return from_zero && h != init_state ? kConvBarred : 0; }

// add-compare-select over N values: m0, m1 the metrics of the predecessors c = 0, c = 1.  The larger candidate survives; a
// tie goes to c = 0.
template <int N>
CONV_HD int32_t conv_acs(const ConvLane &r, const int16_t *v, int32_t m0, int32_t m1, uint32_t &c) {
    int32_t c0 = m0, c1 = m1;
    for (int i = 0; i < N; ++i) {
        c0 += (int32_t)v[i] * r.d[0][i];
        c1 += (int32_t)v[i] * r.d[1][i];
    }
    c = c1 > c0;
    return c ? c1 : c0;
}

// the end state: (ma, ia) is kept against (mb, ib) when it is larger, or equal at the lower index
CONV_HD bool conv_keeps(int32_t ma, uint32_t ia, int32_t mb, uint32_t ib) { return ma > mb || (ma == mb && ia < ib); }

// one step of the traceback: the path is in state s behind the step whose survivor word is `word` (the window's NS bits start
// at bit `base`); `bit` is that step's decision, the result the state behind the step before it
CONV_HD uint32_t conv_back(uint64_t word, uint32_t base, uint32_t s, int K, uint32_t &bit) {
    bit = s & 1;
    return conv_pred(s, (uint32_t)(word >> (base + s)) & 1u, K);
}

// ---- the encoder ---------------------------------------------------------------------------------------------------------------
// input bit of the step k counted from the call's first: from the packed bits, or, in front of them, from the state word
CONV_HD uint32_t conv_in_bit(const uint64_t *bits, uint32_t state, int64_t k) {
    if (k < 0) return -k <= 32 ? state >> (-k - 1) & 1u : 0u;
    return (uint32_t)(bits[k >> 6] >> (k & 63)) & 1u;
}

// the window of step k read oldest bit first: bit m = the input bit K-1-m steps back, so coded bit i is parity(w & gen[i])
CONV_HD uint32_t conv_in_window(const uint64_t *bits, uint32_t state, int64_t k, int K) {
    uint32_t w = 0;
    for (int m = 0; m < K; ++m) w |= conv_in_bit(bits, state, k - (K - 1) + m) << m;
    return w;
}

CONV_HD uint32_t conv_parity(uint32_t v) {
    v ^= v >> 4;
    v ^= v >> 2;
    v ^= v >> 1;
    return v & 1;                                  // v < 2^8
}

}  // namespace bbb
