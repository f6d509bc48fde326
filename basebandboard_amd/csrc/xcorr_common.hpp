// xcorr_common.hpp -- the per-thread core of the data-to-waveform correlation (include/bbb.h, bbb_xcorr_accumulate_i16),
// for the device and for the host: tests/xcorr_host.cpp runs the same code lane by lane against the definition.
//
// With u = n - origin, q = floor(u / spb) and r = u mod spb, sample n adds s[q - j'] * x[n] to lag spb * j' + r for every
// j' with q - j' >= 0.  A lane owns one residue r and XT consecutive lag groups j' = jbase + j (j < XT <= 32), and walks
// consecutive q.  With p = q - jbase it keeps the window W, bit j = data bit p - j (0 where there is none), moved on by one
// bit per step, and XT int32 accumulators.  Two step forms:
//   masked   acc[j] += bit_j ? x : 0, total += x; the signed sum 2 acc[j] - total is formed at the flush.  Every window bit
//            must be a real bit: p >= XT - 1.
//   signed   acc[j] += j <= p ? (bit_j ? x : -x) : 0: the first bits of the stream, where lag groups reach below bit 0.
// A lane flushes before it changes form.  |x| <= 32768 = 2^15, so acc and total reach 2^31, one more than int32 holds, after
// 2^16 steps at the earliest; a lane flushes every kXcorrFlushSteps = 2^15 steps, where they are within 2^30.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define XCORR_HD __host__ __device__ __forceinline__
#else
#define XCORR_HD inline
#endif

namespace bbb {

constexpr int kXcorrThreads = 256;
constexpr int kXcorrSteps = 32;                        // steps of a lane per tile
constexpr int kXcorrTile = kXcorrThreads * kXcorrSteps;    // samples per tile
constexpr int kXcorrFlushSteps = 32768;                // 2^15 steps of at most 2^15 each: within 2^30 (int32 wraps after 2^16 steps)

// floor division and the matching remainder by a power of two 1 << sh
XCORR_HD long long xcorr_floor_div(long long v, unsigned sh) { return v >> sh; }
XCORR_HD unsigned xcorr_floor_mod(long long v, unsigned sh) { return (unsigned)(v & ((1ll << sh) - 1)); }

// The tile in LDS: sample k (k < kXcorrTile) of the tile lies in segment k / (kXcorrSteps spb); a segment is followed by
// spb unused halfwords.  Lane (c, s) = (tid mod spb, tid / spb) reads sample spb (kXcorrSteps s + t) + c at step t.
XCORR_HD unsigned xcorr_lds_index(unsigned k, unsigned spb_sh) {
    const unsigned seg_sh = 5 + spb_sh;
    return (((k >> seg_sh) * (kXcorrSteps + 1)) << spb_sh) + (k & ((1u << seg_sh) - 1));
}
XCORR_HD unsigned xcorr_lane_sample(unsigned tid, unsigned t, unsigned spb_sh) {
    const unsigned c = tid & ((1u << spb_sh) - 1), s = tid >> spb_sh;
    return ((kXcorrSteps * s + t) << spb_sh) + c;
}

// 32 data bits from bit number lo on (bit i of the result is data bit lo + i); bits outside [bit0, bit0 + 64 nwords) read 0.
// Whatever the packed words hold beyond the last supplied bit may come back: a caller's range check keeps such bits away
// from every term that counts.
XCORR_HD uint32_t xcorr_bits32(const unsigned long long *bits, long long bit0, long long nwords, long long lo) {
    const long long rel = lo - bit0;
    const long long w = rel >> 6;
    const unsigned sh = (unsigned)(rel & 63);
    const unsigned long long a = (w >= 0 && w < nwords) ? bits[w] : 0ull;
    const unsigned long long b = (w + 1 >= 0 && w + 1 < nwords) ? bits[w + 1] : 0ull;
    const unsigned long long v = sh ? (a >> sh) | (b << (64 - sh)) : a;
    return (uint32_t)v;
}

XCORR_HD uint32_t xcorr_brev32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(v);
#else
    v = (v >> 16) | (v << 16);
    v = ((v & 0xff00ff00u) >> 8) | ((v & 0x00ff00ffu) << 8);
    v = ((v & 0xf0f0f0f0u) >> 4) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v & 0xccccccccu) >> 2) | ((v & 0x33333333u) << 2);
    return ((v & 0xaaaaaaaau) >> 1) | ((v & 0x55555555u) << 1);
#endif
}

XCORR_HD int xcorr_mul24(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    return a * b;
#endif
}

template <int XT>
struct XcorrLane {
    int acc[XT];
    int total;
    int steps;                                         // since the last flush

    XCORR_HD void clear() {
#pragma unroll
        for (int j = 0; j < XT; j++) acc[j] = 0;
        total = 0;
        steps = 0;
    }
};

template <int XT>
XCORR_HD void xcorr_step_masked(XcorrLane<XT> &a, uint32_t W, int x) {
#pragma unroll
    for (int j = 0; j < XT; j++) a.acc[j] += xcorr_mul24((int)((W >> j) & 1u), x);
    a.total += x;
}

// p = q - jbase of this step (any sign): lag groups j > p reach below bit 0 and take nothing
template <int XT>
XCORR_HD void xcorr_step_signed(XcorrLane<XT> &a, uint32_t W, int x, long long p) {
#pragma unroll
    for (int j = 0; j < XT; j++) {
        const int v = ((W >> j) & 1u) ? x : -x;
        a.acc[j] += (long long)j <= p ? v : 0;
    }
}

// hands sink(j, value) the int64 sum of every lag group and clears the lane
template <int XT, class Sink>
XCORR_HD void xcorr_flush(XcorrLane<XT> &a, bool masked, Sink &&sink) {
#pragma unroll
    for (int j = 0; j < XT; j++) {
        const long long v = masked ? 2ll * a.acc[j] - (long long)a.total : (long long)a.acc[j];
        if (v) sink(j, v);
    }
    a.clear();
}

// One lane's share of one tile: kXcorrSteps samples x(0) .. x(kXcorrSteps - 1) at bit numbers q0, q0 + 1, ... (a sample
// that does not count -- outside the call's range, or below the origin -- must come as 0).  `masked_now` is the form the
// lane's accumulators are in and is updated; sink as in xcorr_flush.
template <int XT, class Sample, class Sink>
XCORR_HD void xcorr_lane_tile(XcorrLane<XT> &a, bool &masked_now, long long q0, unsigned jbase, const unsigned long long *bits,
                              long long bit0, long long nwords, Sample &&x, Sink &&sink) {
    const long long p0 = q0 - (long long)jbase;
    const bool masked = p0 >= XT - 1;
    if (masked != masked_now || a.steps + kXcorrSteps > kXcorrFlushSteps) xcorr_flush(a, masked_now, sink);
    masked_now = masked;
    // before the first step: bit j of W is data bit p0 - 1 - j; F holds the bits the steps shift in
    uint32_t W = xcorr_brev32(xcorr_bits32(bits, bit0, nwords, p0 - 32));
    uint32_t F = xcorr_bits32(bits, bit0, nwords, p0);
    if (masked) {
#pragma unroll 4
        for (int t = 0; t < kXcorrSteps; t++) {
            W = (W << 1) | (F & 1u);
            F >>= 1;
            xcorr_step_masked(a, W, x(t));
        }
    } else {
        // window bits that stand for bits below 0 hold whatever xcorr_bits32 gave: the step does not look at them
#pragma unroll 1
        for (int t = 0; t < kXcorrSteps; t++) {
            W = (W << 1) | (F & 1u);
            F >>= 1;
            xcorr_step_signed(a, W, x(t), p0 + t);
        }
    }
    a.steps += kXcorrSteps;
}

}  // namespace bbb
