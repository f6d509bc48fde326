// tx_common.hpp -- what the transmitter's kernels (tx_kernels.hip), the BER sweep over its settings (txsweep_kernels.hip),
// the eye (eye_common.hpp) and the filtered link (link_kernels.hip) share: the coefficient set as a kernel argument, the
// 12-bit wrap, one entry of the shaped-value table, the data-bit window and the bits a range decides per bathtub phase.
#pragma once

#include "bbb_common.hpp"

namespace bbb {

struct Coeffs64 { int16_t c[64]; };

__device__ __forceinline__ int wrap12_dev(int v) { return (int)((unsigned)v << 20) >> 20; }

// One entry of the shaped-value table: ROM idx contributes +c[8 idx + ph] when data bit M - idx is 1 (bit 7 - idx of q), else
// -c (bitshaper.py:52-58,:74); the 12-bit wrap of the sum is the adder tree's sample (:76-86).  Every table builder calls
// this and applies its own layout.
__device__ __forceinline__ int shaped_entry(const int16_t *coeffs, int ph, int q) {
    int sum = 0;
#pragma unroll
    for (int idx = 0; idx < 8; idx++) {
        const int c = coeffs[8 * idx + ph];
        sum += ((q >> (7 - idx)) & 1) ? c : -c;
    }
    return wrap12_dev(sum);
}

// the bits a range of samples decides at each bathtub phase: b[p] counts the m >= 0 with 8m + 45 + p in [first, first + n)
static inline void tx_phase_bits(uint64_t first, uint64_t n, unsigned long long *b) {
    const uint64_t last = first + n - 1;
    for (int p = 0; p < 8; p++) {
        const uint64_t s = BBB_TX_BIT_SAMPLE0 + p;
        b[p] = 0;
        if (last < s) continue;
        const uint64_t lo = first <= s ? 0 : (first - s + 7) / 8, hi = (last - s) / 8;
        b[p] = hi >= lo ? hi - lo + 1 : 0;
    }
}

// Q bit j = data bit M0-7+j, j = 0..9 (bits before the first one are 0: the reset shift register).
// `bits` holds data bits m0 .. m0+navail-1 and nothing else may be read: a window reaching past them
// (only bits that no sample of the request needs) takes the bit-by-bit path, which reads 0 there
__device__ __forceinline__ unsigned data_window10(const unsigned long long *__restrict bits, long long m0, unsigned long long navail,
                                                  int source, long long M0) {
    unsigned Q = 0;
    if (source == 0 && M0 - 7 >= m0 && (unsigned long long)(M0 - 7 - m0) + 10 <= navail) {
        const unsigned long long rel = (unsigned long long)(M0 - 7 - m0);
        const unsigned sh = (unsigned)(rel & 63);
        unsigned long long w = bits[rel >> 6] >> sh;
        if (sh > 54) w |= bits[(rel >> 6) + 1] << (64 - sh);
        Q = (unsigned)w & 0x3ffu;
    } else {
#pragma unroll 1
        for (int j = 0; j < 10; j++) {
            const long long m = M0 - 7 + j;
            unsigned b = 0;
            if (m >= 0) {
                if (source == 0) {
                    const unsigned long long rel = (unsigned long long)(m - m0);
                    if (m >= m0 && rel < navail) b = (unsigned)((bits[rel >> 6] >> (rel & 63)) & 1ull);
                } else {
                    b = (m & 255) == 0;                                  // Pulser: counter == 0 (tx.py:28-30)
                }
            }
            Q |= b << j;
        }
    }
    return Q;
}

}  // namespace bbb
