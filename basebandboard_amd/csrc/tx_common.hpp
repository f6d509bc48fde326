// tx_common.hpp -- device helpers shared by the transmitter's kernels (tx_kernels.hip) and the BER sweep over its
// settings (txsweep_kernels.hip): the coefficient set as a kernel argument, the 12-bit wrap and the data-bit window.
#pragma once

#include "bbb_common.hpp"

namespace bbb {

struct Coeffs64 { int16_t c[64]; };

__device__ __forceinline__ int wrap12_dev(int v) { return (int)((unsigned)v << 20) >> 20; }

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
