// eye_common.hpp -- what the eye kernels (eye_kernels.hip) and the filtered link (link_kernels.hip) share: the row rule, the
// layout of a block's LDS histogram, the bits a range decides per phase, and the kernel that folds the per-block slab into
// the u64 outputs.
#pragma once

#include "bbb_common.hpp"

namespace bbb {

constexpr int kEyeRows = 256, kEyeLanes = 64;          // a block's histogram: [256 rows][64 lane-columns] u32 in LDS

struct EyeTubBits { unsigned long long v[8]; };

__device__ __forceinline__ unsigned eye_row(int x, unsigned shift) {
    int v = x >> shift;
    v = v < -128 ? -128 : (v > 127 ? 127 : v);
    return (unsigned)(127 - v);
}

// outputs += the slab ([blocks][nbins + 8] u32): thread t < nbins sums bin t over the blocks, t = nbins + p the errors of phase p
static __global__ void __launch_bounds__(256)
eye_reduce_kernel(const uint32_t *__restrict scratch, unsigned blocks, unsigned nbins, unsigned long long *__restrict hist,
                  unsigned long long *__restrict tub, EyeTubBits bits) {
    const unsigned t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nbins + 8) return;
    const bool is_tub = t >= nbins;
    if (is_tub ? !tub : !hist) return;
    unsigned long long sum = 0;
    for (unsigned b = 0; b < blocks; b++) sum += scratch[(unsigned long long)b * (nbins + 8) + t];
    if (!is_tub) {
        hist[t] += sum;
    } else {
        const unsigned p = t - nbins;
        tub[2 * p] += bits.v[p];
        tub[2 * p + 1] += sum;
    }
}

// the bits a range of samples decides at each phase: m >= 0 with 8m + 45 + p in [first, first + n)
static inline void eye_tub_bits(uint64_t first, uint64_t n, EyeTubBits *b) {
    const uint64_t last = first + n - 1;
    for (int p = 0; p < 8; p++) {
        const uint64_t s = BBB_TX_BIT_SAMPLE0 + p;
        b->v[p] = 0;
        if (last < s) continue;
        const uint64_t lo = first <= s ? 0 : (first - s + 7) / 8, hi = (last - s) / 8;
        b->v[p] = hi >= lo ? hi - lo + 1 : 0;
    }
}

}  // namespace bbb
