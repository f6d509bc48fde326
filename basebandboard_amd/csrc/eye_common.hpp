// eye_common.hpp -- what the eye kernels (eye_kernels.hip) and the filtered link (link_kernels.hip) share: the row and the
// decision rule, a block's LDS histogram (zeroing, the bank-spreading add, the fold at the flush), the block's bathtub
// errors, and the kernel that folds the per-block slab into the u64 outputs with the host function that launches it.
//
// The histogram is u32 counts laid out [256 rows][64 LANE-COLUMNS]: lane-column lc holds the samples with
// (n - col_origin) mod 64 = lc and is folded to column lc mod ncols at the flush.  The bank of a b32 LDS access is
// (a/4) mod 32 in lane groups of 32 (MI355X_MICROARCH.md, LDS), and row * 64 is a multiple of 32, so an instruction whose 32
// lanes touch 32 distinct lane-columns mod 32 is free of conflicts whatever the rows are.
#pragma once

#include "bbb_common.hpp"
#include "tx_common.hpp"

namespace bbb {

constexpr int kEyeRows = 256, kEyeLanes = 64;          // a block's histogram: [256 rows][64 lane-columns] u32 in LDS
typedef uint32_t eye_u32x4 __attribute__((ext_vector_type(4)));

struct EyeTubBits { unsigned long long v[8]; };

__device__ __forceinline__ unsigned eye_row(int x, unsigned shift) {
    int v = x >> shift;
    v = v < -128 ? -128 : (v > 127 ? 127 : v);
    return (unsigned)(127 - v);
}

__device__ __forceinline__ unsigned eye_decide(int x, int thr, int strict) { return strict ? (x > thr) : (x >= thr); }

// a block of nthreads zeroes its histogram H (HIST) and its errors E; the caller's barrier follows
template <bool HIST>
__device__ __forceinline__ void eye_zero(uint32_t *H, uint32_t *E, int t, int nthreads) {
    if constexpr (HIST) {
        eye_u32x4 *h4 = reinterpret_cast<eye_u32x4 *>(H);
        for (int i = t; i < kEyeRows * kEyeLanes / 4; i += nthreads) h4[i] = eye_u32x4{0u, 0u, 0u, 0u};
    }
    if (t < 8) E[t] = 0;
}

// H[A[j]] += 1 for a lane's 8 consecutive samples, slot j on lane-column cb + 8 (lane mod 8) + j.  Taken in slot order,
// lanes l, l+4, ..., l+28 would all sit on one bank at step j.  Each lane instead takes its 8 addresses ROTATED by
// rot = (lane >> 2) & 7 (three select stages): at step j it adds slot (j + rot) mod 8, and the 32 lanes of a group cover 32
// distinct banks.  MASKED: an address of ~0u is a sample that does not count; without it there is no compare per sample.
template <bool MASKED>
__device__ __forceinline__ void eye_add8(uint32_t *H, unsigned (&A)[8], unsigned rot) {
#pragma unroll
    for (unsigned sh = 1; sh < 8; sh <<= 1) {                    // A[j] <- A[(j + rot) mod 8]
        const bool on = rot & sh;
        unsigned B[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            // both read first: a choice between two loads can end as one load at a run-time index, which on an array
            // kept in registers is seven compares and selects
            const unsigned up = A[(j + sh) & 7], own = A[j];
            B[j] = on ? up : own;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) A[j] = B[j];
    }
#pragma unroll
    for (int j = 0; j < 8; j++)
        if (!MASKED || A[j] != ~0u) atomicAdd(&H[A[j]], 1u);
}

// the errors a thread counted per sample slot (slot j of every thread has phase (d + j) mod 8): per wave, then per block in E
__device__ __forceinline__ void eye_fold_errors(uint32_t *E, const uint32_t (&err)[8], unsigned d, unsigned lane) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t e = err[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
        if (lane == 0 && e) atomicAdd(&E[(d + j) & 7], e);
    }
}

// flush, after a barrier: fold the 64 lane-columns to ncols and store the block's partial ([nbins + 8] u32 of the slab) with
// plain stores
template <bool HIST, bool TUB>
__device__ __forceinline__ void eye_flush(const uint32_t *H, const uint32_t *E, uint32_t *__restrict scratch, unsigned nbins,
                                          unsigned ncols, unsigned t, unsigned nthreads) {
    uint32_t *out = scratch + (unsigned long long)blockIdx.x * (nbins + 8);
    if constexpr (HIST) {
        const unsigned lg = 31 - __builtin_clz(ncols), fold = kEyeLanes >> lg;
        for (unsigned bin = t; bin < nbins; bin += nthreads) {
            const unsigned row = bin >> lg, col = bin & (ncols - 1);
            uint32_t sum = 0;
            for (unsigned k = 0; k < fold; k++) sum += H[row * kEyeLanes + col + (k << lg)];
            out[bin] = sum;
        }
    }
    if (TUB && t < 8) out[nbins + t] = E[t];
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

// hist and tub (either may be nullptr) += the slab of a launch over samples [first, first + n), with the bits they decide
static inline int eye_reduce_launch(const uint32_t *scratch, unsigned blocks, unsigned nbins, uint64_t *hist, uint64_t *tub,
                                    uint64_t first, uint64_t n, hipStream_t st) {
    EyeTubBits tb;
    tx_phase_bits(first, n, tb.v);
    eye_reduce_kernel<<<(nbins + 8 + 255) / 256, 256, 0, st>>>(scratch, blocks, nbins, reinterpret_cast<unsigned long long *>(hist),
                                                               reinterpret_cast<unsigned long long *>(tub), tb);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
