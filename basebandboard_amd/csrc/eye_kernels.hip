// eye_kernels.hip -- eye histogram and bathtub counts of int16 samples (include/bbb.h, "eye diagram and bathtub").
//
// Reference semantics: the DSO of gateware/bbb/dso.py:12-72 (256 rows x 64 columns, row = 127 - sample, column = position
// after a line trigger), counted instead of lit; the bathtub decides data bit m from sample 8m + 45 + p at phase p.
//
// One accumulate kernel serves the capture side (bbb_eye_accumulate_i16) and the transmitter side (bbb_tx_eye_run).  What a
// block keeps and how it hands it on is eye_common.hpp's, shared with the filtered link (link_kernels.hip):
//  - the histogram in LDS, [256 rows][64 lane-columns] u32, folded to ncols at the flush.  A thread reads 8 consecutive
//    samples with one 16-byte load (group g of the body, g = lane mod 8 within 8 lanes) and adds them with eye_add8, whose
//    rotation keeps the 32 lanes of a group on 32 distinct banks;
//  - the flush (eye_flush) writes the block's folded partial with plain stores to a scratch slab ([blocks][256 ncols + 8]
//    u32); eye_reduce_launch adds the slab into the u64 outputs (no global atomics: 256 blocks x 16 Ki bins would be 4 M of
//    them);
//  - bathtub errors are counted in registers per sample slot j (slot j of every group has the same phase), reduced per wave,
//    then per block in LDS (eye_fold_errors); the number of bits decided per phase is exact arithmetic on the range, added by
//    the host.
// Samples per launch are below 2^31 (the host cuts longer ranges), so every u32 count of a block is exact.
#include "bbb_common.hpp"
#include "eye_common.hpp"

#include <algorithm>

namespace bbb {

constexpr int kEyeThreads = 1024;
constexpr int kEyeUnroll = 4;                          // 16-byte loads in flight per thread
constexpr uint64_t kEyeLaunchMax = 1ull << 31;         // samples per launch

// data bit m, or -1 when it does not count (m < 0, or outside the bits supplied)
__device__ __forceinline__ int eye_bit(const EyeLaunch &a, long long m) {
    if (m < 0) return -1;
    if (a.pulser) return (m & 255) == 0;                            // Pulser: counter == 0 (tx.py:28-30)
    if (m < a.bit0) return -1;
    const unsigned long long rel = (unsigned long long)(m - a.bit0);
    if (rel >= a.nbits) return -1;
    return (int)((a.bits[rel >> 6] >> (rel & 63)) & 1ull);
}

// samples [0, head) and [head + 8 ngroups, nsamples) of the launch are the "extras" (at most 7 + 7): the body's 16-byte loads
// need x + head to be 16-byte aligned.
template <bool HIST, bool TUB>
__global__ void __launch_bounds__(kEyeThreads)
eye_accumulate_kernel(EyeLaunch a, const int16_t *__restrict x, unsigned head, unsigned long long ngroups, unsigned long long nsamples,
                      unsigned long long first, uint32_t *__restrict scratch) {
    __shared__ uint32_t H[HIST ? kEyeRows * kEyeLanes : 1];
    __shared__ uint32_t E[8];
    eye_zero<HIST>(H, E, threadIdx.x, kEyeThreads);
    __syncthreads();

    const unsigned lane = threadIdx.x & 63;
    const unsigned rot = (lane >> 2) & 7;
    const unsigned long long s0 = first + head;                              // sample number of the body's first sample
    const unsigned cb = (unsigned)((s0 - a.col_origin) & 63) + 8u * (lane & 7);   // lane-column of this lane's slot 0 (g = lane mod 8)
    const long long r0 = (long long)s0 - BBB_TX_BIT_SAMPLE0;
    const long long F = r0 >> 3;                                             // floor: bit of slot 0 of group 0
    const unsigned d = (unsigned)(r0 & 7);                                   // its phase; slots j >= 8 - d belong to bit F + g + 1
    uint32_t err[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    const eye_u32x4 *xv = reinterpret_cast<const eye_u32x4 *>(x + head);
    const unsigned long long stride = (unsigned long long)gridDim.x * kEyeThreads;
    for (unsigned long long g0 = (unsigned long long)blockIdx.x * kEyeThreads + threadIdx.x; g0 < ngroups; g0 += stride * kEyeUnroll) {
        eye_u32x4 v[kEyeUnroll];
#pragma unroll
        for (int u = 0; u < kEyeUnroll; u++) {
            const unsigned long long g = g0 + u * stride;
            if (g < ngroups) v[u] = xv[g];
        }
#pragma unroll
        for (int u = 0; u < kEyeUnroll; u++) {
            const unsigned long long g = g0 + u * stride;
            if (g >= ngroups) break;
            int s[8];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                s[2 * i] = (int)(int16_t)(v[u][i] & 0xffffu);
                s[2 * i + 1] = (int)v[u][i] >> 16;
            }
            if constexpr (TUB) {
                const long long m = F + (long long)g;
                const int b0 = eye_bit(a, m), b1 = eye_bit(a, m + 1);
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int b = (unsigned)j < 8u - d ? b0 : b1;
                    err[j] += (b >= 0) & (eye_decide(s[j], a.threshold, a.strict) != (unsigned)b);
                }
            }
            if constexpr (HIST) {
                unsigned A[8];
#pragma unroll
                for (int r = 0; r < 8; r++) A[r] = eye_row(s[r], a.shift) * kEyeLanes + ((cb + r) & 63);
                eye_add8<false>(H, A, rot);
            }
        }
    }

    // the extras, one sample per thread of block 0
    if (blockIdx.x == 0 && threadIdx.x < 16) {
        const unsigned long long tail0 = head + 8 * ngroups;
        const unsigned t = threadIdx.x;
        const unsigned long long i = t < head ? t : tail0 + (t - head);
        if (i < nsamples) {
            const unsigned long long n = first + i;
            const int xs = x[i];
            if constexpr (HIST) atomicAdd(&H[eye_row(xs, a.shift) * kEyeLanes + (unsigned)((n - a.col_origin) & 63)], 1u);
            if constexpr (TUB) {
                const long long rn = (long long)n - BBB_TX_BIT_SAMPLE0;
                const int b = eye_bit(a, rn >> 3);
                if (b >= 0 && eye_decide(xs, a.threshold, a.strict) != (unsigned)b) atomicAdd(&E[rn & 7], 1u);
            }
        }
    }
    if constexpr (TUB) eye_fold_errors(E, err, d, lane);
    __syncthreads();
    eye_flush<HIST, TUB>(H, E, scratch, kEyeRows * a.ncols, a.ncols, threadIdx.x, kEyeThreads);
}

int eye_grid_blocks(uint64_t nsamples) {
    int dev = 0, cus = 0;
    BBB_HIP(hipGetDevice(&dev));
    BBB_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const uint64_t per_launch = std::min<uint64_t>(nsamples, kEyeLaunchMax);
    // one block per CU (64 KiB of LDS, 16 waves); fewer for short launches: at least 16 groups of 8 samples per thread
    const uint64_t want = (per_launch + (uint64_t)kEyeThreads * 128 - 1) / ((uint64_t)kEyeThreads * 128);
    return (int)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)std::max(cus, 1)));
}

int eye_accumulate_launch(const EyeLaunch &a, const int16_t *samples, uint64_t nsamples, uint64_t first_sample, uint32_t *scratch,
                          int blocks, uint64_t *hist, uint64_t *bathtub, hipStream_t st) {
    const unsigned nbins = kEyeRows * a.ncols;
    for (uint64_t off = 0; off < nsamples;) {
        const uint64_t n = std::min(nsamples - off, kEyeLaunchMax);
        const int16_t *x = samples + off;
        const unsigned head = (unsigned)std::min<uint64_t>(((16 - ((uintptr_t)x & 15)) & 15) / 2, n);
        const uint64_t ngroups = (n - head) / 8;
        const uint64_t want = (ngroups + kEyeThreads - 1) / kEyeThreads;
        const unsigned nb = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)blocks, want));
        const uint64_t first = first_sample + off;
        if (a.want_hist && a.want_tub)
            eye_accumulate_kernel<true, true><<<nb, kEyeThreads, 0, st>>>(a, x, head, ngroups, n, first, scratch);
        else if (a.want_hist)
            eye_accumulate_kernel<true, false><<<nb, kEyeThreads, 0, st>>>(a, x, head, ngroups, n, first, scratch);
        else
            eye_accumulate_kernel<false, true><<<nb, kEyeThreads, 0, st>>>(a, x, head, ngroups, n, first, scratch);
        BBB_HIP(hipGetLastError());
        const int rc = eye_reduce_launch(scratch, nb, nbins, a.want_hist ? hist : nullptr, a.want_tub ? bathtub : nullptr, first, n, st);
        if (rc) return rc;
        off += n;
    }
    return BBB_OK;
}

}  // namespace bbb
