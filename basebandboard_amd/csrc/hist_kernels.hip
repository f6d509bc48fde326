// hist_kernels.hip -- the histogram of the CLTGRNG sample stream (include/bbb.h, bbb_awgn_hist).
//
// Reference semantics: the counting half of software/clt-grng/clt-grng-evaluate.py:18-50 -- bin (x + k/2) of the delivered,
// truncated sample x -- over a range of the stream instead of 100 000 draws.
//
// Three kernels:
//  - hist_planes_kernel, the "histogram mover": a guest beside awgn256_planes_kernel, in unplane_kernel's place.  It fetches the 8
//    count planes of a unit (source wave, 8 of its lanes, 128 steps: 32 KiB, 32 768 samples) from the staging slot by LDS-DMA
//    and unpacks them with the reader every mover of the staged stream uses (stage_common.hpp: the unit, its raw image, the
//    order of the units), turns them into bytes (planes8_to_bytes) and BINS the bytes where the byte mover transposes and
//    stores them: nothing is written per sample;
//  - hist_samples_kernel: the same binning over int8 / int16 samples in memory, for every generator the planes form does not
//    exist for (k = 16 .. 128, 512, table-driven matrices) and for short ranges.  Correct, not fast;
//  - hist_reduce_kernel: hist[b] += the blocks' partials, in u64.  No global atomics.
// The block's histogram is u32 [bins][64 lanes] in LDS, as the eye's (eye_kernels.hip): a lane only ever touches its own column,
// the bank of word b * 64 + lane is the lane (MI355X_MICROARCH.md, LDS), so a ds_add_u32 of a wave is free of bank conflicts
// whatever the 64 bins are -- and two thirds of all samples fall into 16 of them.  Four waves share the columns: the add is atomic.
// A launch counts at most 2^31 samples, less than a u32 holds (the launch functions refuse more; bbb_awgn_hist sends at most
// 2^30 to the mover and 2^26 to the plain kernel), so every partial count is exact.
#include "bbb_common.hpp"
#include "bitslice_util.hpp"
#include "stage_common.hpp"

#include <algorithm>
#include <mutex>

namespace bbb {

typedef uint32_t hist_u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned kHistLanes = 64;
constexpr unsigned kHistRaw = kStageUnitBytes;                            // one unit's count planes
constexpr unsigned kHistTable = 256 * kHistLanes * 4;                     // 64 KiB: the block's histogram, at the start of the LDS
constexpr unsigned kHistPlanesLds = kHistTable + 2 * kHistRaw;            // 128 KiB of the CU's 160
constexpr int kHistSampleThreads = 1024;

// bin `bin` of a block's table: the sum over the 64 lane columns, read ROTATED by the bin (thread t starts at column t mod 64):
// the 64 threads of a wave then read 64 different banks at every step
__device__ __forceinline__ uint32_t hist_fold(const uint32_t *H, unsigned bin) {
    uint32_t sum = 0;
    for (unsigned l = 0; l < kHistLanes; l++) sum += H[bin * kHistLanes + ((l + bin) & (kHistLanes - 1))];
    return sum;
}

__global__ void __launch_bounds__(256, 7)      // <= 72 registers: a wave of this kernel must fit beside the sample kernel's
hist_planes_kernel(const hist_u32x4 *__restrict stage, unsigned long long nsamples, unsigned L, StageGeom ge, uint32_t *__restrict scratch) {
    // (dynamic, as unplane_kernel's: a static array of this size makes hipcc declare a register count no guest can have)
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    typedef __attribute__((address_space(3))) void *lds_void_ptr;
    const unsigned tid = threadIdx.x, lane = tid & 63;
    const unsigned wv = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    uint32_t *const H = lds;                                              // [256 bins][64 lanes]
    uint32_t *const raw0 = lds + kHistTable / 4;                          // [2][c = 2 s + half][quad-step][lane8][16 B]
    {
        hist_u32x4 *h4 = reinterpret_cast<hist_u32x4 *>(H);
        for (unsigned i = tid; i < kHistTable / 16; i += 256) h4[i] = hist_u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    const unsigned l8 = tid & 7, qs = tid >> 3;                           // lane of eight and quad-step this thread bins
    const uint32_t hbase = (uint32_t)(uintptr_t)(lds_void_ptr)H;         // LDS address of the table
    const uint32_t column = lane * 4u;                                    // byte offset of this lane's column in a bin's row
    StagePos cur;
    const unsigned n_it = stage_block_units(ge, blockIdx.x, &cur);
    StagePos nxt = cur;
    stage_advance(nxt, ge);
    unsigned buf = 0;
    if (n_it) stage_dma_unit(stage, ge, cur, L, raw0, wv, lane);
    for (unsigned it = 0; it < n_it; it++, buf ^= 1) {
        const bool more = it + 1 < n_it;
        if (more) stage_dma_unit(stage, ge, nxt, L, raw0 + (buf ^ 1) * (kHistRaw / 4), wv, lane);
        // this unit's DMA has landed: the only vector-memory operations of this kernel are its DMA, 8 per unit and wave, in order
        if (more) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // ---- bin: the samples of steps 4 qs .. 4 qs + 3 of the 32 generators of lane q8 * 8 + l8
        {
            uint32_t Z[4][8];
            stage_unpack<true>(raw0 + buf * (kHistRaw / 4), tid, Z);      // (the staged plane 7 is that of the int8: bin = x + 128)
#pragma unroll
            for (unsigned s = 0; s < 4; s++) planes8_to_bytes(Z[s]);      // Z[s][i] byte q = the bin of generator j = 8 q + i at step 4 qs + s
            // stream position of generator j = 0 of this lane at the thread's first step; generator j is 64 L further each
            const unsigned step = cur.rg * 128 + 4 * qs;
            const unsigned long long span = 64ull * L;
            const unsigned long long off0 = (((unsigned long long)ge.w_lo + cur.w) * kStageWaveGens + cur.q8 * 8 + l8) * L + step;
            // byte address of (bin, this lane's column) in ONE V_PERM_B32: byte 0 = the column (4 lane < 256), byte 1 = the bin
#define BBB_HIST_ADD(WORD, Q) \
    asm volatile("ds_add_u32 %0, %1" ::"v"(hbase + __builtin_amdgcn_perm(column, (WORD), 0x0c0c0004u | ((Q) << 8))), "v"(1u) : "memory")
            if (step + 3 < L && off0 + 3 + 31 * span < nsamples) {
                // every sample of the thread exists (all but the units at the end of the range and of a segment)
#pragma unroll
                for (unsigned s = 0; s < 4; s++) {
#pragma unroll
                    for (unsigned i = 0; i < 8; i++) {
                        BBB_HIST_ADD(Z[s][i], 0u); BBB_HIST_ADD(Z[s][i], 1u); BBB_HIST_ADD(Z[s][i], 2u); BBB_HIST_ADD(Z[s][i], 3u);
                    }
                }
            } else {
#pragma unroll
                for (unsigned s = 0; s < 4; s++) {
                    // the generators j < nj of this lane have a sample at step + s inside [0, nsamples)
                    const unsigned long long o = off0 + s;
                    unsigned nj = 0;
                    if (step + s < L && o < nsamples) {
                        const unsigned long long m = (nsamples - o - 1) / span + 1;
                        nj = m < 32 ? (unsigned)m : 32u;
                    }
#pragma unroll
                    for (unsigned i = 0; i < 8; i++) {
                        if (i < nj) BBB_HIST_ADD(Z[s][i], 0u);
                        if (i + 8 < nj) BBB_HIST_ADD(Z[s][i], 1u);
                        if (i + 16 < nj) BBB_HIST_ADD(Z[s][i], 2u);
                        if (i + 24 < nj) BBB_HIST_ADD(Z[s][i], 3u);
                    }
                }
            }
#undef BBB_HIST_ADD
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();           // raw[buf] is free for the unit after next
        cur = nxt;
        stage_advance(nxt, ge);
    }
    __syncthreads();
    scratch[(size_t)blockIdx.x * 256 + tid] = hist_fold(H, tid);
}

// bin (x + nbins / 2) mod nbins of every sample; 16-byte loads over the body, the ragged end by single threads of block 0.
// x is 16-byte aligned (the caller's own buffer)
template <typename T>
__global__ void __launch_bounds__(kHistSampleThreads)
hist_samples_kernel(const T *__restrict x, unsigned long long nsamples, unsigned nbins, uint32_t *__restrict scratch) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *const H = lds;                                              // [nbins][64 lanes]
    for (unsigned i = threadIdx.x; i < nbins * kHistLanes; i += kHistSampleThreads) H[i] = 0u;
    __syncthreads();
    constexpr unsigned PER = 16 / sizeof(T);                              // samples per 16-byte load
    const unsigned lane = threadIdx.x & 63, half = nbins >> 1, mask = nbins - 1;
    const unsigned long long ngroups = nsamples / PER;
    const hist_u32x4 *xv = reinterpret_cast<const hist_u32x4 *>(x);
    const unsigned long long stride = (unsigned long long)gridDim.x * kHistSampleThreads;
    for (unsigned long long g = (unsigned long long)blockIdx.x * kHistSampleThreads + threadIdx.x; g < ngroups; g += stride) {
        const hist_u32x4 v = xv[g];
#pragma unroll
        for (unsigned e = 0; e < PER; e++) {
            int s;
            if (sizeof(T) == 1) s = (int)(int8_t)((v[e >> 2] >> (8 * (e & 3))) & 0xffu);
            else s = (int)(int16_t)((v[e >> 1] >> (16 * (e & 1))) & 0xffffu);
            atomicAdd(&H[(((unsigned)s + half) & mask) * kHistLanes + lane], 1u);
        }
    }
    if (blockIdx.x == 0) {
        const unsigned long long i = ngroups * PER + threadIdx.x;
        if (threadIdx.x < PER && i < nsamples) atomicAdd(&H[(((unsigned)(int)x[i] + half) & mask) * kHistLanes + lane], 1u);
    }
    __syncthreads();
    for (unsigned bin = threadIdx.x; bin < nbins; bin += kHistSampleThreads) scratch[(size_t)blockIdx.x * nbins + bin] = hist_fold(H, bin);
}

// hist[t] += bin t of the partials
__global__ void __launch_bounds__(256)
hist_reduce_kernel(const uint32_t *__restrict scratch, unsigned used, unsigned nbins, unsigned long long *__restrict hist) {
    const unsigned t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nbins) return;
    unsigned long long sum = 0;
    for (unsigned b = 0; b < used; b++) sum += scratch[(size_t)b * nbins + t];
    hist[t] += sum;
}

int hist_grid_blocks() {
    int dev = 0, cus = 0;
    BBB_HIP(hipGetDevice(&dev));
    BBB_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    return std::max(cus, 1);                   // one block per CU: the table takes 64 KiB (k = 256) or 128 KiB (k = 512) of its LDS
}

// both kernels take more dynamic LDS than a kernel may have unasked
static int hist_lds_attributes() {
    static std::mutex mu;
    static bool attr_set[64] = {false};
    int dev = 0;
    BBB_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(mu);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        const int most = (int)(kHistMaxBins * kHistLanes * 4);
        BBB_HIP(hipFuncSetAttribute((const void *)hist_planes_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kHistPlanesLds));
        BBB_HIP(hipFuncSetAttribute((const void *)hist_samples_kernel<int8_t>, hipFuncAttributeMaxDynamicSharedMemorySize, most));
        BBB_HIP(hipFuncSetAttribute((const void *)hist_samples_kernel<int16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, most));
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    return BBB_OK;
}

int hist_planes_launch(const void *stage, uint64_t nsamples, unsigned L, unsigned nlanes, uint32_t *scratch, int blocks, unsigned *used,
                       hipStream_t st) {
    if (nsamples == 0 || nsamples > (1ull << 31)) return fail(BBB_EINVAL, "a histogram launch counts 1 .. 2^31 samples");
    if (L == 0 || blocks < 1) return fail(BBB_EINVAL, "bad histogram launch");
    // (the planes form exists for k = 256 only: a block's partial is 256 counts, and `scratch` holds blocks x 256 of them)
    StageGeom ge;      // the window [0, nsamples)
    const unsigned nb = stage_geom(0, nsamples, L, nlanes, (uint64_t)blocks, &ge);
    if (!nb) return fail(BBB_EINVAL, "staged range out of the histogram mover's reach");
    int rc = hist_lds_attributes();
    if (rc) return rc;
    hipLaunchKernelGGL(hist_planes_kernel, dim3(nb), dim3(256), kHistPlanesLds, st, (const hist_u32x4 *)stage, (unsigned long long)nsamples, L, ge,
                       scratch);
    BBB_HIP(hipGetLastError());
    *used = nb;
    return BBB_OK;
}

int hist_samples_launch(const void *samples, int elem, uint64_t nsamples, unsigned nbins, uint32_t *scratch, int blocks, unsigned *used,
                        hipStream_t st) {
    if (nsamples == 0 || nsamples > (1ull << 31)) return fail(BBB_EINVAL, "a histogram launch counts 1 .. 2^31 samples");
    if (nbins < 2 || nbins > kHistMaxBins || (nbins & (nbins - 1)) || blocks < 1 || ((uintptr_t)samples & 15) || (elem != 1 && elem != 2))
        return fail(BBB_EINVAL, "bad histogram launch");
    int rc = hist_lds_attributes();
    if (rc) return rc;
    // at least 16 loads per thread before another block is worth its table
    const uint64_t want = (nsamples + (uint64_t)kHistSampleThreads * 256 - 1) / ((uint64_t)kHistSampleThreads * 256);
    const unsigned nb = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)blocks));
    const size_t smem = (size_t)nbins * kHistLanes * 4;
    if (elem == 1)
        hipLaunchKernelGGL(hist_samples_kernel<int8_t>, dim3(nb), dim3(kHistSampleThreads), smem, st, (const int8_t *)samples,
                           (unsigned long long)nsamples, nbins, scratch);
    else
        hipLaunchKernelGGL(hist_samples_kernel<int16_t>, dim3(nb), dim3(kHistSampleThreads), smem, st, (const int16_t *)samples,
                           (unsigned long long)nsamples, nbins, scratch);
    BBB_HIP(hipGetLastError());
    *used = nb;
    return BBB_OK;
}

int hist_reduce_launch(const uint32_t *scratch, unsigned used, unsigned nbins, uint64_t *hist, hipStream_t st) {
    hipLaunchKernelGGL(hist_reduce_kernel, dim3((nbins + 255) / 256), dim3(256), 0, st, scratch, used, nbins,
                       reinterpret_cast<unsigned long long *>(hist));
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
