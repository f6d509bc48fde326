// txsweep_kernels.hip -- bit errors of the shaped link for many transmitter settings in one pass (include/bbb.h,
// "BER of the shaped link over many transmitter settings in one pass").
//
// Reference semantics: TX.x of gateware/bbb/tx.py:60-81, x = wrap12(bit_en * shaped + noise_en * wrap12(g * noise_var)),
// decided per phase as in the bathtub of eye_kernels.hip: data bit m from sample n = 8m + 45 + p, decision
// strict ? x > threshold : x >= threshold.
//
// The noise sample g(n) and the data bits are the same for every setting; only the arithmetic after them differs.  A launch
// serves up to 2 kSweepMaxPairs settings that share one coefficient set (bit_en = 0 is the all-zero set), so one table
// T[ph][q] of tx_waveform_kernel (wrap12 of the sum; q = bits M-7..M, M = floor((n-17)/8), ph = (n-17) mod 8) sits in LDS.
// A thread takes 16 int8 noise samples with one 16-byte load and one 10-bit data window (data_window10).  Everything of a
// sample fits 16 bits, so two settings share one lane operation (packed u16 / i16):
//  - the table holds y0 = 16 wrap12(sum) + 8 (mod 2^16).  For a setting, y = 16 g nv + y0 (mod 2^16) = 16 x + 8 exactly: the
//    16-bit wrap IS the 12-bit wrap of the sum, scaled by 16 (the inner wrap12(g nv) changes nothing: |g nv| <= 128 * 15).
//    16 x + 8 lies in [-32760, 32760].
//  - the decision is folded into the sign.  Let t = threshold (+1 when strict: x >= t), clamped to [-2048, 2048].
//    Data bit 1: error iff x < t iff y - 16 t < 0.  Data bit 0: error iff x >= t iff ~y - (-16 t) < 0, and
//    ~y = (-16 g) nv + ~y0: the lane negates g and complements the table value once per sample, not per setting.  Since
//    y = 16 x + 8 (and ~y = -16 x - 9), any bound within 7 of +-16 t gives the same signs: both bounds saturate to int16.
//    With every t = 0 the error is the sign of y itself: one v_pk_mad_u16, one shift and one add per two settings.
//  - slot j of every 8-aligned group of samples has the same bathtub phase (d + j) mod 8, so per setting the errors sit in
//    8 packed registers (two 16-bit counters each) -- no histogram.
// A block reduces per wave, writes its partial with plain stores to a scratch slab, and a small kernel folds the slab in
// u64 (no global atomics), adding the bits decided per phase, which the host knows exactly from the range (tx_phase_bits of
// tx_common.hpp, the eye's and the link's too).
// Every per-thread 16-bit counter stays below 2 * kSweepMaxIters * 64 < 2^16, and a launch covers < 2^31 samples.
#include "bbb_common.hpp"
#include "tx_common.hpp"

#include <algorithm>

namespace bbb {

constexpr int kSweepThreads = 256;
constexpr uint64_t kSweepMaxIters = 256;          // groups of 16 samples per thread and launch (the packed counters' bound)
constexpr uint64_t kSweepLaunchMax = 1ull << 31;  // samples per launch
typedef uint32_t sw_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long sw_u64x2 __attribute__((ext_vector_type(2)));
typedef unsigned short sw_u16x2 __attribute__((ext_vector_type(2)));
typedef short sw_i16x2 __attribute__((ext_vector_type(2)));

struct SweepPairs { uint32_t nv2[kSweepMaxPairs], t0[kSweepMaxPairs], t1[kSweepMaxPairs]; };
struct SweepOut { int32_t idx[2 * kSweepMaxPairs]; unsigned long long bits[8]; };

// the table of tx_waveform_kernel, as y0 = 16 T + 8 (mod 2^16); block t builds set t
__global__ void __launch_bounds__(256)
txsweep_table_kernel(const int16_t *__restrict coeffs, uint16_t *__restrict tables) {
    const int16_t *cf = coeffs + 64 * blockIdx.x;
    uint16_t *T = tables + 8 * 256 * blockIdx.x;
    for (int e = threadIdx.x; e < 8 * 256; e += blockDim.x)
        T[e] = (uint16_t)(((unsigned)shaped_entry(cf, e >> 8, e & 255) * 16u + 8u) & 0xffffu);
}

// the 16 samples of one thread's group: noise bytes nz, data window Q of bits M0-7 .. M0+2, sample e has (n - 17) mod 8 =
// (c0 + e) mod 8.  EDGE: only samples lo <= e < hi count.
template <int NP, bool THR, bool EDGE>
__device__ __forceinline__ void sweep_group(const SweepPairs &P, const uint16_t *T, unsigned long long nz0, unsigned long long nz1,
                                            unsigned Q, unsigned c0, unsigned lo, unsigned hi, uint32_t (&acc)[NP][8]) {
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const unsigned ce = c0 + (unsigned)e, ph = ce & 7u, qsh = ce >> 3;
        // the decided bit m = floor((n - 45) / 8) sits at window index M - m + 7 = qsh + (ph < 4 ? 3 : 4)
        const unsigned b = (Q >> (qsh + (ph < 4 ? 3u : 4u))) & 1u;
        const unsigned q = (Q >> qsh) & 255u;
        const int g = (int)(int8_t)((e < 8 ? nz0 : nz1) >> (8 * (e & 7)));
        const unsigned g16 = (unsigned)g << 4;
        const unsigned gb = (b ? g16 : 0u - g16) & 0xffffu;
        const uint32_t gb2 = gb | (gb << 16);
        const uint32_t y0 = T[ph * 256 + q];
        const uint32_t yb2 = (y0 | (y0 << 16)) ^ (b - 1u);        // ~y0 in both halves when the bit is 0
        uint32_t vm = 0x00010001u;
        if constexpr (EDGE) vm = ((unsigned)e >= lo && (unsigned)e < hi) ? 0x00010001u : 0u;
#pragma unroll
        for (int k = 0; k < NP; k++) {
            sw_u16x2 y = __builtin_bit_cast(sw_u16x2, gb2) * __builtin_bit_cast(sw_u16x2, P.nv2[k]) + __builtin_bit_cast(sw_u16x2, yb2);
            if constexpr (THR)
                y = __builtin_bit_cast(sw_u16x2, __builtin_elementwise_sub_sat(__builtin_bit_cast(sw_i16x2, y),
                                                                               __builtin_bit_cast(sw_i16x2, b ? P.t1[k] : P.t0[k])));
            uint32_t s = __builtin_bit_cast(uint32_t, y >> (unsigned short)15);
            if constexpr (EDGE) s &= vm;
            acc[k][e & 7] += s;                                      // two 16-bit counters, no carry between them
        }
    }
}

template <int NP, bool THR>
__global__ void __launch_bounds__(kSweepThreads)
txsweep_kernel(SweepPairs P, const uint16_t *__restrict tab, const int8_t *__restrict noise, const unsigned long long *__restrict bits,
               long long m0, unsigned long long navail, int source, unsigned long long first, unsigned long long nsamples,
               uint32_t *__restrict scratch) {
    __shared__ __attribute__((aligned(16))) uint16_t T[8 * 256];
    __shared__ uint32_t W[kSweepThreads / 64][NP * 16];
    reinterpret_cast<sw_u32x4 *>(T)[threadIdx.x] = reinterpret_cast<const sw_u32x4 *>(tab)[threadIdx.x];     // 256 x 16 B
    __syncthreads();
    const unsigned c0 = (unsigned)((first - 17) & 7);                   // (n - 17) mod 8 of every group's sample 0
    uint32_t acc[NP][8];
#pragma unroll
    for (int k = 0; k < NP; k++)
#pragma unroll
        for (int j = 0; j < 8; j++) acc[k][j] = 0;
    const unsigned long long ngroups = (nsamples + 15) / 16;
    for (unsigned long long g = (unsigned long long)blockIdx.x * kSweepThreads + threadIdx.x; g < ngroups;
         g += (unsigned long long)gridDim.x * kSweepThreads) {
        const unsigned long long base = g * 16, n0 = first + base;
        const long long M0 = ((long long)n0 - 17) >> 3;                  // floor
        const unsigned Q = data_window10(bits, m0, navail, source, M0);
        unsigned long long nz0 = 0, nz1 = 0;
        if (base + 16 <= nsamples && n0 >= BBB_TX_BIT_SAMPLE0) {
            if (noise) {
                const sw_u64x2 v = *reinterpret_cast<const sw_u64x2 *>(noise + base);
                nz0 = v[0];
                nz1 = v[1];
            }
            sweep_group<NP, THR, false>(P, T, nz0, nz1, Q, c0, 0, 16, acc);
        } else {
            // the chunk's ragged end, and samples before the first decided bit (n < 45)
            const unsigned hi = nsamples - base < 16 ? (unsigned)(nsamples - base) : 16u;
            const unsigned lo = n0 >= BBB_TX_BIT_SAMPLE0 ? 0u : (unsigned)std::min<unsigned long long>(16, BBB_TX_BIT_SAMPLE0 - n0);
            if (noise)
                for (unsigned e = 0; e < hi; e++) {
                    const unsigned long long v = (unsigned long long)(uint8_t)noise[base + e] << (8 * (e & 7));
                    if (e < 8) nz0 |= v; else nz1 |= v;
                }
            sweep_group<NP, THR, true>(P, T, nz0, nz1, Q, c0, lo, hi, acc);
        }
    }

    // per wave (both 16-bit halves at once: a sum over 64 lanes stays below 2^16), then per block
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned d = (c0 + 4) & 7;                                       // bathtub phase of slot 0: (n - 45) mod 8
#pragma unroll
    for (int k = 0; k < NP; k++)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            uint32_t v = acc[k][j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0) {
                const unsigned p = (d + (unsigned)j) & 7;
                W[wave][(2 * k) * 8 + p] = v & 0xffffu;
                W[wave][(2 * k + 1) * 8 + p] = v >> 16;
            }
        }
    __syncthreads();
    if (threadIdx.x < NP * 16) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kSweepThreads / 64; w++) s += W[w][threadIdx.x];
        scratch[(unsigned long long)blockIdx.x * (NP * 16) + threadIdx.x] = s;
    }
}

// counters[idx][p] += (bits decided at phase p, the blocks' errors): block t folds slot t >> 3, phase t & 7
__global__ void __launch_bounds__(256)
txsweep_reduce_kernel(const uint32_t *__restrict scratch, unsigned blocks, unsigned width, SweepOut o,
                      unsigned long long *__restrict counters) {
    __shared__ unsigned long long R[4];
    const unsigned t = blockIdx.x;
    const int i = o.idx[t >> 3];
    if (i < 0) return;                                                      // padding: the whole block
    unsigned long long s = 0;
    for (unsigned b = threadIdx.x; b < blocks; b += 256) s += scratch[(unsigned long long)b * width + t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) R[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned p = t & 7;
        unsigned long long *c = counters + ((unsigned long long)i * 8 + p) * 2;
        c[0] += o.bits[p];
        c[1] += R[0] + R[1] + R[2] + R[3];
    }
}

int sweep_tables_launch(const int16_t *coeffs_dev, int ntab, uint16_t *tables, hipStream_t st) {
    if (ntab <= 0) return BBB_OK;
    txsweep_table_kernel<<<ntab, 256, 0, st>>>(coeffs_dev, tables);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

int sweep_grid_blocks(uint64_t n) {
    int dev = 0, cus = 0;
    BBB_HIP(hipGetDevice(&dev));
    BBB_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // the most any launch takes: four blocks per CU, or more when a thread would otherwise take over kSweepMaxIters groups
    const uint64_t groups = (std::min<uint64_t>(n, kSweepLaunchMax) + 15) / 16;
    const uint64_t least = (groups + kSweepThreads * kSweepMaxIters - 1) / (kSweepThreads * kSweepMaxIters);
    return (int)std::max<uint64_t>({1, least, 4 * (uint64_t)std::max(cus, 1)});
}

// One round of resident blocks (grid-stride, every thread the same share of groups): the grid is what the CUs hold at once
// for this kernel's registers (NP = 8 runs 3 waves per SIMD: 3 blocks per CU), not a fixed count that would leave a tail.
template <int NP, bool THR>
static int sweep_dispatch(unsigned groups, int blocks, hipStream_t st, const SweepPairs &P, const uint16_t *tab, const SweepChunk &c,
                          uint32_t *scratch, unsigned *nb_out) {
    static int per_cu = 0;                                     // the same on every device this library runs on (gfx950)
    if (!per_cu) {
        int v = 0;
        BBB_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, txsweep_kernel<NP, THR>, kSweepThreads, 0));
        per_cu = std::max(1, std::min(v, 4));
    }
    int dev = 0, cus = 0;
    BBB_HIP(hipGetDevice(&dev));
    BBB_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const uint64_t least = ((uint64_t)groups + kSweepThreads * kSweepMaxIters - 1) / (kSweepThreads * kSweepMaxIters);
    const uint64_t want = std::max<uint64_t>(least, (uint64_t)std::max(cus, 1) * per_cu);
    // fewer blocks only when every thread has at most one group
    const unsigned nb = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)blocks, want, ((uint64_t)groups + kSweepThreads - 1) / kSweepThreads}));
    const unsigned long long navail = c.bits ? c.navail : 0;
    txsweep_kernel<NP, THR><<<nb, kSweepThreads, 0, st>>>(P, tab, c.noise, c.bits, c.m0, navail, c.source, c.first, c.n, scratch);
    *nb_out = nb;
    return BBB_OK;
}

int sweep_launch(const SweepGroup &g, const uint16_t *tables, const SweepChunk &c, uint32_t *scratch, int blocks,
                 uint64_t *counters, hipStream_t st) {
    if (c.n == 0) return BBB_OK;
    if (c.n > kSweepLaunchMax) return fail(BBB_EINVAL, "a sweep launch covers at most 2^31 samples");
    if (g.pairs < 1 || g.pairs > kSweepMaxPairs) return fail(BBB_EINVAL, "bad sweep group");
    const int np = g.pairs <= 1 ? 1 : (g.pairs <= 4 ? 4 : 8);
    SweepPairs P{};
    SweepOut o{};
    for (int k = 0; k < kSweepMaxPairs; k++) {
        P.nv2[k] = g.nv2[k];
        P.t0[k] = g.t0[k];
        P.t1[k] = g.t1[k];
        o.idx[2 * k] = k < g.pairs ? g.idx[2 * k] : -1;
        o.idx[2 * k + 1] = k < g.pairs ? g.idx[2 * k + 1] : -1;
    }
    tx_phase_bits(c.first, c.n, o.bits);
    const unsigned groups = (unsigned)((c.n + 15) / 16);
    const uint16_t *tab = tables + (uint64_t)g.table * 8 * 256;
    unsigned nb = 0;
    int rc;
    if (np == 1) rc = g.thr ? sweep_dispatch<1, true>(groups, blocks, st, P, tab, c, scratch, &nb) : sweep_dispatch<1, false>(groups, blocks, st, P, tab, c, scratch, &nb);
    else if (np == 4) rc = g.thr ? sweep_dispatch<4, true>(groups, blocks, st, P, tab, c, scratch, &nb) : sweep_dispatch<4, false>(groups, blocks, st, P, tab, c, scratch, &nb);
    else rc = g.thr ? sweep_dispatch<8, true>(groups, blocks, st, P, tab, c, scratch, &nb) : sweep_dispatch<8, false>(groups, blocks, st, P, tab, c, scratch, &nb);
    if (rc) return rc;
    BBB_HIP(hipGetLastError());
    txsweep_reduce_kernel<<<np * 16, 256, 0, st>>>(scratch, nb, (unsigned)(np * 16), o, reinterpret_cast<unsigned long long *>(counters));
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
