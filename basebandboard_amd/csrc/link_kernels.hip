// link_kernels.hip -- eye, bathtub and BER of the shaped link BEHIND a receive filter (include/bbb.h, bbb_link_sweep_*).
//
//   x(n)   = TX.x of a setting (tx_kernels.hip), 0 for n < 0
//   acc(n) = sum_{i < ntaps} h[i] x(n - i)          z(n) = sat16(acc(n) >> shift)          (fir_kernels.hip)
//   stream sample s is acc(s + delay) / z(s + delay): decided per phase as the bathtub of eye_kernels.hip decides x, binned
//   as its histogram bins x.
// One launch serves one setting over the chunk's cached int8 noise; the int16 waveform exists in LDS only.  A workgroup step
// takes kLinkTile outputs, indexed by WAVEFORM sample j = s + delay:
//  1. every thread forms the 8 samples x(j0 .. j0 + 7), j0 = tile + 8 t, from one 8-byte noise load, one 64-bit window of
//     data bits (the shaper's 10-bit window of data_window10 on top, the bits its outputs are decided against below: loaded
//     one step ahead) and the setting's table of shaped values T[ph][q] in LDS (the sweep's table, 16 T + 8, taken back to T
//     when it is copied in); threads t < ngroups also form the 8 ngroups samples in front of the tile.  The host places the
//     tiles so that j0 - norg (norg: the sample of noise[0]) is a multiple of 8 and (j0 - 17) mod 8 is one value c0 for the
//     whole launch;
//  2. the image is fir_common.hpp's, and fir_block8, the one block core fir_kernel runs too, gives every thread its eight
//     outputs from it.  Two images alternate, so a step costs one barrier;
//  3. slot r of every thread has the same bathtub phase: the errors are counted in 8 registers, and the two data bits a
//     thread's outputs belong to sit in the window it formed its samples from;
//  4. HIST: eye_common.hpp's LDS histogram (eye_add8 with its mask for the outputs that do not count, eye_flush).
// The block's partial goes to a scratch slab with plain stores and eye_reduce_launch folds it in u64 (no global atomics);
// the bits decided per phase are host arithmetic on the range.  Outputs outside [out_lo, out_hi) -- at most 7 in front, the
// ragged end behind -- are formed and dropped.  A launch covers < 2^31 samples, so every u32 count is exact.
#include "bbb_common.hpp"
#include "eye_common.hpp"
#include "fir_common.hpp"
#include "tx_common.hpp"

#include <algorithm>

namespace bbb {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct LinkRaw { unsigned long long nz, bw; };

// What the waveform samples j0 .. j0 + 7 are made of: their 8 noise bytes, and the data bits Mb .. Mb + 63 with
// Mb = M0 - kBitsBelow, M0 = floor((j0 - 17) / 8).  Bits kBitsBelow - 7 .. kBitsBelow + 2 of bw are the shaper's 10-bit
// window of data_window10 (data bits M0 - 7 .. M0 + 2; bits below 0 read as 0: the reset shift register); the bits a thread
// decides lie at most (255 + 28) / 8 + 1 = 36 bits below M0.  j0 - norg is a multiple of 8.
constexpr int kBitsBelow = 47;
__device__ inline LinkRaw fetch8(const LinkLaunch &a, long long j0) {
    LinkRaw r{0, 0};
    if (j0 + 8 <= 0) return r;
    if (a.noise) {
        const long long idx = j0 - a.norg;
        if (idx >= 0 && (unsigned long long)idx + 8 <= a.nnoise) {
            r.nz = *reinterpret_cast<const unsigned long long *>(a.noise + idx);
        } else {
            for (int e = 0; e < 8; e++)
                if (idx + e >= 0 && (unsigned long long)(idx + e) < a.nnoise) r.nz |= (unsigned long long)(uint8_t)a.noise[idx + e] << (8 * e);
        }
    }
    const long long Mb = ((j0 - 17) >> 3) - kBitsBelow;                 // floor
    if (a.source) {
        const unsigned pos = (unsigned)(-Mb) & 255u;                    // Pulser: the one multiple of 256 from Mb on (tx.py:28-30)
        if (pos < 64 && Mb + (long long)pos >= 0) r.bw = 1ull << pos;
    } else if (Mb >= a.m0) {
        const unsigned long long rel = (unsigned long long)(Mb - a.m0), w = rel >> 6;
        const unsigned sh = (unsigned)(rel & 63);
        if (w + 1 < a.nwords) {
            const unsigned long long w0 = a.bits[w], w1 = a.bits[w + 1];
            r.bw = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
        }
    } else if (a.m0 - Mb < 64) {
        r.bw = a.bits[0] << (unsigned)(a.m0 - Mb);                      // only at the start of the stream, where m0 = 0
    }
    return r;
}

// ... and the samples themselves as four dwords; 0 below sample 0.  (j0 - 17) mod 8 = c0
__device__ inline uint4 shape8(const LinkLaunch &a, const int16_t *T, unsigned c0, long long j0, const LinkRaw &r) {
    if (j0 + 8 <= 0) return make_uint4(0, 0, 0, 0);
    const unsigned Q = (unsigned)(r.bw >> (kBitsBelow - 7)) & 0x3ffu;
    uint32_t x[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const unsigned ce = c0 + (unsigned)e, ph = ce & 7u;
        const unsigned q = (Q >> (ce >> 3)) & 255u;
        const int g = (int)(int8_t)(r.nz >> (8 * e));
        const int v = wrap12_dev((int)T[ph * 256 + q] + wrap12_dev(g * a.nv));           // tx.py:75-81
        x[e] = j0 + e >= 0 ? (uint32_t)v & 0xffffu : 0u;
    }
    return make_uint4(x[0] | x[1] << 16, x[2] | x[3] << 16, x[4] | x[5] << 16, x[6] | x[7] << 16);
}

template <bool HIST>
__global__ __launch_bounds__(kFirThreads) void link_kernel(LinkLaunch a, uint32_t *__restrict scratch) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[2][kFirLdsWords];
    __shared__ __attribute__((aligned(16))) int16_t T[8 * 256];
    __shared__ uint32_t H[HIST ? kEyeRows * kEyeLanes : 1];
    __shared__ uint32_t E[8];
    const int t = threadIdx.x;
    {
        // the sweep's table holds 16 T + 8 (mod 2^16): an arithmetic shift of the int16 gives T back
        const u32x4 v = reinterpret_cast<const u32x4 *>(a.table)[t];                          // 256 x 16 B = the table
        u32x4 w;
#pragma unroll
        for (int k = 0; k < 4; k++)
            w[k] = ((uint32_t)((int)(int16_t)(v[k] & 0xffffu) >> 4) & 0xffffu) | ((uint32_t)((int)v[k] >> 20) << 16);
        reinterpret_cast<u32x4 *>(T)[t] = w;
    }
    eye_zero<HIST>(H, E, t, kFirThreads);
    __syncthreads();

    const int ng = (int)a.ngroups;
    const unsigned c0 = (unsigned)((a.tb - 17) & 7);
    const unsigned lane = t & 63, rot = (lane >> 2) & 7;
    // stream sample of the first tile's output 0, its bathtub phase and its lane-column (a tile is a multiple of 64 samples)
    const long long s00 = a.tb - (long long)a.delay;
    const unsigned d = (unsigned)((s00 - BBB_TX_BIT_SAMPLE0) & 7);             // slots j >= 8 - d belong to the next bit
    const unsigned cb = (unsigned)(((unsigned long long)s00 - a.col_origin) & 63) + 8u * (lane & 7);
    const uint64_t nsteps = ((uint64_t)(a.out_hi - a.tb) + kLinkTile - 1) / kLinkTile;
    uint32_t err[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    // the inputs of a step are loaded one step ahead, as fir_kernel loads its samples
    auto own = [&](uint64_t step) { return fetch8(a, a.tb + (long long)(step * kLinkTile) + 8 * t); };
    auto lead = [&](uint64_t step) { return t < ng ? fetch8(a, a.tb + (long long)(step * kLinkTile) - 8 * (t + 1)) : LinkRaw{0, 0}; };
    uint64_t s = blockIdx.x;
    LinkRaw cur{0, 0}, cur_lead{0, 0};
    if (s < nsteps) {
        cur = own(s);
        cur_lead = lead(s);
    }
    for (int par = 0; s < nsteps; s += gridDim.x, par ^= 1) {
        const long long base = a.tb + (long long)(s * kLinkTile);
        const uint64_t next = s + gridDim.x;
        LinkRaw nxt{0, 0}, nxt_lead{0, 0};
        if (next < nsteps) {
            nxt = own(next);
            nxt_lead = lead(next);
        }
        uint32_t *L = lds[par];
        *reinterpret_cast<uint4 *>(L + kFirHist / 2 + 4 * t) = shape8(a, T, c0, base + 8 * t, cur);
        if (t < ng) *reinterpret_cast<uint4 *>(L + kFirHist / 2 - 4 * (t + 1)) = shape8(a, T, c0, base - 8 * (t + 1), cur_lead);
        const unsigned long long bw = cur.bw;
        cur = nxt;
        cur_lead = nxt_lead;
        __syncthreads();
        const long long n0 = base + 8 * t;
        // this thread's outputs inside the range: lo <= r < hi
        const int lo = (int)min((long long)8, max((long long)0, a.out_lo - n0));
        const int hi = (int)min((long long)8, max((long long)0, a.out_hi - n0));
        if (hi <= lo) continue;
        int acc[8];
        fir_block8(L, t, ng, a.taps, acc);
        // the decisions against the data bits
        const long long F = (n0 - (long long)a.delay - BBB_TX_BIT_SAMPLE0) >> 3;       // floor: the bit of slot 0
        const unsigned at = (unsigned)(F - ((n0 - 17) >> 3) + kBitsBelow);              // where bit F sits in bw
        const int b0 = F >= 0 ? (int)((bw >> at) & 1ull) : -1, b1 = F + 1 >= 0 ? (int)((bw >> (at + 1)) & 1ull) : -1;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int b = (unsigned)j < 8u - d ? b0 : b1;
            err[j] += (unsigned)(j >= lo && j < hi && b >= 0) & (eye_decide(acc[j], a.threshold, a.strict) != (unsigned)b);
        }
        if constexpr (HIST) {
            unsigned A[8];
#pragma unroll
            for (int r = 0; r < 8; r++)
                A[r] = r >= lo && r < hi ? eye_row(sat16(acc[r] >> a.shift), a.eye_shift) * kEyeLanes + ((cb + r) & 63) : ~0u;
            eye_add8<true>(H, A, rot);
        }
    }

    eye_fold_errors(E, err, d, lane);
    __syncthreads();
    eye_flush<HIST, true>(H, E, scratch, HIST ? kEyeRows * a.ncols : 0, a.ncols, t, kFirThreads);
}

}  // namespace

int link_grid_blocks(bool hist) {
    int dev = 0, cus = 0, per_cu = 0;
    BBB_HIP(hipGetDevice(&dev));
    BBB_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // one round of resident blocks (a grid-stride loop over the steps): what a CU holds at once, not a count that leaves a tail
    if (hist) BBB_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, link_kernel<true>, kFirThreads, 0));
    else BBB_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, link_kernel<false>, kFirThreads, 0));
    return std::max(cus, 1) * std::max(per_cu, 1);
}

int link_launch(const LinkLaunch &a, bool hist, uint64_t first, uint64_t n, uint32_t *scratch, int blocks, uint64_t *hist_out,
                uint64_t *counters, hipStream_t st) {
    if (n == 0) return BBB_OK;
    if (n > kLinkLaunchMax) return fail(BBB_EINVAL, "a link launch covers at most 2^31 samples");
    const uint64_t nsteps = ((uint64_t)(a.out_hi - a.tb) + kLinkTile - 1) / kLinkTile;
    const unsigned nb = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(nsteps, (uint64_t)blocks));
    if (hist) link_kernel<true><<<nb, kFirThreads, 0, st>>>(a, scratch);
    else link_kernel<false><<<nb, kFirThreads, 0, st>>>(a, scratch);
    BBB_HIP(hipGetLastError());
    return eye_reduce_launch(scratch, nb, hist ? kEyeRows * a.ncols : 0, hist ? hist_out : nullptr, counters, first, n, st);
}

}  // namespace bbb
