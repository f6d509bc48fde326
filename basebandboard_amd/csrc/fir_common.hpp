// fir_common.hpp -- what the FIR filter (fir_kernels.hip) and the filtered link (link_kernels.hip) share: the LDS image of a
// workgroup step and the block core that turns it into eight outputs per thread.
//
// The image of a step: kFirThreads threads, thread t owns the 8 samples n0 .. n0 + 7, n0 = 8 t, of the step's kFirTile; they
// are the four dwords from kFirHist / 2 + 4 t on.  The 8 * ngroups samples in front of the step lie below dword kFirHist / 2
// (thread t < ngroups stores the four dwords from kFirHist / 2 - 4 (t + 1) on).  How the samples get there is the kernel's
// own business: fir_kernel loads them, link_kernel shapes them.
#pragma once

#include "bbb_common.hpp"

namespace bbb {

constexpr int kFirThreads = 256;
constexpr int kFirHist = 256;                 // LDS samples in front of a step's first sample (8 * ngroups are staged)
constexpr int kFirLdsWords = (kFirHist + kFirTile) / 2 + 4;
static_assert(kLinkTile == kFirTile, "link_kernel runs fir_block8 on fir_kernel's image");
static_assert(kFirTile == 8 * kFirThreads, "eight samples per thread");

typedef short fir_v2s __attribute__((ext_vector_type(2)));

// two taps of one output: v_dot2_i32_i16
__device__ __forceinline__ int dot2(uint32_t x, uint32_t h, int acc) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(fir_v2s, x), __builtin_bit_cast(fir_v2s, h), acc, false);
}

__device__ __forceinline__ int sat16(int v) { return min(max(v, -32768), 32767); }

// acc[r] = sum_i h[i] x[n0 + r - i] for thread t's outputs n0 + r, r < 8, over the image L and ng groups of four tap words
// (word p = h[2p + 1] | h[2p] << 16; `taps` is the kernel argument's array, so the words stay scalar loads).  The pairs of
// the odd outputs are aligned dwords, those of the even outputs straddle two and are made with v_alignbyte_b32.  Going from
// pair p to p + 1 moves every window down by exactly one dword, so four pairs cost one 16-byte LDS read (aligned: dword
// 4 t + kFirHist / 2 - 4 g), four new v_alignbyte_b32 and 32 dot products.
__device__ __forceinline__ void fir_block8(const uint32_t *L, int t, unsigned ng, const uint32_t *taps, int (&acc)[8]) {
    const int D0 = kFirHist / 2 + 4 * t;                            // the dword of x[n0], x[n0 + 1]
    const uint4 h4 = *reinterpret_cast<const uint4 *>(L + D0);
    uint32_t d[8], al[7];
    d[4] = h4.x, d[5] = h4.y, d[6] = h4.z, d[7] = h4.w;
#pragma unroll
    for (int k = 4; k < 7; ++k) al[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], 2);
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = 0;
    for (unsigned g = 0; g < ng; ++g) {                             // unsigned: a trip of two groups loads its 8 tap words at once
        // d[k] is dword D0 - 4 g - 4 + k, al[k] its high sample with the low sample of the next
        const uint4 l4 = *reinterpret_cast<const uint4 *>(L + D0 - 4 * (g + 1));
        d[0] = l4.x, d[1] = l4.y, d[2] = l4.z, d[3] = l4.w;
#pragma unroll
        for (int k = 0; k < 4; ++k) al[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], 2);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t h = taps[4 * g + u];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[2 * r + 1] = dot2(d[4 - u + r], h, acc[2 * r + 1]);
                acc[2 * r] = dot2(al[3 - u + r], h, acc[2 * r]);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) d[4 + k] = d[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) al[4 + k] = al[k];
    }
}

}  // namespace bbb
