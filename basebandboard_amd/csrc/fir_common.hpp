// fir_common.hpp -- what the FIR filter (fir_kernels.hip), the filtered link (link_kernels.hip) and the down-converter
// (ddc_kernels.hip) share: the LDS image of a workgroup step, the load of a thread's eight input samples, the block core that
// turns the image into eight outputs per thread and the point core that turns it into one.
//
// The image of a step: kFirThreads threads, thread t owns the 8 samples n0 .. n0 + 7, n0 = 8 t, of the step's kFirTile; they
// are the four dwords from kFirHist / 2 + 4 t on.  The 8 * ngroups samples in front of the step lie below dword kFirHist / 2
// (thread t < ngroups stores the four dwords from kFirHist / 2 - 4 (t + 1) on).  How the samples get there is the kernel's
// own business: fir_kernel loads them, link_kernel shapes them, ddc_kernel mixes them with its oscillator (two images).
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

// the input samples j0 .. j0 + 7 of a launch structure A (in, nin, nbefore, in_vec) as four dwords; 0 before in[-nbefore]
// and from in[nin] on.  One 16-byte load where the input is 16-byte aligned and the eight lie inside the record.
template <class A>
__device__ __forceinline__ uint4 fir_load8(const A &a, int64_t j0) {
    const int64_t lo = -(int64_t)a.nbefore, hi = (int64_t)a.nin;
    if (j0 + 8 <= lo || j0 >= hi) return make_uint4(0, 0, 0, 0);
    if (a.in_vec && j0 >= lo && j0 + 8 <= hi) return *reinterpret_cast<const uint4 *>(a.in + j0);
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t j = j0 + 2 * k;
        const uint32_t s0 = j >= lo && j < hi ? (uint16_t)a.in[j] : 0u;
        const uint32_t s1 = j + 1 >= lo && j + 1 < hi ? (uint16_t)a.in[j + 1] : 0u;
        w[k] = s0 | s1 << 16;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

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

// The point core: acc[i] = sum_k h[k] x_i[n - k] of ONE output n over NI images of the same step (x_i: image L[i]), n = l0 + 1 -
// kFirHist counted from the step's first sample (l0: the image's sample index of the lower sample of pair 0).  Per pair and
// image one ds_read_b32, one v_alignbyte_b32 whose byte selector (0 or 2) is the parity of l0, and one dot product.  The
// images' chains are independent, so the reads of one hide behind the dot products of the other.
template <int NI>
__device__ __forceinline__ void fir_point(const uint32_t *const (&L)[NI], int l0, int ng, const uint32_t *taps, int (&acc)[NI]) {
    const int dw = l0 >> 1;
    const uint32_t sel = (l0 & 1) ? 2u : 0u;
    uint32_t prev[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        prev[i] = L[i][dw + 1];
        acc[i] = 0;
    }
    for (int g = 0; g < ng; ++g) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t h = taps[4 * g + u];
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const uint32_t c = L[i][dw - 4 * g - u];
                acc[i] = dot2(__builtin_amdgcn_alignbyte(prev[i], c, sel), h, acc[i]);
                prev[i] = c;
            }
        }
    }
}

}  // namespace bbb
