// fir_kernels.hip -- the exact integer FIR filter over int16 samples (include/bbb.h, bbb_fir_*).
//
//   acc(n) = sum_{i < ntaps} h[i] * x[n - i]        y[q] = sat(acc(phase + q * decim) >> shift)
// sum |h| <= 65535 keeps |acc| below 2^31, so int32 is the definition.  One v_dot2_i32_i16 is two taps of one output: the
// tap word of pair p holds h[2p + 1] in its low half and h[2p] in its high half and meets the dword (x[n - 2p - 1], x[n - 2p])
// in memory order.  The tap words are a kernel argument (zero-padded to groups of four) and are read with scalar loads.
// A workgroup stages the 2048 inputs of its step and the 8 * ngroups samples in front of them in LDS, loaded one step ahead
// as sinc_kernel does (16-byte loads where the input is 16-byte aligned and the chunk lies inside the record, 2-byte loads
// otherwise); the two LDS buffers alternate, so a step costs one barrier.
//
// The image and the block core are fir_common.hpp's, shared with the filtered link (link_kernels.hip).
// Block form (decim = 1): a thread produces the 8 outputs n0 .. n0 + 7, n0 = 8 t, with fir_block8.
// Point form (decim > 1): a thread produces one requested output at a time with fir_point.
// The slicer writes no samples: the block kernel's 8 decisions are one byte of the packed output, the point kernel takes a
// ballot of 64 consecutive bits (lane = q mod 64) and stores whole words, or ORs the words a step shares with its neighbour
// into the zeroed output.
#include "bbb_common.hpp"
#include "eye_common.hpp"
#include "fir_common.hpp"

#include <algorithm>

namespace bbb {
namespace {

// MODE 0: int16 out, 1: int32 out, 2: packed decisions.  POINT: the kernel for decim > 1.
template <int MODE, bool POINT>
__global__ __launch_bounds__(kFirThreads) void fir_kernel(FirLaunch a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[2][kFirLdsWords];
    const int t = threadIdx.x;
    const uint64_t nsteps = (a.nin + kFirTile - 1) / kFirTile;
    const int ng = (int)a.ngroups;
    auto own = [&](uint64_t step) { return fir_load8(a, (int64_t)(step * kFirTile) + 8 * t); };
    auto lead = [&](uint64_t step) { return t < ng ? fir_load8(a, (int64_t)(step * kFirTile) - 8 * (t + 1)) : make_uint4(0, 0, 0, 0); };
    uint64_t s = blockIdx.x;
    uint4 cur = make_uint4(0, 0, 0, 0), cur_lead = cur;
    if (s < nsteps) {
        cur = own(s);
        cur_lead = lead(s);
    }
    for (int par = 0; s < nsteps; s += gridDim.x, par ^= 1) {
        const uint64_t base = s * kFirTile, next = s + gridDim.x;
        uint4 nxt = make_uint4(0, 0, 0, 0), nxt_lead = nxt;
        if (next < nsteps) {
            nxt = own(next);
            nxt_lead = lead(next);
        }
        uint32_t *L = lds[par];
        *reinterpret_cast<uint4 *>(L + kFirHist / 2 + 4 * t) = cur;
        if (t < ng) *reinterpret_cast<uint4 *>(L + kFirHist / 2 - 4 * (t + 1)) = cur_lead;
        cur = nxt;
        cur_lead = nxt_lead;
        __syncthreads();
        if constexpr (!POINT) {
            const uint64_t n0 = base + 8 * t;
            // the slicer also writes the zero bytes that complete the last word
            if (n0 >= (MODE == 2 ? (a.nin + 63) / 64 * 64 : a.nin)) continue;
            int acc[8];
            fir_block8(L, t, ng, a.taps, acc);
            const int nv = (int)min((uint64_t)8, a.nin > n0 ? a.nin - n0 : 0);     // outputs of this thread inside the record
            if constexpr (MODE == 2) {
                uint32_t byte = 0;
#pragma unroll
                for (int r = 0; r < 8; ++r) byte |= (uint32_t)(r < nv && eye_decide(acc[r], a.threshold, a.strict)) << r;
                reinterpret_cast<uint8_t *>(a.out)[n0 >> 3] = (uint8_t)byte;
            } else if constexpr (MODE == 0) {
                int16_t *out = reinterpret_cast<int16_t *>(a.out) + n0;
                int y[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) y[r] = sat16(acc[r] >> a.shift);
                if (a.out_vec && nv == 8) {
                    uint32_t w[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) w[k] = ((uint32_t)y[2 * k] & 0xFFFFu) | (uint32_t)y[2 * k + 1] << 16;
                    *reinterpret_cast<uint4 *>(out) = make_uint4(w[0], w[1], w[2], w[3]);
                } else {
#pragma unroll
                    for (int r = 0; r < 8; ++r)
                        if (r < nv) out[r] = (int16_t)y[r];
                }
            } else {
                int32_t *out = reinterpret_cast<int32_t *>(a.out) + n0;
                if (a.out_vec && nv == 8) {
                    reinterpret_cast<int4 *>(out)[0] = make_int4(acc[0] >> a.shift, acc[1] >> a.shift, acc[2] >> a.shift, acc[3] >> a.shift);
                    reinterpret_cast<int4 *>(out)[1] = make_int4(acc[4] >> a.shift, acc[5] >> a.shift, acc[6] >> a.shift, acc[7] >> a.shift);
                } else {
#pragma unroll
                    for (int r = 0; r < 8; ++r)
                        if (r < nv) out[r] = acc[r] >> a.shift;
                }
            }
        } else {
            // the outputs whose input index lies in this step: q_lo <= q < q_hi
            const uint64_t end = base + kFirTile;
            const uint64_t q_lo = base <= a.phase ? 0 : (base - a.phase + a.decim - 1) / a.decim;
            const uint64_t q_hi = end <= a.phase ? 0 : min(a.nout, (end - a.phase + a.decim - 1) / a.decim);
            const int lane = t & 63;
            for (uint64_t qb = (q_lo & ~63ull) + (uint64_t)(t - lane); qb < q_hi; qb += kFirThreads) {
                const uint64_t q = qb + lane;
                const bool valid = q >= q_lo && q < q_hi;
                int acc1[1] = {0};
                const uint32_t *const img[1] = {L};
                // l0: the lower sample of pair 0
                if (valid) fir_point(img, (int)(a.phase + q * a.decim - base) + kFirHist - 1, ng, a.taps, acc1);
                const int acc = acc1[0];
                if constexpr (MODE == 2) {
                    const unsigned long long bits = __ballot(valid && eye_decide(acc, a.threshold, a.strict)), mask = __ballot(valid);
                    if (lane == 0 && mask) {
                        unsigned long long *w = reinterpret_cast<unsigned long long *>(a.out) + (qb >> 6);
                        if (mask == ~0ull) *w = bits;
                        else atomicOr(w, bits);
                    }
                } else if constexpr (MODE == 0) {
                    if (valid) reinterpret_cast<int16_t *>(a.out)[q] = (int16_t)sat16(acc >> a.shift);
                } else {
                    if (valid) reinterpret_cast<int32_t *>(a.out)[q] = acc >> a.shift;
                }
            }
        }
    }
}

template <int MODE>
void launch_mode(const FirLaunch &a, unsigned g, hipStream_t st) {
    if (a.decim == 1) fir_kernel<MODE, false><<<g, kFirThreads, 0, st>>>(a);
    else fir_kernel<MODE, true><<<g, kFirThreads, 0, st>>>(a);
}

}  // namespace

int fir_launch(const FirLaunch &a, int mode, int grid, hipStream_t st) {
    const uint64_t nsteps = (a.nin + kFirTile - 1) / kFirTile;
    const unsigned g = (unsigned)std::min<uint64_t>(nsteps, (uint64_t)grid);
    if (mode == 0) launch_mode<0>(a, g, st);
    else if (mode == 1) launch_mode<1>(a, g, st);
    else launch_mode<2>(a, g, st);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
