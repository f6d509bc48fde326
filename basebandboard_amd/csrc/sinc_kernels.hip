// sinc_kernels.hip -- the scope's 16x sinc interpolator (gateware/bbb/sinc.py:52-130; include/bbb.h, bbb_sinc_*).
//
//   acc(m, c) = sum_{i=0..7} h[16 i + c] * x[m - i]        y[16 m + c] = int8(acc(m, c) >> 8)
// One thread per input sample m: it holds x[m - 7 .. m] as two dwords of int8 (memory order) and, for each phase c, takes
// two v_dot4c_i32_i8 against the two BRAM words of that phase (sinc.py:42-48 packs them in exactly the order the window
// has in memory: word 2c = h[c], h[16 + c], h[32 + c], h[48 + c] from the top byte down meets x[m], x[m - 1], x[m - 2],
// x[m - 3]; word 2c + 1 meets x[m - 4 .. m - 7]).  |acc| <= 25 984, so int32 and one arithmetic shift are the module's
// 16-bit adder tree exactly; the shift itself is a byte selection folded into the packing of the store.  The 32 words are a kernel argument and live in scalar registers.
// A workgroup stages the 256 inputs of its step and the 7 in front of them in LDS as int8 (int16 input is shifted and
// clamped there, once per sample); a thread reads the three aligned dwords that hold its window and shifts it out with
// v_alignbyte_b32.  No thread waits on another launch; the two LDS buffers alternate, so a step costs one barrier.
// A thread's 16 outputs are one 16-byte store (int8, non-temporal) or two (int16), a wave's stores 1 KiB or 2 KiB contiguous.
#include "bbb_common.hpp"

#include <algorithm>

namespace bbb {
namespace {

constexpr int kThreads = 256;                 // threads per workgroup = input samples per step
constexpr int kLead = 8;                      // LDS bytes in front of a step's first input (7 are read)
constexpr int kLdsWords = (kLead + kThreads) / 4 + 1;

template <bool IN16>
__device__ inline uint32_t sample8(const SincLaunch &a, int64_t j) {
    if constexpr (IN16) {
        const int v = reinterpret_cast<const int16_t *>(a.in)[j] >> a.shift;
        return (uint32_t)min(max(v, -128), 127) & 0xFFu;
    } else {
        return reinterpret_cast<const uint8_t *>(a.in)[j];
    }
}

template <bool IN16, bool OUT16>
__global__ __launch_bounds__(kThreads) void sinc_kernel(SincLaunch a) {
    __shared__ uint32_t lds[2][kLdsWords];
    const int t = threadIdx.x;
    const uint64_t nsteps = (a.n + kThreads - 1) / kThreads;
    // a step's own sample, and from the first 8 threads one of the samples in front of the step: the record's, then the
    // caller's, then 0.  Both are loaded one step ahead, so that a wave computes while its next loads are in flight.
    auto own = [&](uint64_t step) -> uint32_t {
        const uint64_t m = step * kThreads + t;
        return m < a.n ? sample8<IN16>(a, (int64_t)m) : 0u;
    };
    auto lead = [&](uint64_t step) -> uint32_t {
        const int64_t j = (int64_t)(step * kThreads) - kLead + t;
        return t < kLead && j >= -(int64_t)a.nbefore ? sample8<IN16>(a, j) : 0u;
    };
    uint64_t s = blockIdx.x;
    uint32_t cur = 0, cur_lead = 0;
    if (s < nsteps) {
        cur = own(s);
        cur_lead = lead(s);
    }
    for (int par = 0; s < nsteps; s += gridDim.x, par ^= 1) {
        const uint64_t m = s * kThreads + t, next = s + gridDim.x;
        uint32_t nxt = 0, nxt_lead = 0;
        if (next < nsteps) {
            nxt = own(next);
            nxt_lead = lead(next);
        }
        uint8_t *bytes = reinterpret_cast<uint8_t *>(lds[par]);
        bytes[kLead + t] = (uint8_t)cur;
        if (t < kLead) bytes[t] = (uint8_t)cur_lead;
        cur = nxt;
        cur_lead = nxt_lead;
        __syncthreads();
        if (m >= a.n) continue;
        // the window x[m - 7 .. m] is LDS bytes t + 1 .. t + 8
        const int q = (t + 1) >> 2, o = (t + 1) & 3;
        const uint32_t d0 = lds[par][q], d1 = lds[par][q + 1], d2 = lds[par][q + 2];
        const int lo = (int)__builtin_amdgcn_alignbyte(d1, d0, o);      // x[m - 7 .. m - 4]
        const int hi = (int)__builtin_amdgcn_alignbyte(d2, d1, o);      // x[m - 3 .. m]
        int acc[16];
#pragma unroll
        for (int c = 0; c < 16; ++c)
            acc[c] = __builtin_amdgcn_sdot4(hi, (int)a.words[2 * c], __builtin_amdgcn_sdot4(lo, (int)a.words[2 * c + 1], 0, false),
                                            false);
        // y = acc >> 8 is byte 1 of acc as int8 and bytes 1 and 2 as int16 (|acc| < 2^15): the wide paths pick those bytes
        // with v_perm_b32 (selector 0..3: a byte of the second operand, 4..7: of the first) and never shift
        if constexpr (OUT16) {
            int16_t *out = reinterpret_cast<int16_t *>(a.out) + 16 * m;
            if (a.vec) {
                uint32_t w[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) w[k] = __builtin_amdgcn_perm((uint32_t)acc[2 * k + 1], (uint32_t)acc[2 * k], 0x06050201u);
                // plain stores: each of the two covers half of every line it touches, and the cache joins the halves.  As
                // non-temporal stores they took 1.09 ms per 2^30 outputs instead of 0.61.
                reinterpret_cast<uint4 *>(out)[0] = make_uint4(w[0], w[1], w[2], w[3]);
                reinterpret_cast<uint4 *>(out)[1] = make_uint4(w[4], w[5], w[6], w[7]);
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c) out[c] = (int16_t)(acc[c] >> 8);
            }
        } else {
            int8_t *out = reinterpret_cast<int8_t *>(a.out) + 16 * m;
            if (a.vec) {
                uint32_t w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t p01 = __builtin_amdgcn_perm((uint32_t)acc[4 * k + 1], (uint32_t)acc[4 * k], 0x0c0c0501u);
                    const uint32_t p23 = __builtin_amdgcn_perm((uint32_t)acc[4 * k + 3], (uint32_t)acc[4 * k + 2], 0x0c0c0501u);
                    w[k] = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
                }
                // a wave's store is 1 KiB of whole lines that nobody reads back soon: non-temporal (0.23 ms per 2^30 outputs
                // against 0.29 with plain stores)
                typedef uint32_t v4u __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store((v4u){w[0], w[1], w[2], w[3]}, reinterpret_cast<v4u *>(out));
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c) out[c] = (int8_t)(acc[c] >> 8);
            }
        }
    }
}

}  // namespace

int sinc_launch(const SincLaunch &a, bool in16, bool out16, int grid, hipStream_t st) {
    const uint64_t nsteps = (a.n + kThreads - 1) / kThreads;
    const unsigned g = (unsigned)std::min<uint64_t>(nsteps, (uint64_t)grid);
    if (in16) {
        if (out16) sinc_kernel<true, true><<<g, kThreads, 0, st>>>(a);
        else sinc_kernel<true, false><<<g, kThreads, 0, st>>>(a);
    } else {
        if (out16) sinc_kernel<false, true><<<g, kThreads, 0, st>>>(a);
        else sinc_kernel<false, false><<<g, kThreads, 0, st>>>(a);
    }
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
