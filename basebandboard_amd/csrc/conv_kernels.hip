// conv_kernels.hip -- the convolutional codec on the device (include/bbb.h, bbb_conv_decode and bbb_conv_encode).
//
// The decoder is mlse_kernels.hip's plan on another trellis.  Block j of B steps is decided by one Viterbi run over its window,
// the W steps in front of it and the D behind it included (mlse_common.hpp has the arithmetic); windows do not depend on one
// another.  NS = 2^(K-1) lanes own one window, one lane per state: a wave holds 64 / NS windows, at K = 7 a wave IS one
// trellis.  Per workgroup:
//   * one thread per step stages the received values of the workgroup's whole span of steps into LDS, DEPUNCTURED: the
//     value's number comes from the period's table (conv_value_of_step: a multiply by the period's reciprocal, no division in
//     the loop), a punctured position, a value in front of the history and one behind the record are written as 0, a hard
//     bit as +1 / -1.  A step is N int16 padded to one LDS read (4 bytes at N = 2, 8 at N = 3), so the ACS loop is uniform;
//   * every wave walks the steps of its windows in lockstep.  A lane fetches the int32 metrics of its state's two
//     predecessors with one cross-lane move each (conv_fetch), adds the two gains (the lane's d(c_i) times the step's
//     values), keeps the larger; the 64 survivor bits of the wave are one ballot, one u64 per step in LDS;
//   * the NS lanes of a window agree on the end state through a butterfly (a terminated window that ends the record takes
//     state 0), and the window's lane 0 walks the survivor words back, packs the block's decisions and ORs them into the
//     zeroed output (blocks share words).
// The encoder has one thread per output word; it is bound by memory and kept plain.
#include "conv_launch.hpp"

#include <algorithm>

namespace bbb {
namespace {

constexpr size_t kConvLdsTarget = 40 * 1024;       // four workgroups in a compute unit's 160 KiB

// LDS of a workgroup: WL survivor words per wave, then the values of wpg B + W + D steps.  The workgroup shrinks until that
// fits; if 64 threads still hold more windows than fit (small NS, long blocks, N = 3), the workgroup owns fewer windows
// than its lanes could and the others idle.
struct ConvShape {
    uint32_t threads, wpg;
    size_t bytes;
};
size_t conv_lds_bytes(uint32_t threads, uint32_t wpg, uint32_t n, const MlseGeom &g) {
    const size_t wl = g.B + g.W + g.D;
    return ((size_t)(threads / kWave) * wl * 8 + ((size_t)wpg * g.B + g.W + g.D) * (n == 2 ? 4 : 8) + 15) & ~(size_t)15;
}
ConvShape conv_shape(uint32_t ns, uint32_t n, const MlseGeom &g) {
    ConvShape s{};
    for (uint32_t threads = 256; threads >= (uint32_t)kWave; threads /= 2) {
        s.threads = threads;
        s.wpg = threads / ns;
        s.bytes = conv_lds_bytes(threads, s.wpg, n, g);
        if (s.bytes <= kConvLdsTarget) return s;
    }
    while (s.wpg > 1 && s.bytes > kConvLdsTarget) {
        s.wpg = (s.wpg + 1) / 2;
        s.bytes = conv_lds_bytes(s.threads, s.wpg, n, g);
    }
    return s;                                      // one window of 64 threads: at most 512 * 8 + 512 * 8 bytes
}

// The metric of predecessor C of every lane's state: a lane of the lane's own group of NS.  At NS = 4 the group is a quad and
// the move is a DPP quad permutation (lane q reads lane {0, 0, 1, 1}[q] for C = 0 and {2, 2, 3, 3}[q] for C = 1: conv_pred
// spelt out); above that it is ds_bpermute_b32 with the byte address worked out once.  Every lane of the wave is active where
// this is called.
template <int NS, int C>
__device__ __forceinline__ int32_t conv_fetch(int32_t m, int addr) {
    if constexpr (NS == 4) {
        static_assert(conv_pred(3, 0, 3) == 1 && conv_pred(1, 1, 3) == 2, "the quad permutation is conv_pred's");
        return __builtin_amdgcn_update_dpp(0, m, C ? 0xFA : 0x50, 0xF, 0xF, true);
    } else {
        return __builtin_amdgcn_ds_bpermute(addr, m);
    }
}

template <int NS, int N>
__global__ __launch_bounds__(256) void conv_decode_kernel(ConvLaunch a, uint32_t wpg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int K = NS == 4 ? 3 : NS == 8 ? 4 : NS == 16 ? 5 : NS == 32 ? 6 : 7;
    constexpr int SW = N == 2 ? 2 : 4;                                // int16 per staged step
    const int t = threadIdx.x, nthr = blockDim.x, lane = t & (kWave - 1), w = t / kWave;
    const uint32_t B = a.geom.B, W = a.geom.W, D = a.geom.D, WL = B + W + D;
    uint64_t *surv = reinterpret_cast<uint64_t *>(lds) + (size_t)w * WL;                             // this wave's
    int16_t *stage = reinterpret_cast<int16_t *>(lds + (size_t)(nthr / kWave) * WL * 8);
    const uint32_t h = (uint32_t)lane & (NS - 1), gbase = (uint32_t)lane & ~(uint32_t)(NS - 1);
    const ConvLane rule = conv_lane(a.gen, N, K, h);
    const int addr0 = (int)(gbase | conv_pred(h, 0, K)) * 4, addr1 = (int)(gbase | conv_pred(h, 1, K)) * 4;
    const uint64_t ngrp = (a.nblocks + wpg - 1) / wpg, end = a.first + a.nsteps;
    for (uint64_t grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
        const uint64_t jg = a.j0 + grp * wpg;
        const uint32_t nwin = (uint32_t)min((uint64_t)wpg, a.j0 + a.nblocks - jg);
        // the span: the steps from the first window's first to the last window's last, step T at index T - lo_u of the stage.
        // Its first step's place in the period and value number are worked out once per workgroup, every other step's from them.
        const int64_t lo_u = (int64_t)(jg * B) - (int64_t)W;
        const uint64_t T_lo = lo_u > 0 ? (uint64_t)lo_u : 0, T_hi = min(end, (jg + nwin) * B + D);
        const uint32_t r0 = (uint32_t)(T_lo % a.punct.p);
        const int64_t base = (int64_t)conv_idx(a.punct, T_lo) - (int64_t)a.idx_first;
        for (uint32_t i = (uint32_t)t; i < (uint32_t)(T_hi - T_lo); i += (uint32_t)nthr) {
            uint32_t r;
            const int64_t rel = conv_value_of_step(a.punct, base, r0, i, r);
            int16_t v[kConvMaxN];
            conv_step_values(a.punct, a.in, a.hard != 0, a.in_first, rel, a.rel_lo, a.rel_hi, r, v);
            int16_t *dst = stage + ((int64_t)T_lo - lo_u + i) * SW;
            if constexpr (N == 2) {
                *reinterpret_cast<uint32_t *>(dst) = (uint32_t)(uint16_t)v[0] | (uint32_t)(uint16_t)v[1] << 16;
            } else {
                *reinterpret_cast<uint2 *>(dst) = make_uint2((uint32_t)(uint16_t)v[0] | (uint32_t)(uint16_t)v[1] << 16, (uint32_t)(uint16_t)v[2]);
            }
        }
        __syncthreads();
        // the windows: window wi of the workgroup starts at step wi B of the stage
        const uint32_t wi = (uint32_t)w * (kWave / NS) + (uint32_t)lane / NS;
        const bool valid = wi < nwin;
        const MlseWindow win = mlse_window(a.geom, jg + wi, a.first, a.nsteps, a.ndecided);
        const int16_t *yw = stage + (size_t)(valid ? wi : 0) * B * SW;       // (a window beyond nwin decides nothing)
        int32_t m = conv_start(win.from_zero, h, a.init_state);
        // the steps [s_lo, s_hi) of the window's WL are walked: a_hi <= lo + WL, and a window beyond nwin walks none
        const uint32_t s_lo = valid ? (uint32_t)((int64_t)win.a_lo - win.lo) : 0u, s_hi = valid ? (uint32_t)((int64_t)win.a_hi - win.lo) : 0u;
        for (uint32_t s = 0; s < WL; ++s) {
            const bool active = s >= s_lo && s < s_hi;
            int16_t v[SW];
            if constexpr (N == 2) {
                const uint32_t x = *reinterpret_cast<const uint32_t *>(yw + (size_t)s * SW);
                v[0] = (int16_t)x;
                v[1] = (int16_t)(x >> 16);
            } else {
                const uint2 x = *reinterpret_cast<const uint2 *>(yw + (size_t)s * SW);
                v[0] = (int16_t)x.x;
                v[1] = (int16_t)(x.x >> 16);
                v[2] = (int16_t)x.y;
            }
            const int32_t m0 = conv_fetch<NS, 0>(m, addr0), m1 = conv_fetch<NS, 1>(m, addr1);
            uint32_t c;
            const int32_t mn = conv_acs<N>(rule, v, m0, m1, c);
            if (active) m = mn;
            const uint64_t word = __ballot(c);
            if (lane == 0) surv[s] = word;
        }
        uint32_t best = h;
#pragma unroll
        for (int d = 1; d < NS; d <<= 1) {
            const int32_t om = __shfl_xor(m, d);
            const uint32_t ob = (uint32_t)__shfl_xor((int)best, d);
            if (!conv_keeps(m, best, om, ob)) {
                m = om;
                best = ob;
            }
        }
        if (a.forced_end && win.a_hi == end) best = 0;
        __syncthreads();                           // the survivor words are written, the stage is read
        if (valid && h == 0) {
            uint32_t s = best;
            uint64_t out = 0;
            for (uint32_t i = WL; i-- > W;) {
                const uint64_t T = (uint64_t)(win.lo + (int64_t)i);          // i >= W: T >= j B
                if (T >= win.a_hi) continue;
                if (T < win.e_lo) break;
                uint32_t bit;
                s = conv_back(surv[i], gbase, s, K, bit);
                if (T < win.e_hi) {
                    const uint64_t k = T - a.first;
                    out |= (uint64_t)bit << (k & 63);
                    if ((k & 63) == 0 || T == win.e_lo) {
                        atomicOr(reinterpret_cast<unsigned long long *>(a.bits) + (k >> 6), (unsigned long long)out);
                        out = 0;
                    }
                }
            }
        }
    }
    if (a.stats && blockIdx.x == 0 && t == 0) {
        a.stats[0] += a.nblocks;
        a.stats[1] += a.ndecided;
    }
}

template <int NS, int N>
int launch(const ConvLaunch &a, int cus, hipStream_t st) {
    const ConvShape s = conv_shape(NS, N, a.geom);
    const uint64_t ngrp = (a.nblocks + s.wpg - 1) / s.wpg;
    const unsigned grid = (unsigned)std::min<uint64_t>(ngrp, (uint64_t)std::max(1, cus) * 16);
    conv_decode_kernel<NS, N><<<grid, s.threads, s.bytes, st>>>(a, s.wpg);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

template <int NS>
int launch_n(const ConvLaunch &a, int cus, hipStream_t st) {
    return a.n == 2 ? launch<NS, 2>(a, cus, st) : launch<NS, 3>(a, cus, st);
}

// ---- the encoder ---------------------------------------------------------------------------------------------------------------
constexpr int kConvEncodeThreads = 256;

// Output word wd holds the transmitted bits 64 wd .. 64 wd + 63 of the call, bit x of the record's stream: the period it lies
// in and its place there come from one division per word, the step and coded bit behind every place from the table.
__global__ __launch_bounds__(kConvEncodeThreads) void conv_encode_kernel(ConvEncodeLaunch a) {
    const uint32_t state = a.state ? *a.state : a.init_state;
    const uint64_t nwords = (a.nout + 63) / 64;
    for (uint64_t wd = (uint64_t)blockIdx.x * kConvEncodeThreads + threadIdx.x; wd < nwords; wd += (uint64_t)gridDim.x * kConvEncodeThreads) {
        const uint64_t x = a.idx_first + wd * 64;
        uint64_t period = x / a.punct.ptot;
        uint32_t place = (uint32_t)(x % a.punct.ptot);
        const uint32_t nb = (uint32_t)min((uint64_t)64, a.nout - wd * 64);
        uint64_t out = 0;
        for (uint32_t b = 0; b < nb; ++b) {
            const int64_t k = (int64_t)(period * a.punct.p + a.punct.inv_step[place] - a.first);
            const uint32_t bit = conv_parity(conv_in_window(a.bits, state, k, (int)a.K) & a.gen[a.punct.inv_bit[place]]);
            out |= (uint64_t)bit << b;
            if (++place == a.punct.ptot) {
                place = 0;
                ++period;
            }
        }
        a.out[wd] = out;
    }
}

// behind the encode kernel on the same stream: the state in front of first + nsteps
__global__ void conv_state_kernel(ConvEncodeLaunch a) {
    const uint32_t state = *a.state;
    uint32_t h = 0;
    for (uint32_t i = 0; i + 1 < a.K; ++i) h |= conv_in_bit(a.bits, state, (int64_t)a.nsteps - 1 - (int64_t)i) << i;
    *a.state = h;
}

}  // namespace

int conv_decode_launch(const ConvLaunch &a, int cus, hipStream_t st) {
    switch (a.K) {
    case 3: return launch_n<4>(a, cus, st);
    case 4: return launch_n<8>(a, cus, st);
    case 5: return launch_n<16>(a, cus, st);
    case 6: return launch_n<32>(a, cus, st);
    default: return launch_n<64>(a, cus, st);
    }
}

int conv_encode_launch(const ConvEncodeLaunch &a, hipStream_t st) {
    const uint64_t nwords = (a.nout + 63) / 64;
    const unsigned grid = (unsigned)std::min<uint64_t>((nwords + kConvEncodeThreads - 1) / kConvEncodeThreads, 1u << 20);
    conv_encode_kernel<<<grid, kConvEncodeThreads, 0, st>>>(a);
    BBB_HIP(hipGetLastError());
    if (a.state) {
        conv_state_kernel<<<1, 1, 0, st>>>(a);
        BBB_HIP(hipGetLastError());
    }
    return BBB_OK;
}

}  // namespace bbb
