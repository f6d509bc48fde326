// mlse_kernels.hip -- the exact Viterbi sequence detector over int16 samples (include/bbb.h, bbb_mlse_run).
//
// Block j of B symbols is decided by one Viterbi run over its window, the W symbols in front of it and the D behind it
// included (mlse_common.hpp has the arithmetic); windows do not depend on one another, so they are handed out freely.
// NS = 2^mem lanes own one window, one lane per state: a wave holds 64 / NS windows, a workgroup threads / NS consecutive
// ones.  Per workgroup:
//   * all threads produce the y of the workgroup's whole span of symbols into LDS, step by step through fir_common.hpp's
//     image and fir_point, exactly as bbb_fir_filter forms its int16 output; y never reaches memory;
//   * every wave walks the symbols of its windows in lockstep.  A lane fetches the metrics of its state's two predecessors
//     with two cross-lane moves (mlse_fetch), adds the two gains (constants of the lane times y), keeps the larger; the 64
//     survivor bits of the wave are one ballot, one u64 per symbol in LDS;
//   * the NS lanes of a window agree on the end state through a butterfly, and the window's lane 0 walks the survivor words
//     back, packs the block's decisions and ORs them into the zeroed output (blocks share words).
// One lane per window, the other form, needs 2 bytes of survivors per symbol and LANE, 512 bytes per lane at the default
// window, besides the y: a compute unit's 160 KiB hold fewer than 200 such lanes, less than one wave per SIMD.  Here a
// wave's survivors are 8 bytes per symbol whatever NS is.
#include "mlse_launch.hpp"
#include "fir_common.hpp"

#include <algorithm>

namespace bbb {
namespace {

constexpr size_t kMlseLdsTarget = 40 * 1024;       // four workgroups in a compute unit's 160 KiB
constexpr size_t kMlseImageBytes = (size_t)kFirLdsWords * 4;
static_assert(kMlseImageBytes % 16 == 0, "the survivor words behind the image are aligned");

// LDS of a workgroup: the image, WL survivor words per wave, the y of wpg B + W + D symbols
struct MlseShape {
    uint32_t threads, wpg, span;
    size_t bytes;
};
MlseShape mlse_shape(uint32_t ns, const MlseGeom &g) {
    MlseShape s{};
    for (uint32_t threads = 256; threads >= (uint32_t)kWave; threads /= 2) {
        s.threads = threads;
        s.wpg = threads / ns;
        s.span = s.wpg * g.B + g.W + g.D;
        s.bytes = (kMlseImageBytes + (size_t)(threads / kWave) * (g.B + g.W + g.D) * 8 + 2 * (size_t)s.span + 15) & ~(size_t)15;
        if (s.bytes <= kMlseLdsTarget) break;
    }
    return s;                                      // 64 threads: at most 4624 + 4096 + 2 * (32 * 512 + 256) < 42 KiB
}

// The metric of predecessor C of every lane's state: lane src of the lane's own group of NS.  Up to four states the group lies
// inside a quad and the move is a DPP quad permutation, VALU latency and no LDS traffic (lane q of a quad reads lane
// {0, 0, 2, 2}[q] for C = 0 and {1, 1, 3, 3}[q] for C = 1 at NS = 2, {0, 0, 1, 1}[q] and {2, 2, 3, 3}[q] at NS = 4: mlse_pred
// spelt out); above that it is ds_bpermute_b32.  Every lane of the wave is active where this is called.
template <int NS, int C>
__device__ __forceinline__ int64_t mlse_fetch(int64_t m, int src) {
    if constexpr (NS <= 4) {
        constexpr int ctrl = NS == 2 ? (C ? 0xF5 : 0xA0) : (C ? 0xFA : 0x50);
        static_assert(NS != 2 || (mlse_pred(1, 0, 1) == 0 && mlse_pred(0, 1, 1) == 1), "the quad permutation is mlse_pred's");
        static_assert(NS != 4 || (mlse_pred(3, 0, 2) == 1 && mlse_pred(1, 1, 2) == 2), "the quad permutation is mlse_pred's");
        const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(uint64_t)m, ctrl, 0xF, 0xF, true);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)((uint64_t)m >> 32), ctrl, 0xF, 0xF, true);
        return (int64_t)((uint64_t)hi << 32 | lo);
    } else {
        return __shfl((long long)m, src);
    }
}

template <int NS, int THREADS>
__global__ __launch_bounds__(THREADS) void mlse_kernel(MlseLaunch a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int L = NS == 2 ? 1 : NS == 4 ? 2 : NS == 8 ? 3 : 4;
    constexpr int nthr = THREADS, PER = kFirThreads / THREADS;        // PER: the 8-sample pieces of a step that a thread stages
    constexpr int AHEAD = THREADS == 64 ? 2 : 3;                      // steps whose samples are in flight at once
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave, ng = (int)a.ngroups;
    const uint32_t B = a.geom.B, W = a.geom.W, D = a.geom.D, WL = B + W + D, wpg = (uint32_t)nthr / NS;
    uint32_t *img = reinterpret_cast<uint32_t *>(lds);
    uint64_t *surv = reinterpret_cast<uint64_t *>(lds + kMlseImageBytes) + (size_t)w * WL;          // this wave's
    int16_t *ys = reinterpret_cast<int16_t *>(lds + kMlseImageBytes + (size_t)(nthr / kWave) * WL * 8);
    const uint32_t h = (uint32_t)lane & (NS - 1), gbase = (uint32_t)lane & ~(uint32_t)(NS - 1);
    const MlseLane rule = mlse_lane(a.g, L, h);
    const int src0 = (int)(gbase | mlse_pred(h, 0, L)), src1 = (int)(gbase | mlse_pred(h, 1, L));
    const uint64_t ngrp = (a.nblocks + wpg - 1) / wpg, end = a.first + a.nsym;
    for (uint64_t grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
        const uint64_t jg = a.j0 + grp * wpg;
        const uint32_t nwin = (uint32_t)min((uint64_t)wpg, a.j0 + a.nblocks - jg);
        // the span: the symbols from the first window's first to the last window's last, index K - lo_u of ys
        const int64_t lo_u = (int64_t)(jg * B) - (int64_t)W;
        const uint64_t K_lo = lo_u > 0 ? (uint64_t)lo_u : 0, K_hi = min(end, (jg + nwin) * B + D);
        const int64_t q_lo = (int64_t)K_lo - (int64_t)a.first, q_hi = (int64_t)K_hi - (int64_t)a.first;   // counted from the call's first
        const int64_t n_lo = (int64_t)a.phase + q_lo * (int64_t)a.decim, n_last = (int64_t)a.phase + (q_hi - 1) * (int64_t)a.decim;
        // The span's steps, AHEAD at a time: a workgroup has few threads and a step is one round trip to memory, so the samples
        // of AHEAD steps are requested together and then staged and filtered one step after the other.
        for (int64_t base0 = n_lo & ~7ll; base0 <= n_last; base0 += AHEAD * kFirTile) {
            uint4 own[AHEAD][PER], lead[AHEAD];
#pragma unroll
            for (int p = 0; p < AHEAD; ++p) {
                const int64_t base = base0 + p * kFirTile;
                if (base <= n_last) {
#pragma unroll
                    for (int k = 0; k < PER; ++k) own[p][k] = fir_load8(a, base + 8 * (t + k * nthr));
                    lead[p] = t < ng ? fir_load8(a, base - 8 * (t + 1)) : make_uint4(0, 0, 0, 0);
                }
            }
#pragma unroll
            for (int p = 0; p < AHEAD; ++p) {
                const int64_t base = base0 + p * kFirTile;
                if (base > n_last) continue;       // (the same for every thread)
                __syncthreads();                   // the image's and, in the first step, the span's readers are done
#pragma unroll
                for (int k = 0; k < PER; ++k) *reinterpret_cast<uint4 *>(img + kFirHist / 2 + 4 * (t + k * nthr)) = own[p][k];
                if (t < ng) *reinterpret_cast<uint4 *>(img + kFirHist / 2 - 4 * (t + 1)) = lead[p];
                __syncthreads();
                const int64_t s_lo = max(q_lo, mlse_ceil_div(base - (int64_t)a.phase, a.decim));
                const int64_t s_hi = min(q_hi, mlse_ceil_div(base + kFirTile - (int64_t)a.phase, a.decim));
                for (int64_t q = s_lo + t; q < s_hi; q += nthr) {
                    int acc[1];
                    const uint32_t *const im[1] = {img};
                    fir_point(im, (int)((int64_t)a.phase + q * (int64_t)a.decim - base) + kFirHist - 1, ng, a.taps, acc);
                    ys[q + (int64_t)a.first - lo_u] = (int16_t)sat16(acc[0] >> a.shift);
                }
            }
        }
        __syncthreads();
        // the windows: window wi of the workgroup starts at ys[wi B]
        const uint32_t wi = (uint32_t)w * (kWave / NS) + (uint32_t)lane / NS;
        const bool valid = wi < nwin;
        const MlseWindow win = mlse_window(a.geom, jg + wi, a.first, a.nsym, a.ndecided);
        const int16_t *yw = ys + (size_t)wi * B;   // (a window beyond nwin reads inside the span's allocation and decides nothing)
        int64_t m = mlse_start(win.from_zero, h, a.init_state);
        for (uint32_t s = 0; s < WL; ++s) {
            const int64_t K = win.lo + (int64_t)s;
            const bool active = valid && K >= (int64_t)win.a_lo && K < (int64_t)win.a_hi;
            const int64_t m0 = mlse_fetch<NS, 0>(m, src0), m1 = mlse_fetch<NS, 1>(m, src1);
            uint32_t c;
            const int64_t mn = mlse_acs(rule, yw[s], m0, m1, c);
            if (active) m = mn;
            const uint64_t word = __ballot(c);
            if (lane == 0) surv[s] = word;
        }
        uint32_t best = h;
#pragma unroll
        for (int d = 1; d < NS; d <<= 1) {
            const int64_t om = __shfl_xor((long long)m, d);
            const uint32_t ob = (uint32_t)__shfl_xor((int)best, d);
            if (!mlse_keeps(m, best, om, ob)) {
                m = om;
                best = ob;
            }
        }
        __syncthreads();                           // the survivor words are written, the span is read
        if (valid && h == 0) {
            uint32_t s = best;
            uint64_t out = 0;
            for (uint32_t i = WL; i-- > W;) {
                const uint64_t K = (uint64_t)(win.lo + (int64_t)i);          // i >= W: K >= j B
                if (K >= win.a_hi) continue;
                if (K < win.e_lo) break;
                uint32_t bit;
                s = mlse_back(surv[i], gbase, s, L, bit);
                if (K < win.e_hi) {
                    const uint64_t k = K - a.first;
                    out |= (uint64_t)bit << (k & 63);
                    if ((k & 63) == 0 || K == win.e_lo) {
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

template <int NS>
int launch(const MlseLaunch &a, int cus, hipStream_t st) {
    const MlseShape s = mlse_shape(NS, a.geom);
    const uint64_t ngrp = (a.nblocks + s.wpg - 1) / s.wpg;
    const unsigned grid = (unsigned)std::min<uint64_t>(ngrp, (uint64_t)std::max(1, cus) * 16);
    if (s.threads == 256) mlse_kernel<NS, 256><<<grid, 256, s.bytes, st>>>(a);
    else if (s.threads == 128) mlse_kernel<NS, 128><<<grid, 128, s.bytes, st>>>(a);
    else mlse_kernel<NS, 64><<<grid, 64, s.bytes, st>>>(a);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace

int mlse_launch(const MlseLaunch &a, int cus, hipStream_t st) {
    switch (a.mem) {
    case 1: return launch<2>(a, cus, st);
    case 2: return launch<4>(a, cus, st);
    case 3: return launch<8>(a, cus, st);
    default: return launch<16>(a, cus, st);
    }
}

}  // namespace bbb
