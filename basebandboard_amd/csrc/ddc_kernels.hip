// ddc_kernels.hip -- the digital down-converter: quadrature mixer, two exact FIR filters, I/Q or polar outputs
// (include/bbb.h, bbb_ddc_run).
//
//   mi(n), mq(n) = x(n) times the local oscillator's cosine and minus sine (ddc_common.hpp), a function of the absolute
//                  sample number first_sample + n alone: no oscillator state exists
//   ai(n) = sum_{i < ntaps} h[i] mi(n - i)      aq(n) likewise      I[q] = sat16(ai(phase + q decim) >> shift), Q[q] likewise
// The workgroup step is fir_kernel's: 2048 inputs and the 8 * ngroups samples in front of them, loaded one step ahead
// (fir_load8).  The mixer runs between the load and LDS: a thread looks up c and s of its 8 samples in its replica of the
// ROM (nco_common.hpp: the NCO's 16 bank-rotated replicas, filled once per workgroup from the kernel's arguments), multiplies,
// shifts and writes the I and the Q image in fir_common.hpp's geometry.  The raw samples never reach LDS, and nothing but
// outputs reaches memory.  Two pairs of images alternate, so a step costs one barrier.
// Block form (decim = 1): fir_block8 on each image gives a thread the 8 (I, Q) pairs n0 .. n0 + 7: 32 or 64 contiguous bytes.
// Point form (decim > 1): fir_point over both images gives a thread one pair: one 4- or 8-byte store.
// POLAR is a register epilogue on the IQ16 pair (ddc_polar).
// LDS: 4 images of 4624 B + 16 ROM replicas of 2052 B = 51328 B, three workgroups per CU (kDdcWgPerCu).
#include "bbb_common.hpp"
#include "ddc_common.hpp"
#include "fir_common.hpp"
#include "nco_common.hpp"

#include <algorithm>

namespace bbb {
namespace {

constexpr int kDdcLdsBytes = 4 * (4 * kFirLdsWords + kNcoLdsWords);
constexpr int kDdcWgPerCu = 160 * 1024 / kDdcLdsBytes;               // what a CU's 160 KiB of LDS hold at once

// the I and Q image words of the samples j0 .. j0 + 7 (raw: fir_load8's four dwords; jabs: the absolute number of j0)
__device__ __forceinline__ void mix8(const DdcLaunch &a, const int16_t *rom_l, const uint4 &raw, uint32_t jabs, uint4 &wi, uint4 &wq) {
    const uint32_t r[4] = {raw.x, raw.y, raw.z, raw.w};
    uint32_t mi[8], mq[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int x = (int)(int16_t)(r[k >> 1] >> (16 * (k & 1)));
        const uint32_t adr = ddc_adr(a.pa0, a.fcw, jabs + (uint32_t)k);
        int vi, vq;
        ddc_mix(x, rom_l[(adr + 256u) & 1023u], rom_l[adr], vi, vq);
        mi[k] = (uint32_t)vi & 0xFFFFu;
        mq[k] = (uint32_t)vq & 0xFFFFu;
    }
    wi = make_uint4(mi[0] | mi[1] << 16, mi[2] | mi[3] << 16, mi[4] | mi[5] << 16, mi[6] | mi[7] << 16);
    wq = make_uint4(mq[0] | mq[1] << 16, mq[2] | mq[3] << 16, mq[4] | mq[5] << 16, mq[6] | mq[7] << 16);
}

// one output pair of MODE 0 (IQ16) or 2 (POLAR) as its 4-byte element
template <int MODE>
__device__ __forceinline__ uint32_t pair16(int ai, int aq, uint32_t shift) {
    const int i = sat16(ai >> shift), q = sat16(aq >> shift);
    if constexpr (MODE == 2) {
        uint32_t mag;
        int ph;
        ddc_polar(i, q, mag, ph);
        return (mag & 0xFFFFu) | (uint32_t)ph << 16;
    } else {
        return ((uint32_t)i & 0xFFFFu) | (uint32_t)q << 16;
    }
}

// MODE 0: IQ16, 1: IQ32, 2: POLAR.  POINT: the kernel for decim > 1.
template <int MODE, bool POINT>
__global__ __launch_bounds__(kFirThreads) void ddc_kernel(DdcLaunch a) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[2][2][kFirLdsWords];
    __shared__ uint32_t rom_lds[kNcoLdsWords];
    const int t = threadIdx.x;
    const int16_t *rom_l = nco_rom_to_lds(a.rom, rom_lds);
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
        uint32_t *LI = lds[par][0], *LQ = lds[par][1];
        const uint32_t jbase = a.first + (uint32_t)base;              // modulo 2^32: the low 24 bits are what counts
        uint4 wi, wq;
        mix8(a, rom_l, cur, jbase + 8u * (uint32_t)t, wi, wq);
        *reinterpret_cast<uint4 *>(LI + kFirHist / 2 + 4 * t) = wi;
        *reinterpret_cast<uint4 *>(LQ + kFirHist / 2 + 4 * t) = wq;
        if (t < ng) {
            mix8(a, rom_l, cur_lead, jbase - 8u * (uint32_t)(t + 1), wi, wq);
            *reinterpret_cast<uint4 *>(LI + kFirHist / 2 - 4 * (t + 1)) = wi;
            *reinterpret_cast<uint4 *>(LQ + kFirHist / 2 - 4 * (t + 1)) = wq;
        }
        cur = nxt;
        cur_lead = nxt_lead;
        __syncthreads();
        if constexpr (!POINT) {
            const uint64_t n0 = base + 8 * t;
            if (n0 >= a.nin) continue;
            int ai[8], aq[8];
            fir_block8(LI, t, ng, a.taps, ai);
            fir_block8(LQ, t, ng, a.taps, aq);
            const int nv = (int)min((uint64_t)8, a.nin - n0);           // outputs of this thread inside the record
            if constexpr (MODE == 1) {
                int32_t *out = reinterpret_cast<int32_t *>(a.out) + 2 * n0;
                if (a.out_vec && nv == 8) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        reinterpret_cast<int4 *>(out)[k] = make_int4(ai[2 * k] >> a.shift, aq[2 * k] >> a.shift, ai[2 * k + 1] >> a.shift, aq[2 * k + 1] >> a.shift);
                } else {
#pragma unroll
                    for (int r = 0; r < 8; ++r)
                        if (r < nv) reinterpret_cast<int2 *>(out)[r] = make_int2(ai[r] >> a.shift, aq[r] >> a.shift);
                }
            } else {
                uint32_t *out = reinterpret_cast<uint32_t *>(a.out) + n0;
                uint32_t w[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) w[r] = pair16<MODE>(ai[r], aq[r], a.shift);
                if (a.out_vec && nv == 8) {
                    reinterpret_cast<uint4 *>(out)[0] = make_uint4(w[0], w[1], w[2], w[3]);
                    reinterpret_cast<uint4 *>(out)[1] = make_uint4(w[4], w[5], w[6], w[7]);
                } else {
#pragma unroll
                    for (int r = 0; r < 8; ++r)
                        if (r < nv) out[r] = w[r];
                }
            }
        } else {
            // the outputs whose input index lies in this step: q_lo <= q < q_hi
            const uint64_t end = base + kFirTile;
            const uint64_t q_lo = base <= a.phase ? 0 : (base - a.phase + a.decim - 1) / a.decim;
            const uint64_t q_hi = end <= a.phase ? 0 : min(a.nout, (end - a.phase + a.decim - 1) / a.decim);
            for (uint64_t q = q_lo + (uint64_t)t; q < q_hi; q += kFirThreads) {
                const int l0 = (int)(a.phase + q * a.decim - base) + kFirHist - 1;         // the lower sample of pair 0
                const uint32_t *const img[2] = {LI, LQ};
                int acc[2];
                fir_point(img, l0, ng, a.taps, acc);                                        // the two chains interleave
                if constexpr (MODE == 1) reinterpret_cast<int2 *>(a.out)[q] = make_int2(acc[0] >> a.shift, acc[1] >> a.shift);
                else reinterpret_cast<uint32_t *>(a.out)[q] = pair16<MODE>(acc[0], acc[1], a.shift);
            }
        }
    }
}

template <int MODE>
void launch_mode(const DdcLaunch &a, unsigned g, hipStream_t st) {
    if (a.decim == 1) ddc_kernel<MODE, false><<<g, kFirThreads, 0, st>>>(a);
    else ddc_kernel<MODE, true><<<g, kFirThreads, 0, st>>>(a);
}

}  // namespace

int ddc_launch(const DdcLaunch &a, int mode, int cus, hipStream_t st) {
    const uint64_t nsteps = (a.nin + kFirTile - 1) / kFirTile;
    const unsigned g = (unsigned)std::min<uint64_t>(nsteps, (uint64_t)std::max(1, cus) * kDdcWgPerCu);   // one resident round
    if (mode == 0) launch_mode<0>(a, g, st);
    else if (mode == 1) launch_mode<1>(a, g, st);
    else launch_mode<2>(a, g, st);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
