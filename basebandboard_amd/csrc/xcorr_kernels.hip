// xcorr_kernels.hip -- exact correlation of int16 samples with their own data bits (include/bbb.h, "pulse response").
//
//   xc[l] += s[m] * x[n]   for every sample n of the call and lag l < nlags with n - origin - l = spb * m, m >= 0
//
// With u = n - origin, q = floor(u / spb), r = u mod spb: sample n adds s[q - j] x[n] to lag spb j + r for j < J =
// ceil(nlags / spb).  The per-lane core is xcorr_common.hpp: a lane owns one residue and XT lag groups (XT = 8 when J <= 8,
// 16 when J <= 16, else 32; row y of the grid takes groups [XT y, XT y + XT)), and walks kXcorrSteps consecutive q per tile.
//
// A workgroup of 256 lanes takes tiles of kXcorrTile = 8192 samples.  Tiles are cut where the sample pointer is 16-byte
// aligned, so that global reads are 16-byte loads whatever spb and the pointer's alignment are; a tile's first and last
// vector are read element by element where they cross the call's range.  Samples that do not count (outside the range, or
// below the origin) are staged as 0.  The tile lies in LDS cut into 256 / spb segments of 32 spb samples, one per group of
// spb lanes; a segment is followed by spb unused halfwords, which spreads the lanes of a wavefront over all banks (lane (c, s)
// reads halfword 33 spb s + spb t + c at step t).  Lanes flush into an int64 lag array in LDS (ds_add_u64) every 2^15
// steps (half of what their int32 partials could take) and at the end; the workgroup writes the array to its row of a slab with plain stores and a reduce launch adds the
// slab into the counters.
#include "bbb_common.hpp"
#include "xcorr_common.hpp"

#include <algorithm>
#include <mutex>

namespace bbb {

namespace {

constexpr int kXcorrLdsHalves = (kXcorrSteps + 1) * kXcorrThreads;
constexpr int kXcorrMaxLw = 32 * 32;                  // XT * spb at most
constexpr int kXcorrReduceOut = 8;

typedef short xcorr_i16x8 __attribute__((ext_vector_type(8)));

// ubase = first_sample - origin - a, with a = the samples before x[0] back to the 16-byte boundary (0..7): tile t holds
// samples i = kXcorrTile t - a + k (k < kXcorrTile) at u = ubase + kXcorrTile t + k
template <int XT>
__global__ void __launch_bounds__(kXcorrThreads)
xcorr_kernel(const int16_t *__restrict x, long long nsamples, long long ubase, unsigned a, unsigned spb_sh, unsigned nlags,
             const unsigned long long *__restrict bits, long long bit0, long long nwords, long long ntiles,
             unsigned long long *__restrict partials) {
    __shared__ __attribute__((aligned(16))) int16_t S[kXcorrLdsHalves];
    __shared__ unsigned long long Lg[kXcorrMaxLw];
    const unsigned tid = threadIdx.x;
    const unsigned spb = 1u << spb_sh, lw = (unsigned)XT << spb_sh;
    const unsigned c = tid & (spb - 1), s = tid >> spb_sh;
    const unsigned jbase = blockIdx.y * XT;
    const unsigned r = xcorr_floor_mod(ubase + c, spb_sh);           // kXcorrTile and a segment are multiples of spb
    const unsigned seg_sh = 5 + spb_sh;                               // a segment: kXcorrSteps * spb samples
    const int16_t *mine = S + xcorr_lds_index(xcorr_lane_sample(tid, 0, spb_sh), spb_sh);     // step t: + spb t

    for (unsigned i = tid; i < lw; i += kXcorrThreads) Lg[i] = 0;

    XcorrLane<XT> lane;
    lane.clear();
    bool masked_now = true;
    auto sink = [&](int j, long long v) {
        const unsigned lag = ((jbase + (unsigned)j) << spb_sh) + r;
        if (lag < nlags) atomicAdd(&Lg[((unsigned)j << spb_sh) + r], (unsigned long long)v);
    };

    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long ub = ubase + t * kXcorrTile, ib = t * kXcorrTile - (long long)a;
        if (ub + kXcorrTile <= 0) continue;                           // the whole tile lies below the origin
        __syncthreads();                                              // the previous tile is read (and Lg is cleared)
        for (unsigned g = tid; g < kXcorrTile / 8; g += kXcorrThreads) {
            const unsigned k = 8 * g;
            const long long i = ib + k;
            xcorr_i16x8 v;
            if (i >= 0 && i + 8 <= nsamples) {
                v = *reinterpret_cast<const xcorr_i16x8 *>(x + i);
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = (i + e >= 0 && i + e < nsamples) ? x[i + e] : (int16_t)0;
            }
            const long long u = ub + k;
            if (u < 0) {
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = u + e < 0 ? (short)0 : v[e];
            }
            const unsigned idx = xcorr_lds_index(k, spb_sh);
            if (spb_sh >= 3) {
                *reinterpret_cast<xcorr_i16x8 *>(S + idx) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 8; e++) S[idx + e] = v[e];
            }
        }
        __syncthreads();
        const long long q0 = xcorr_floor_div(ub + c + ((long long)s << seg_sh), spb_sh);
        xcorr_lane_tile<XT>(lane, masked_now, q0, jbase, bits, bit0, nwords,
                            [&](int step) { return (int)mine[(unsigned)step << spb_sh]; }, sink);
    }
    xcorr_flush(lane, masked_now, sink);
    __syncthreads();
    unsigned long long *out = partials + ((unsigned long long)blockIdx.y * gridDim.x + blockIdx.x) * lw;
    for (unsigned i = tid; i < lw; i += kXcorrThreads) out[i] = Lg[i];
}

// xc[o] += the slab: lag o lies in row y = o / lw of the grid at entry o - y lw.  A block takes 8 consecutive lags, 32
// threads per lag each summing every 32nd workgroup.  (The eye's and the ACF's reduce kernels fold uint32 partials and a
// 16-lag block layout with a sum entry: neither reads this slab.)
__global__ void __launch_bounds__(256)
xcorr_reduce_kernel(const unsigned long long *__restrict partials, unsigned gx, unsigned lw, unsigned nlags,
                    unsigned long long *__restrict xc) {
    __shared__ unsigned long long R[256];
    const unsigned ol = threadIdx.x % kXcorrReduceOut, sl = threadIdx.x / kXcorrReduceOut;
    const unsigned o = blockIdx.x * kXcorrReduceOut + ol;
    unsigned long long sum = 0;
    if (o < nlags) {
        const unsigned y = o / lw;
        const unsigned long long *p = partials + (unsigned long long)y * gx * lw + (o - y * lw);
        for (unsigned xb = sl; xb < gx; xb += 256 / kXcorrReduceOut) sum += p[(unsigned long long)xb * lw];
    }
    R[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x < kXcorrReduceOut && o < nlags) {
        unsigned long long t = 0;
        for (unsigned k = 0; k < 256 / kXcorrReduceOut; k++) t += R[k * kXcorrReduceOut + threadIdx.x];
        xc[o] += t;
    }
}

// the Pulser's data bits: bit m is 1 where (m & 255) == 0; word w holds bits first_bit + 64 w ..
__global__ void xcorr_pulser_bits_kernel(unsigned long long *dst, unsigned long long first_bit, unsigned long long nwords) {
    const unsigned long long w = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    const unsigned long long lo = first_bit + 64 * w;
    const unsigned long long next = (lo + 255) & ~255ull;             // the first multiple of 256 at or above lo
    dst[w] = next - lo < 64 ? 1ull << (next - lo) : 0ull;
}

unsigned spb_shift(uint32_t spb) {
    unsigned sh = 0;
    while ((1u << sh) < spb) sh++;
    return sh;
}

// what the grid is sized by on a device, queried once: compute units and resident workgroups per unit of the three kernels
struct XcorrDevice {
    int cus = 0, occ[3] = {0, 0, 0};              // XT 8, 16, 32
    bool ok = false;
};

template <int XT>
int per_cu() {
    int n = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, xcorr_kernel<XT>, kXcorrThreads, 0) == hipSuccess ? n : -1;
}

const XcorrDevice *device_info() {
    static std::mutex mu;
    static XcorrDevice info[64];
    static bool tried[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!tried[dev]) {
        XcorrDevice d;
        d.occ[0] = per_cu<8>(), d.occ[1] = per_cu<16>(), d.occ[2] = per_cu<32>();
        d.ok = hipDeviceGetAttribute(&d.cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && d.occ[0] > 0 &&
               d.occ[1] > 0 && d.occ[2] > 0;
        if (!d.ok) return nullptr;                // not remembered: the next call asks again
        info[dev] = d;
        tried[dev] = true;
    }
    return &info[dev];
}

}  // namespace

XcorrPlan xcorr_plan(uint32_t spb, uint32_t nlags, uint64_t max_nsamples) {
    XcorrPlan p{};
    const uint32_t J = (nlags + spb - 1) / spb;
    p.xt = J <= 8 ? 8 : J <= 16 ? 16 : 32;
    p.gy = (int)((J + p.xt - 1) / p.xt);
    p.lw = (uint32_t)p.xt * spb;
    const XcorrDevice *d = device_info();
    if (!d) {
        p.gx = -1;
        return p;
    }
    const int cus = d->cus, occ = d->occ[p.xt == 8 ? 0 : p.xt == 16 ? 1 : 2];
    const uint64_t ntiles = std::max<uint64_t>(1, (max_nsamples + 7 + kXcorrTile - 1) / kXcorrTile);
    const uint64_t want = std::max<uint64_t>(1, (uint64_t)std::max(cus, 1) * std::max(occ, 1) / p.gy);
    p.gx = (int)std::min<uint64_t>(ntiles, want);
    p.scratch_words = (uint64_t)p.gx * p.gy * p.lw;
    return p;
}

int xcorr_launch(const XcorrPlan &p, const XcorrLaunch &l, uint64_t *scratch, int64_t *xc, hipStream_t st) {
    if (l.nsamples == 0) return BBB_OK;
    const unsigned a = (unsigned)(((uintptr_t)l.samples >> 1) & 7);
    const uint64_t ntiles = (l.nsamples + a + kXcorrTile - 1) / kXcorrTile;
    const unsigned gx = (unsigned)std::min<uint64_t>((uint64_t)p.gx, ntiles);
    const long long ubase = (long long)l.first_sample - (long long)l.origin - (long long)a;
    const long long nwords = (long long)((l.nbits + 63) / 64);
    const unsigned sh = spb_shift(l.spb);
    unsigned long long *part = reinterpret_cast<unsigned long long *>(scratch);
    const auto *bits = reinterpret_cast<const unsigned long long *>(l.bits);
    const dim3 grid(gx, (unsigned)p.gy);
    if (p.xt == 8)
        xcorr_kernel<8><<<grid, kXcorrThreads, 0, st>>>(l.samples, (long long)l.nsamples, ubase, a, sh, l.nlags, bits,
                                                        (long long)l.bit0, nwords, (long long)ntiles, part);
    else if (p.xt == 16)
        xcorr_kernel<16><<<grid, kXcorrThreads, 0, st>>>(l.samples, (long long)l.nsamples, ubase, a, sh, l.nlags, bits,
                                                         (long long)l.bit0, nwords, (long long)ntiles, part);
    else
        xcorr_kernel<32><<<grid, kXcorrThreads, 0, st>>>(l.samples, (long long)l.nsamples, ubase, a, sh, l.nlags, bits,
                                                         (long long)l.bit0, nwords, (long long)ntiles, part);
    BBB_HIP(hipGetLastError());
    xcorr_reduce_kernel<<<(l.nlags + kXcorrReduceOut - 1) / kXcorrReduceOut, 256, 0, st>>>(
        part, gx, p.lw, l.nlags, reinterpret_cast<unsigned long long *>(xc));
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

int xcorr_pulser_bits_launch(uint64_t *dst, uint64_t first_bit, uint64_t nwords, hipStream_t st) {
    if (nwords == 0) return BBB_OK;
    xcorr_pulser_bits_kernel<<<(unsigned)((nwords + 255) / 256), 256, 0, st>>>(reinterpret_cast<unsigned long long *>(dst),
                                                                              first_bit, nwords);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
