// nco_kernels.hip -- the numerically controlled oscillator (gateware/bbb/nco.py:25-44; include/bbb.h, bbb_nco_*).
//
// The module's registers, clocked once per sample t (fm, am, pm each a constant or a buffer):
//   adr(t) = ((pa >> 14) + pm(t)) mod 1024        pa' = (pa + fcw + fm(t)) mod 2^24
//   q' = rom[adr(t)]    w' = q    y' = am(t) * w    x(t) = y >> 16
// From a state (pa0, q0, w0, y0) at the start of a launch, with R(j) = rom[adr(j)] for j >= 0, R(-1) = q0, R(-2) = w0:
//   x(0) = y0 >> 16,   x(k) = (am(k - 1) * R(k - 3)) >> 16 for k >= 1,   pa(j) = pa0 + sum_{s < j} (fcw + fm(s)) mod 2^24,
// and the state after n clocks is pa(n), q = R(n - 1), w = R(n - 2), y = am(n - 1) * R(n - 3).
// Every thread owns 8 consecutive samples j0 .. j0 + 7 (j0 a multiple of 8) and computes R(j0 - 3) .. R(j0 + 7) and
// am(j0 - 1) .. am(j0 + 7) itself, so that no thread waits on another; the look-behind loads hit the cache lines the
// neighbouring thread has just read.  The state lives in two device slots: a launch reads one and writes the other.
#include "bbb_common.hpp"
#include "nco_common.hpp"

namespace bbb {
namespace {

constexpr int kPer = 8;                               // samples per thread and step: one 16-byte store of x
constexpr int kStep = kNcoThreads * kPer;             // samples per workgroup and step
constexpr int kScanTile = kStep * kNcoScanSteps;      // samples per tile of the fm scan
constexpr uint32_t kMask24 = 0xFFFFFFu;

// 8 consecutive values from p[j0 ..], zero beyond n; one 16-byte load when all 8 exist and the buffers are aligned
template <typename T>
__device__ inline void load8(const T *p, uint64_t j0, uint64_t n, bool vec, T v[kPer]) {
    if (vec && j0 + kPer <= n) {
        if constexpr (sizeof(T) == 2) {
            const uint4 u = *reinterpret_cast<const uint4 *>(p + j0);
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int k = 0; k < kPer; ++k) v[k] = (T)(uint16_t)(w[k >> 1] >> (16 * (k & 1)));
        } else {
            const uint4 a = *reinterpret_cast<const uint4 *>(p + j0), b = *reinterpret_cast<const uint4 *>(p + j0 + 4);
            v[0] = (T)a.x; v[1] = (T)a.y; v[2] = (T)a.z; v[3] = (T)a.w;
            v[4] = (T)b.x; v[5] = (T)b.y; v[6] = (T)b.z; v[7] = (T)b.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kPer; ++k) v[k] = j0 + k < n ? p[j0 + k] : T(0);
    }
}

// The outputs of one thread's 8 samples and, from the thread that owns sample n - 1, the state after the launch.
// pa[k] = pa(j0 - 3 + k) for k = 0 .. 11 (the low 24 bits count); the entries of positions below 0 are not read.
template <bool AM, bool PM>
__device__ inline void nco_group(const NcoLaunch &a, const int16_t *rom_l, const bbb_nco_state &s0, uint64_t j0,
                                 const uint32_t pa[12]) {
    int32_t pm[11];     // pm(j0 - 3 .. j0 + 7)
    int32_t am[9];      // am(j0 - 1 .. j0 + 7)
    if constexpr (PM) {
        int16_t v[kPer];
        load8(a.pm, j0, a.n, a.vec, v);
#pragma unroll
        for (int k = 0; k < kPer; ++k) pm[3 + k] = v[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) pm[k] = j0 ? a.pm[j0 - 3 + k] : 0;
    } else {
#pragma unroll
        for (int k = 0; k < 11; ++k) pm[k] = a.pm_c;
    }
    if constexpr (AM) {
        uint16_t v[kPer];
        load8(a.am, j0, a.n, a.vec, v);
#pragma unroll
        for (int k = 0; k < kPer; ++k) am[1 + k] = v[k];
        am[0] = j0 ? a.am[j0 - 1] : 0;
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) am[k] = (int32_t)a.am_c;
    }
    int32_t r[11];      // R(j0 - 3 .. j0 + 7)
#pragma unroll
    for (int k = 0; k < 11; ++k) r[k] = rom_l[((pa[k] >> 14) + (uint32_t)pm[k]) & 1023u];
    if (j0 == 0) {
        r[1] = s0.w;
        r[2] = s0.q;
    }
    int32_t y[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) y[k] = am[k] * r[k];          // |y| <= 65535 * 32768 < 2^31
    if (j0 == 0) y[0] = s0.y;
    if (a.vec && j0 + kPer <= a.n) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = (uint32_t)(uint16_t)(y[2 * k] >> 16) | (uint32_t)(y[2 * k + 1] >> 16) << 16;
        *reinterpret_cast<uint4 *>(a.x + j0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kPer; ++k)
            if (j0 + k < a.n) a.x[j0 + k] = (int16_t)(y[k] >> 16);
    }
    if (j0 < a.n && a.n - j0 <= kPer) {                        // this thread owns sample n - 1
        const int i = (int)(a.n - 1 - j0);
        bbb_nco_state s{};
        // compile-time indices only: a run-time index into pa / r / y would put the arrays in scratch for every thread
#pragma unroll
        for (int k = 0; k < kPer; ++k)
            if (k == i) {
                s.pa = pa[k + 4] & kMask24;
                s.q = r[k + 3];
                s.w = r[k + 2];
                s.y = y[k + 1];
            }
        *a.out = s;
    }
}

// Constant fm: pa(j) = pa0 + j * inc, exact mod 2^24 in 32-bit arithmetic.  A grid-stride loop over steps of kStep samples.
template <bool AM, bool PM>
__global__ __launch_bounds__(kNcoThreads) void nco_const_kernel(NcoLaunch a) {
    __shared__ uint32_t lds[kNcoLdsWords];
    const int16_t *rom_l = nco_rom_to_lds(a.rom, lds);
    const bbb_nco_state s0 = *a.in;
    const uint32_t inc = a.fcw + (uint32_t)a.fm_c;
    const uint64_t nsteps = (a.n + kStep - 1) / kStep;
    for (uint64_t s = blockIdx.x; s < nsteps; s += gridDim.x) {
        const uint64_t j0 = s * kStep + (uint64_t)threadIdx.x * kPer;
        if (j0 >= a.n) continue;
        uint32_t pa[12];
        const uint32_t b = s0.pa + (uint32_t)j0 * inc;
#pragma unroll
        for (int k = 0; k < 12; ++k) pa[k] = b + (uint32_t)(k - 3) * inc;
        nco_group<AM, PM>(a, rom_l, s0, j0, pa);
    }
}

__device__ inline uint32_t fm_inc_sum(const NcoLaunch &a, uint64_t j0, uint32_t inc[kPer]) {
    int32_t f[kPer];
    load8(a.fm, j0, a.n, a.vec, f);
    uint32_t t = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        inc[k] = j0 + k < a.n ? a.fcw + (uint32_t)f[k] : 0u;
        t += inc[k];
    }
    return t;
}

// Per-sample fm, pass 1: tiles[t] = sum of fcw + fm(s) over tile t (uint32; only its low 24 bits will count).
__global__ __launch_bounds__(kNcoThreads) void nco_tile_sums_kernel(NcoLaunch a, uint32_t ntiles) {
    __shared__ uint32_t part[kNcoThreads / kWave];
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        uint32_t sum = 0, inc[kPer];
        for (int st = 0; st < kNcoScanSteps; ++st)
            sum += fm_inc_sum(a, (uint64_t)t * kScanTile + (uint64_t)st * kStep + threadIdx.x * kPer, inc);
#pragma unroll
        for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
        if (threadIdx.x % kWave == 0) part[threadIdx.x / kWave] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t tot = 0;
            for (int w = 0; w < kNcoThreads / kWave; ++w) tot += part[w];
            a.tiles[t] = tot;
        }
        __syncthreads();
    }
}

// Pass 2, one workgroup: tiles[t] = pa0 + the exclusive prefix sum of the tile sums, in place.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void nco_tile_scan_kernel(NcoLaunch a, uint32_t ntiles) {
    __shared__ uint32_t wsum[kScanThreads / kWave];
    const uint32_t per = (ntiles + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = min(ntiles, threadIdx.x * per), hi = min(ntiles, lo + per);
    uint32_t own = 0;
    for (uint32_t i = lo; i < hi; ++i) own += a.tiles[i];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    uint32_t incl = own;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == kWave - 1) wsum[wave] = incl;
    __syncthreads();
    uint32_t run = a.in->pa + incl - own;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t v = a.tiles[i];
        a.tiles[i] = run;
        run += v;
    }
}

// Pass 3: each tile re-reads its fm (from the Infinity Cache: the host keeps a launch's fm within it), scans it within the
// workgroup from the tile's offset, and writes x.
template <bool AM, bool PM>
__global__ __launch_bounds__(kNcoThreads) void nco_scan_kernel(NcoLaunch a, uint32_t ntiles) {
    __shared__ uint32_t lds[kNcoLdsWords];
    __shared__ uint32_t wsum[2][kNcoThreads / kWave];
    const int16_t *rom_l = nco_rom_to_lds(a.rom, lds);
    const bbb_nco_state s0 = *a.in;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    int par = 0;
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        uint32_t carry = a.tiles[t];
        for (int st = 0; st < kNcoScanSteps; ++st, par ^= 1) {
            const uint64_t j0 = (uint64_t)t * kScanTile + (uint64_t)st * kStep + threadIdx.x * kPer;
            uint32_t inc[kPer];
            const uint32_t own = fm_inc_sum(a, j0, inc);
            uint32_t incl = own;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t v = __shfl_up(incl, o);
                if (lane >= o) incl += v;
            }
            if (lane == kWave - 1) wsum[par][wave] = incl;
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kNcoThreads / kWave; ++w) {
                const uint32_t v = wsum[par][w];
                before += w < wave ? v : 0u;
                total += v;
            }
            if (j0 < a.n) {
                uint32_t pa[12];
                pa[3] = carry + before + incl - own;
#pragma unroll
                for (int k = 0; k < kPer; ++k) pa[4 + k] = pa[3 + k] + inc[k];
                if (j0) {
#pragma unroll
                    for (int k = 2; k >= 0; --k) pa[k] = pa[k + 1] - (a.fcw + (uint32_t)a.fm[j0 - 3 + k]);
                } else {
                    pa[0] = pa[1] = pa[2] = 0;
                }
                nco_group<AM, PM>(a, rom_l, s0, j0, pa);
            }
            carry += total;
        }
    }
}

template <bool AM, bool PM>
int launch_form(const NcoLaunch &a, int grid, hipStream_t st) {
    if (!a.fm) {
        const uint64_t nsteps = (a.n + kStep - 1) / kStep;
        nco_const_kernel<AM, PM><<<(unsigned)std::min<uint64_t>(nsteps, grid), kNcoThreads, 0, st>>>(a);
    } else {
        const uint32_t ntiles = (uint32_t)((a.n + kScanTile - 1) / kScanTile);
        const unsigned g = std::min<uint32_t>(ntiles, (uint32_t)grid);
        nco_tile_sums_kernel<<<g, kNcoThreads, 0, st>>>(a, ntiles);
        nco_tile_scan_kernel<<<1, kScanThreads, 0, st>>>(a, ntiles);
        nco_scan_kernel<AM, PM><<<g, kNcoThreads, 0, st>>>(a, ntiles);
    }
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

__global__ void nco_put_state_kernel(bbb_nco_state s, bbb_nco_state *dst) { *dst = s; }

}  // namespace

int nco_put_state(const bbb_nco_state &s, bbb_nco_state *dst, hipStream_t st) {
    nco_put_state_kernel<<<1, 1, 0, st>>>(s, dst);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

uint64_t nco_tiles(uint64_t n) { return (n + kScanTile - 1) / kScanTile; }

int nco_launch(const NcoLaunch &a, int grid, hipStream_t st) {
    if (a.am) return a.pm ? launch_form<true, true>(a, grid, st) : launch_form<true, false>(a, grid, st);
    return a.pm ? launch_form<false, true>(a, grid, st) : launch_form<false, false>(a, grid, st);
}

}  // namespace bbb
