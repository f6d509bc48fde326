// acf_kernels.hip -- exact autocorrelation counters of int16 samples (include/bbb.h, "autocorrelation").
//
//   acf[l] += sum_{n < nfirst} x[n] x[n + l]   (l < nlags; x[j] = 0 for j >= navail),   acf[nlags] += sum_{n < nfirst} x[n]
//
// A Toeplitz product on the i8 matrix cores (v_mfma_i32_16x16x64_i8).  A tile is 1024 first elements from sample t, seen as
// 16 rows of stride 16: A[i][k] = x[t + 16k + i] (i < 16, k < 64), and block a of the lags takes B_a[k][j] = x[t + 16(k + a) + j].
// Entry (i, j) of A.B_a sums the pairs (n, n + l) with l = 16a + j - i; every pair of the tile with 0 <= l < nlags falls in
// exactly one entry (a = (i + l) / 16, j = (i + l) mod 16), so blocks a = 0 .. (nlags + 14) / 16 cover every lag.
//
// The operands are int8 limbs of x = 256 p0 + 16 p1 + lo (p0 = x >> 8, p1 = (x >> 4) & 15, lo = x & 15):
//  - 12-bit data (|x| <= 2048): x = 16 hi + lo with hi = x >> 4 in [-128, 127], four MFMAs per block into the slots of
//    weight 256 (hi.hi'), 16 (hi.lo' + lo.hi') and 1 (lo.lo');
//  - any other int16: nine MFMAs per block into slots of weight 65536, 4096, 256, 16 and 1.
//  The form is chosen from the data for every stage of 4096 first elements and every range of blocks: the workgroup votes
//  over the samples it stages, look-ahead included.
//  Every slot gains at most 2^20 per tile in magnitude, so the int32 accumulators are folded into int64 every 1024 tiles.
//
// Layout (checked on the device against numpy by tests/test_gpu_spectrum.py): lane l holds A[l & 15][k] and B[k][l & 15]
// for 16 values of k (which 16 does not matter: the k order is the same in both operands, and the sum over k is taken in
// any order), and D[4 (l >> 4) + r][l & 15] in accumulator register r.
//
// A workgroup is 4 waves over one stage at a time: it stages the stage's samples (with the look-ahead its blocks need) in
// LDS as byte planes [16 rows][rs dwords] (lo, then hi, or p0 and p1; rs odd), row i holding x[t0 + 16m + i] at byte m.  Lane
// (i, g) of a wave reads A of tile tau at bytes 64 tau + 16 g .. + 15 of row i and B_a at 64 tau + 16 g + a ..: the wave's
// blocks are consecutive, so one 6-dword window per plane serves all of them, realigned with v_alignbyte.  Waves fold
// into an int64 lag array in LDS (ds_add_u64); the workgroup writes it to a scratch slab with plain stores, and a small
// reduce kernel adds the slab into the counters.  Workgroups beyond the first row of the grid take further ranges of blocks
// (4096 lags: 257 blocks, 20 per workgroup).
#include "bbb_common.hpp"

#include <algorithm>

namespace bbb {

namespace {

constexpr int kAcfThreads = 256;                 // 4 waves
constexpr int kAcfWaves = kAcfThreads / kWave;
constexpr uint64_t kAcfStage = 4096;             // first elements per stage: 4 tiles of 16 x 64
constexpr int kAcfMaxBpw = 5;                    // blocks per wave
constexpr unsigned kAcfFlushStages = 256;        // 1024 tiles: each slot stays below 2^30 in magnitude
constexpr int kAcfPlanes = 3;

typedef int acf_i32x4 __attribute__((ext_vector_type(4)));

struct AcfGeom {
    unsigned na, bpw, gy, lw;                    // blocks, blocks per wave (max), block ranges, lag array entries
};

AcfGeom acf_geom(uint32_t nlags) {
    AcfGeom g;
    g.na = (nlags + 14) / 16 + 1;
    g.bpw = std::min<unsigned>(kAcfMaxBpw, (g.na + kAcfWaves - 1) / kAcfWaves);
    const unsigned br = kAcfWaves * g.bpw;
    g.gy = (g.na + br - 1) / br;
    g.lw = 16 * br + 16;
    return g;
}

// the plane row stride (dwords, odd) of the workgroups with blocks up to a_end (exclusive)
__host__ __device__ inline unsigned acf_rs(unsigned a_end) {
    const unsigned rs = 66 + ((a_end - 1) >> 2);
    return rs | 1u;
}

__device__ __forceinline__ uint32_t acf_align(uint32_t hi, uint32_t lo, unsigned sh) {
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

__device__ __forceinline__ acf_i32x4 acf_mfma(const acf_i32x4 &a, const acf_i32x4 &b, const acf_i32x4 &c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
}

// B fragment of block b (0 .. kAcfMaxBpw - 1) from a window W realigned to the wave's first block
template <int B>
__device__ __forceinline__ acf_i32x4 acf_bfrag(const uint32_t (&W)[5]) {
    constexpr int d = B >> 2, s = B & 3;
    acf_i32x4 r;
#pragma unroll
    for (int e = 0; e < 4; e++) r[e] = s ? (int)acf_align(W[d + e + 1], W[d + e], s) : (int)W[d + e];
    return r;
}

// the wave's window of one plane row: bytes [o, o + 20) of `row` with o = 4 q0 + sh
__device__ __forceinline__ void acf_window(const uint32_t *row, unsigned q0, unsigned sh, uint32_t (&W)[5]) {
    uint32_t R[6];
#pragma unroll
    for (int e = 0; e < 6; e++) R[e] = row[q0 + e];
#pragma unroll
    for (int e = 0; e < 5; e++) W[e] = acf_align(R[e + 1], R[e], sh);
}

__device__ __forceinline__ void acf_afrag(const uint32_t *row, unsigned q, acf_i32x4 &a) {
#pragma unroll
    for (int e = 0; e < 4; e++) a[e] = (int)row[q + e];
}

__device__ __forceinline__ void acf_mask(acf_i32x4 &a, unsigned cnt) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const unsigned lo = 4 * e;
        const uint32_t m = cnt >= lo + 4 ? 0xffffffffu : (cnt <= lo ? 0u : ((1u << (8 * (cnt - lo))) - 1u));
        a[e] = (int)((uint32_t)a[e] & m);
    }
}

// FULL = false: the 12-bit form over every stage whose staged samples all fit 12 bits.  Each row y of the grid (a range of
// blocks) stages its own look-ahead and decides for itself: a stage it finds wider is appended to ITS list,
// wide_list[y * nstages ..], wide_count[y] of them, and skipped.  FULL = true: row y takes the full-range form over the
// stages of its list.  So every (stage, row) is counted exactly once, by one of the two kernels.  Planes: 12-bit hi = x >> 4
// and lo; full range p0, p1 and lo.
template <bool FULL>
__global__ void __launch_bounds__(kAcfThreads)
acf_kernel(const int16_t *__restrict x, unsigned long long nfirst, unsigned long long navail, unsigned nlags, unsigned na,
           unsigned bpw, unsigned lw, unsigned long long nstages, unsigned long long *__restrict partials,
           unsigned long long *__restrict wide_list, unsigned long long *__restrict wide_count) {
    extern __shared__ uint32_t acf_smem[];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned a_base = blockIdx.y * kAcfWaves * bpw;
    const unsigned a_end = min(na, a_base + kAcfWaves * bpw);
    const unsigned rs = acf_rs(a_end);                    // this workgroup's planes (the launch sized LDS for the largest)
    const unsigned plane = 16 * rs;
    uint32_t *P = acf_smem;
    unsigned long long *Lg = reinterpret_cast<unsigned long long *>(acf_smem + kAcfPlanes * 16 * acf_rs(na));

    // this wave's blocks: the range [a_base, a_end) cut as evenly as possible
    const unsigned span = a_end - a_base, base = span / kAcfWaves, extra = span % kAcfWaves;
    const unsigned nb = base + (wave < extra);
    const unsigned a0 = a_base + wave * base + min(wave, extra);

    for (unsigned i = tid; i <= lw; i += kAcfThreads) Lg[i] = 0;

    // slots of weight 65536, 4096, 256, 16, 1 (the 12-bit form uses the last three)
    acf_i32x4 acc[kAcfMaxBpw][5];
#pragma unroll
    for (int b = 0; b < kAcfMaxBpw; b++)
#pragma unroll
        for (int s = 0; s < 5; s++) acc[b][s] = acf_i32x4{0, 0, 0, 0};

    const unsigned r = lane & 15, g = lane >> 4;
    const bool want_sum = blockIdx.y == 0;
    long long xsum = 0;
    unsigned since_flush = 0;

    auto flush = [&]() {
#pragma unroll
        for (int b = 0; b < kAcfMaxBpw; b++) {
            if ((unsigned)b < nb) {
                const int a = (int)(a0 + b);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int lag = 16 * a + (int)r - (int)(4 * g + e);
                    const unsigned long long v = ((unsigned long long)(long long)acc[b][0][e] << 16) +
                                                 ((unsigned long long)(long long)acc[b][1][e] << 12) +
                                                 ((unsigned long long)(long long)acc[b][2][e] << 8) +
                                                 ((unsigned long long)(long long)acc[b][3][e] << 4) +
                                                 (unsigned long long)(long long)acc[b][4][e];
                    if (lag >= 0 && lag < (int)nlags && v) atomicAdd(&Lg[lag - 16 * (int)a_base + 15], v);
                }
            }
#pragma unroll
            for (int s = 0; s < 5; s++) acc[b][s] = acf_i32x4{0, 0, 0, 0};
        }
    };

    unsigned long long *const list = wide_list + (unsigned long long)blockIdx.y * nstages;    // this row's
    const unsigned long long nwork = FULL ? wide_count[blockIdx.y] : nstages;
    if (FULL && nwork == 0) return;                       // the row took the 12-bit form everywhere (the reduce skips it)
    for (unsigned long long w = blockIdx.x; w < nwork; w += gridDim.x) {
        const unsigned long long st = FULL ? list[w] : w;
        const unsigned long long t0 = st * kAcfStage;
        __syncthreads();                                   // the previous stage's planes are read
        // stage: item (row, dword column q) = samples t0 + 16 (4q + u) + row, u = 0..3, zero at and beyond navail
        int wide = 0;
        long long ssum = 0;
        for (unsigned item = tid; item < plane; item += kAcfThreads) {
            const unsigned row = item & 15, q = item >> 4;
            uint32_t w0 = 0, w1 = 0, w2 = 0;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const unsigned m = 4 * q + u;
                const unsigned long long n = t0 + 16ull * m + row;
                const int v = n < navail ? (int)x[n] : 0;
                if (want_sum && m < 256 && n < nfirst) ssum += v;
                w0 |= (uint32_t)(v & 15) << (8 * u);
                if (FULL) {
                    w1 |= (uint32_t)((v >> 8) & 255) << (8 * u);
                    w2 |= (uint32_t)((v >> 4) & 15) << (8 * u);
                } else {
                    wide |= (v < -2048) | (v > 2047);
                    w1 |= (uint32_t)((v >> 4) & 255) << (8 * u);
                }
            }
            const unsigned o = row * rs + q;
            P[o] = w0;
            P[plane + o] = w1;
            if (FULL) P[2 * plane + o] = w2;
        }
        if (FULL) {
            __syncthreads();
        } else if (__syncthreads_or(wide)) {
            if (tid == 0) list[atomicAdd(&wide_count[blockIdx.y], 1ull)] = st;
            continue;
        }
        xsum += ssum;

        if (nb) {
            const uint32_t *rowL = P + r * rs;             // lane (r, g): A rows and B columns are both its r
            const uint32_t *row1 = rowL + plane;           // 12-bit: hi; full range: p0
            const uint32_t *row2 = rowL + 2 * plane;       // full range: p1
            const unsigned qa = (a0 >> 2), sh = a0 & 3;
#pragma unroll 1
            for (int tau = 0; tau < 4; tau++) {
                const unsigned long long t = t0 + 1024ull * tau;
                if (t >= nfirst) break;
                const unsigned qt = 16 * tau + 4 * g;      // dword of byte 64 tau + 16 g
                const long long rem = (long long)(nfirst - t) - (long long)(256 * g + r);
                const bool edge = t + 1024 > nfirst;
                const unsigned cnt = rem <= 0 ? 0u : (unsigned)min(16ll, (rem + 15) / 16);
                if constexpr (!FULL) {
                    acf_i32x4 Ah, Al;
                    acf_afrag(row1, qt, Ah);
                    acf_afrag(rowL, qt, Al);
                    if (edge) {
                        acf_mask(Ah, cnt);
                        acf_mask(Al, cnt);
                    }
                    uint32_t Wh[5], Wl[5];
                    acf_window(row1, qt + qa, sh, Wh);
                    acf_window(rowL, qt + qa, sh, Wl);
#define ACF_BLOCK12(B)                                                                           \
    if (B < kAcfMaxBpw && (unsigned)B < nb) {                                                    \
        const acf_i32x4 Bh = acf_bfrag<B>(Wh), Bl = acf_bfrag<B>(Wl);                            \
        acc[B][2] = acf_mfma(Ah, Bh, acc[B][2]);                                                 \
        acc[B][3] = acf_mfma(Ah, Bl, acc[B][3]);                                                 \
        acc[B][3] = acf_mfma(Al, Bh, acc[B][3]);                                                 \
        acc[B][4] = acf_mfma(Al, Bl, acc[B][4]);                                                 \
    }
                    ACF_BLOCK12(0) ACF_BLOCK12(1) ACF_BLOCK12(2) ACF_BLOCK12(3) ACF_BLOCK12(4)
#undef ACF_BLOCK12
                } else {
                    acf_i32x4 A0, A1, Al;
                    acf_afrag(row1, qt, A0);
                    acf_afrag(row2, qt, A1);
                    acf_afrag(rowL, qt, Al);
                    if (edge) {
                        acf_mask(A0, cnt);
                        acf_mask(A1, cnt);
                        acf_mask(Al, cnt);
                    }
                    uint32_t W0[5], W1[5], Wl[5];
                    acf_window(row1, qt + qa, sh, W0);
                    acf_window(row2, qt + qa, sh, W1);
                    acf_window(rowL, qt + qa, sh, Wl);
#define ACF_BLOCK16(B)                                                                           \
    if (B < kAcfMaxBpw && (unsigned)B < nb) {                                                    \
        const acf_i32x4 B0 = acf_bfrag<B>(W0), B1 = acf_bfrag<B>(W1), Bl = acf_bfrag<B>(Wl);     \
        acc[B][0] = acf_mfma(A0, B0, acc[B][0]);                                                 \
        acc[B][1] = acf_mfma(A0, B1, acc[B][1]);                                                 \
        acc[B][1] = acf_mfma(A1, B0, acc[B][1]);                                                 \
        acc[B][2] = acf_mfma(A0, Bl, acc[B][2]);                                                 \
        acc[B][2] = acf_mfma(A1, B1, acc[B][2]);                                                 \
        acc[B][2] = acf_mfma(Al, B0, acc[B][2]);                                                 \
        acc[B][3] = acf_mfma(A1, Bl, acc[B][3]);                                                 \
        acc[B][3] = acf_mfma(Al, B1, acc[B][3]);                                                 \
        acc[B][4] = acf_mfma(Al, Bl, acc[B][4]);                                                 \
    }
                    ACF_BLOCK16(0) ACF_BLOCK16(1) ACF_BLOCK16(2) ACF_BLOCK16(3) ACF_BLOCK16(4)
#undef ACF_BLOCK16
                }
            }
        }
        if (++since_flush == kAcfFlushStages) {
            flush();
            since_flush = 0;
        }
    }
    flush();
    if (want_sum && xsum) atomicAdd(&Lg[lw], (unsigned long long)xsum);
    __syncthreads();
    unsigned long long *out = partials + ((unsigned long long)blockIdx.y * gridDim.x + blockIdx.x) * (lw + 1);
    for (unsigned i = tid; i <= lw; i += kAcfThreads) out[i] = Lg[i];
}

// acf[o] += the slab: o < nlags sums lag o over every workgroup whose blocks reach it, o = nlags the first elements' sum.
// A block takes 8 consecutive outputs, 32 threads per output each summing every 32nd workgroup.  `counts` (the full-range
// pass): row y wrote its partials only if counts[y] > 0; its slab rows are skipped otherwise.
constexpr int kAcfReduceOut = 8;
__global__ void __launch_bounds__(256)
acf_reduce_kernel(const unsigned long long *__restrict partials, unsigned gx, unsigned gy, unsigned lw, unsigned br,
                  unsigned nlags, unsigned long long *__restrict acf, const unsigned long long *__restrict counts) {
    __shared__ unsigned long long S[256];
    const unsigned ol = threadIdx.x % kAcfReduceOut, sl = threadIdx.x / kAcfReduceOut;
    const unsigned o = blockIdx.x * kAcfReduceOut + ol;
    unsigned long long sum = 0;
    if (o == nlags) {
        if (!counts || counts[0])
            for (unsigned xb = sl; xb < gx; xb += 256 / kAcfReduceOut) sum += partials[(unsigned long long)xb * (lw + 1) + lw];
    } else if (o < nlags) {
        for (unsigned y = 0; y < gy; y++) {
            const int idx = (int)o - 16 * (int)(y * br) + 15;
            if (idx < 0 || idx >= (int)lw || (counts && counts[y] == 0)) continue;
            const unsigned long long *p = partials + (unsigned long long)y * gx * (lw + 1) + idx;
            for (unsigned xb = sl; xb < gx; xb += 256 / kAcfReduceOut) sum += p[(unsigned long long)xb * (lw + 1)];
        }
    }
    S[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x < kAcfReduceOut && o <= nlags) {
        unsigned long long t = 0;
        for (unsigned k = 0; k < 256 / kAcfReduceOut; k++) t += S[k * kAcfReduceOut + threadIdx.x];
        acf[o] += t;
    }
}

}  // namespace

AcfPlan acf_plan(uint32_t nlags, uint64_t max_nfirst) {
    AcfPlan p{};
    const AcfGeom g = acf_geom(nlags);
    int dev = 0, cus = 0, per_cu = 0;
    p.smem = (size_t)kAcfPlanes * 16 * acf_rs(g.na) * 4 + (size_t)(g.lw + 1) * 8;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, acf_kernel<false>, kAcfThreads, p.smem) != hipSuccess) {
        p.gx = -1;
        return p;
    }
    const uint64_t nstages = std::max<uint64_t>(1, (max_nfirst + kAcfStage - 1) / kAcfStage);
    const uint64_t want = std::max<uint64_t>(1, (uint64_t)std::max(cus, 1) * std::max(per_cu, 1) / g.gy);
    p.gx = (int)std::min<uint64_t>(nstages, want);
    p.gy = (int)g.gy;
    p.partial_words = (uint64_t)p.gx * g.gy * (g.lw + 1);
    p.scratch_words = p.partial_words + g.gy * (1 + nstages);     // + per row: the count and the list of full-range stages
    return p;
}

int acf_launch(const AcfPlan &p, const int16_t *samples, uint64_t nfirst, uint64_t navail, uint32_t nlags, uint64_t *scratch,
               uint64_t *acf, hipStream_t st) {
    if (nfirst == 0) return BBB_OK;
    const AcfGeom g = acf_geom(nlags);
    const uint64_t nstages = (nfirst + kAcfStage - 1) / kAcfStage;
    const unsigned gx = (unsigned)std::min<uint64_t>((uint64_t)p.gx, nstages);
    unsigned long long *part = reinterpret_cast<unsigned long long *>(scratch);
    unsigned long long *count = part + p.partial_words, *list = count + g.gy;     // [gy] counts, [gy][nstages] lists
    BBB_HIP(hipMemsetAsync(count, 0, g.gy * sizeof(*count), st));
    for (int full = 0; full < 2; full++) {
        if (full)
            acf_kernel<true><<<dim3(gx, g.gy), kAcfThreads, p.smem, st>>>(samples, nfirst, navail, nlags, g.na, g.bpw, g.lw,
                                                                           nstages, part, list, count);
        else
            acf_kernel<false><<<dim3(gx, g.gy), kAcfThreads, p.smem, st>>>(samples, nfirst, navail, nlags, g.na, g.bpw, g.lw,
                                                                            nstages, part, list, count);
        BBB_HIP(hipGetLastError());
        acf_reduce_kernel<<<(nlags + kAcfReduceOut) / kAcfReduceOut, 256, 0, st>>>(
            part, gx, g.gy, g.lw, kAcfWaves * g.bpw, nlags, reinterpret_cast<unsigned long long *>(acf), full ? count : nullptr);
        BBB_HIP(hipGetLastError());
    }
    return BBB_OK;
}

}  // namespace bbb
