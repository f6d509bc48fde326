// rs_kernels.hip -- the Reed-Solomon codec on the device (include/bbb.h, bbb_rs_decode and bbb_rs_encode).
//
// The decoder.  Frames are independent, so there is no state and no window.  A workgroup of four waves takes
// kRsFramesPerGroup coded frames at a time (4 I codewords: a multiple of its waves for every depth):
//   * it stages their bytes, which are contiguous in memory, into LDS from their unaligned start: the bytes up to the first
//     16-byte boundary and behind the last one by one, everything between as 16-byte loads that land 16-byte aligned in LDS
//     too (the stage starts at the same offset into 16 bytes as the memory does).  The de-interleave is then LDS byte reads;
//   * a wave owns one codeword at a time, lane l symbols 4l .. 4l+3 (rs_common.hpp has the per-lane core).  Syndromes in log
//     form, packed four to a word and XOR-reduced over the wave; all zero is the wave-uniform fast path.  Otherwise
//     Berlekamp-Massey with coefficient l in lane l, the discrepancy a cross-lane XOR made of eight ballots (no LDS pipe, and
//     a scalar result), the auxiliary polynomial moved up a lane per step; Lambda and Omega go to a few bytes of LDS of the
//     wave's own; every lane evaluates Lambda at its four positions, the roots are counted by ballot, the lanes that found one
//     work out the value and correct the byte in LDS;
//   * the frames' data bytes, contiguous again, are stored as whole aligned words.
// The field's exp / log tables come with the kernel's arguments and are copied to LDS once per workgroup.
// The encoder is the division by g(x), one codeword per lane with the register in 32 VGPRs; it is not the hot path.
#include "rs_launch.hpp"

#include <algorithm>

namespace bbb {
namespace {

constexpr int kRsThreads = 256, kRsWaves = kRsThreads / kWave;
constexpr uint32_t kRsStageBytes = (16 + kRsFramesPerGroup * kRsMaxDepth * kRsMaxN + 15) & ~15u;
constexpr uint32_t kRsWaveBytes = 128;             // S at 0, Lambda at 32 (33 of 48), Omega at 80 (32)
constexpr uint32_t kRsTableWords = sizeof(RsField) / 4;
static_assert(sizeof(RsField) == 768 && offsetof(RsLaunch, field) == 0, "the tables are the first 192 words of the launch");

// what one lane of a wave wrote to LDS, every lane of it reads behind this
__device__ __forceinline__ void rs_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t rs_wave_xor(uint32_t v) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d);
    return v;
}

// The XOR of a byte over the wave without the LDS pipe: bit b of the result is the parity of the lanes whose bit b is set, one
// ballot and one scalar bit count each.  The result is wave-uniform, which keeps Berlekamp-Massey's b and L in scalar registers.
__device__ __forceinline__ uint32_t rs_wave_xor_byte(uint32_t v) {
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) r |= ((uint32_t)__popcll(__ballot((v >> b) & 1u)) & 1u) << b;
    return r;
}

__device__ __forceinline__ uint32_t rs_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

__device__ __forceinline__ const uint8_t *rs_tables_to_lds(const RsLaunch &a, uint32_t *tab) {
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&a.field);
    for (uint32_t i = threadIdx.x; i < kRsTableWords; i += blockDim.x) tab[i] = src[i];
    __syncthreads();
    return reinterpret_cast<const uint8_t *>(tab);
}

__global__ __launch_bounds__(kRsThreads) void rs_decode_kernel(RsLaunch a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[kRsTableWords];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kRsStageBytes];
    __shared__ __attribute__((aligned(16))) uint8_t wave_mem[kRsWaves * kRsWaveBytes];
    const uint8_t *ex = rs_tables_to_lds(a, tab), *lg = ex + 512;
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
    const RsCode &c = a.code;
    const uint32_t I = c.depth, n = c.n, k = c.k, nroots = c.nroots, fbytes = I * n, dbytes = I * k;
    uint8_t *S = wave_mem + w * kRsWaveBytes, *lamv = S + 32, *omv = S + 80;
    uint32_t n_clean = 0, n_failed = 0, n_sym = 0, n_words = 0, my_bits = 0;      // the first four are the same in every lane
    const uint64_t ngrp = (a.nframes + kRsFramesPerGroup - 1) / kRsFramesPerGroup;
    for (uint64_t grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
        const uint64_t f0 = grp * kRsFramesPerGroup;
        const uint32_t nfr = (uint32_t)min((uint64_t)kRsFramesPerGroup, a.nframes - f0), bytes = nfr * fbytes;
        // ---- stage: byte j of the group at stage[sh + j]
        const uint8_t *src = a.in + f0 * fbytes;
        const uint32_t sh = (uint32_t)((uintptr_t)src & 15u), head = min(bytes, (16u - sh) & 15u), nvec = (bytes - head) / 16u;
        const uint32_t tail0 = head + nvec * 16u;
        if (t < head) stage[sh + t] = src[t];
        for (uint32_t i = t; i < nvec; i += kRsThreads)
            *reinterpret_cast<uint4 *>(stage + sh + head + 16u * i) = *reinterpret_cast<const uint4 *>(src + head + 16u * i);
        if (t < bytes - tail0) stage[sh + tail0 + t] = src[tail0 + t];
        __syncthreads();
        // ---- the codewords: number cw of the group is codeword cw % I of its frame cw / I
        for (uint32_t cw = w; cw < nfr * I; cw += kRsWaves) {
            const uint32_t fr = cw / I, ci = cw - fr * I;
            uint8_t *word = stage + sh + fr * fbytes;
            uint32_t sym = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t s = 4 * lane + q;
                if (s < n) sym |= (uint32_t)word[rs_byte_of(c, ci, s)] << (8 * q);
            }
            uint32_t syn[kRsMaxRoots / 4];
            rs_lane_syndromes(ex, lg, c, sym, lane, syn);
            uint32_t any = 0;
#pragma unroll
            for (uint32_t d = 0; d < kRsMaxRoots / 4; ++d)
                if (4 * d < nroots) {
                    syn[d] = rs_wave_xor(syn[d]);
                    any |= syn[d];
                }
            ++n_words;
            uint32_t nerr = 0;
            if (!any) {
                ++n_clean;
            } else {
                // the syndromes where every lane reads them: lane d holds word d after the select below
                uint32_t mine = 0;
#pragma unroll
                for (uint32_t d = 0; d < kRsMaxRoots / 4; ++d)
                    if (lane == d) mine = syn[d];
                if (lane < kRsMaxRoots / 4) reinterpret_cast<uint32_t *>(S)[lane] = mine;
                rs_wave_sync();
                uint32_t lam = lane == 0, bs = lane == 0, b = 1, L = 0;
                for (uint32_t r = 0; r < nroots; ++r) {
                    const uint32_t up = (uint32_t)__shfl_up((int)bs, 1);
                    bs = lane ? up : 0u;
                    const uint32_t d = rs_wave_xor_byte(rs_bm_term(ex, lg, lam, S, r, lane));
                    rs_bm_update(ex, lg, d, r, b, L, lam, bs);
                }
                nerr = BBB_RS_FAILED;
                if (2 * L <= nroots) {
                    if (lane <= kRsMaxRoots) lamv[lane] = (uint8_t)lam;
                    rs_wave_sync();
                    if (lane < kRsMaxRoots) omv[lane] = lane < L ? (uint8_t)rs_omega(ex, lg, lamv, L, S, lane) : (uint8_t)0;
                    rs_wave_sync();
                    uint32_t roots = 0, found = 0, zl[4], val[4];
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) zl[q] = 4 * lane + q < n ? rs_zlog(c, 4 * lane + q) : 0u;
                    rs_eval4(ex, lg, lamv, L + 1, zl, 0, 1, val);
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) {
                        const bool root = 4 * lane + q < n && val[q] == 0;
                        found |= (uint32_t)root << q;
                        roots += (uint32_t)__popcll(__ballot(root));
                    }
                    if (roots == L) {
                        nerr = L;
                        if (found) {
                            uint32_t num[4], den[4];
                            rs_eval4(ex, lg, omv, L, zl, 0, 1, num);
                            rs_eval4(ex, lg, lamv, L + 1, zl, 1, 2, den);
#pragma unroll
                            for (uint32_t q = 0; q < 4; ++q)
                                if (found >> q & 1) {
                                    const uint32_t mag = rs_value(ex, lg, c, num[q], den[q], zl[q]);
                                    word[rs_byte_of(c, ci, 4 * lane + q)] ^= (uint8_t)mag;
                                    my_bits += (uint32_t)__popc(mag);
                                }
                        }
                        n_sym += L;
                    }
                }
                if (nerr == BBB_RS_FAILED) ++n_failed;
                rs_wave_sync();                    // the wave's bytes are read before its next codeword writes them
            }
            if (a.nerr && lane == 0) a.nerr[(f0 + fr) * I + ci] = (uint8_t)nerr;
        }
        __syncthreads();
        // ---- the data: byte q of the group's output is byte q % dbytes of frame q / dbytes
        uint8_t *dst = a.out + f0 * dbytes;
        const uint32_t obytes = nfr * dbytes, ohead = min(obytes, (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u), nw = (obytes - ohead) / 4u;
        const uint32_t otail0 = ohead + nw * 4u;
        auto data_byte = [&](uint32_t q) -> uint32_t {
            const uint32_t fr = (uint32_t)(q >= dbytes) + (uint32_t)(q >= 2 * dbytes) + (uint32_t)(q >= 3 * dbytes);
            return stage[sh + fr * fbytes + (q - fr * dbytes)];
        };
        if (t < ohead) dst[t] = (uint8_t)data_byte(t);
        for (uint32_t i = t; i < nw; i += kRsThreads) {
            const uint32_t q = ohead + 4u * i;
            *reinterpret_cast<uint32_t *>(dst + q) = data_byte(q) | data_byte(q + 1) << 8 | data_byte(q + 2) << 16 | data_byte(q + 3) << 24;
        }
        if (t < obytes - otail0) dst[otail0 + t] = (uint8_t)data_byte(otail0 + t);
        __syncthreads();                           // the stage is read before the next group's bytes land in it
    }
    if (a.stats) {
        const uint32_t bits = rs_wave_sum(my_bits);
        if (lane == 0 && n_words) {
            unsigned long long *st = reinterpret_cast<unsigned long long *>(a.stats);
            atomicAdd(st + 0, (unsigned long long)n_words);
            if (n_clean) atomicAdd(st + 1, (unsigned long long)n_clean);
            if (n_failed) atomicAdd(st + 2, (unsigned long long)n_failed);
            if (n_sym) atomicAdd(st + 3, (unsigned long long)n_sym);
            if (bits) atomicAdd(st + 4, (unsigned long long)bits);
        }
    }
}

// ---- the encoder ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRsThreads) void rs_encode_kernel(RsLaunch a) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[kRsTableWords];
    __shared__ uint8_t gq[kRsMaxRoots];
    if (threadIdx.x < kRsMaxRoots) gq[threadIdx.x] = a.code.gq[threadIdx.x];
    const uint8_t *ex = rs_tables_to_lds(a, tab), *lg = ex + 512;
    const uint32_t I = a.code.depth, n = a.code.n, k = a.code.k, nroots = a.code.nroots;
    const uint64_t nwords = a.nframes * I;
    for (uint64_t cw = (uint64_t)blockIdx.x * kRsThreads + threadIdx.x; cw < nwords; cw += (uint64_t)gridDim.x * kRsThreads) {
        const uint64_t f = cw / I;
        const uint32_t ci = (uint32_t)(cw - f * I);
        const uint8_t *src = a.in + f * I * k;
        uint8_t *dst = a.out + f * I * n;
        uint8_t par[kRsMaxRoots];
#pragma unroll
        for (uint32_t j = 0; j < kRsMaxRoots; ++j) par[j] = 0;
        for (uint32_t s = 0; s < k; ++s) {
            const uint32_t d = src[rs_byte_of(a.code, ci, s)];
            dst[rs_byte_of(a.code, ci, s)] = (uint8_t)d;
            rs_lfsr_step(ex, lg, gq, par, d);
        }
#pragma unroll
        for (uint32_t j = 0; j < kRsMaxRoots; ++j)
            if (j < nroots) dst[rs_byte_of(a.code, ci, k + j)] = par[j];
    }
}

}  // namespace

int rs_decode_launch(const RsLaunch &a, int cus, hipStream_t st) {
    const uint64_t ngrp = (a.nframes + kRsFramesPerGroup - 1) / kRsFramesPerGroup;
    const unsigned grid = (unsigned)std::min<uint64_t>(ngrp, (uint64_t)std::max(1, cus) * 16);
    rs_decode_kernel<<<grid, kRsThreads, 0, st>>>(a);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

int rs_encode_launch(const RsLaunch &a, hipStream_t st) {
    const uint64_t nwords = a.nframes * a.code.depth;
    const unsigned grid = (unsigned)std::min<uint64_t>((nwords + kRsThreads - 1) / kRsThreads, 1u << 16);
    rs_encode_kernel<<<grid, kRsThreads, 0, st>>>(a);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
