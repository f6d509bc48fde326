// ldpc_kernels.hip -- the LDPC codec on the device (include/bbb.h, bbb_ldpc_decode and bbb_ldpc_encode).
//
// The decoder.  Codewords are independent, so there is no state and no window.  A workgroup of four waves takes a GROUP of
// G = code.group codewords at a time (ldpc_common.hpp has the rule: G Z <= 256 where Z allows it):
//   * it stages their values, which are contiguous in memory, into LDS as the int16 posteriors P from their unaligned start:
//     the halfwords up to the first 16-byte boundary and behind the last one singly, everything between as 16-byte loads that
//     land 16-byte aligned in LDS too.  -32768 becomes -32767 on the way.  HARD bits become +-hard_mag;
//   * the first hard decisions are packed by ballot into a flat bit array (for "bits corrected"), and every lane works out the
//     parity of its checks: a codeword none of whose lanes raised its LDS flag is done with iters 0;
//   * an iteration is J layers with one workgroup barrier behind each.  The G Z checks of a layer are spread over the lanes;
//     the lane of row r reads P[(r + s) mod Z] of every block of its row, so consecutive lanes read consecutive halfwords.
//     ldpc_check keeps the Q_e in registers; the compressed record of the check (two words and a byte, LDS) is read and
//     written once.  Behind the last layer the parities again, the flags, and one barrier more for the iteration table.  A
//     codeword that has converged skips the work and waits at the barriers for its group;
//   * the last hard decisions are packed by ballot; every output word of the group's data is gathered from that array by one
//     lane.  Words that lie wholly inside the group's bits are stored; the (at most two) words shared with a neighbouring group
//     are OR-ed into memory that the launch zeroed.
// P, the records and the bit arrays live in LDS for the whole decode and never reach global memory; nothing is kept per lane
// but registers.  Registers and LDS decide the occupancy: 117 VGPRs allow four workgroups a compute unit; array(3, 1, 2) takes
// 0.8 KiB of LDS and array(127, 4, 16) 18.0 KiB (four workgroups either way), the largest code (n 16384, m 8192) 108.1 KiB (one).
// The encoder is one workgroup per codeword, a halfword per bit in LDS and J serial steps; it is not the hot path.
#include "ldpc_launch.hpp"

#include <algorithm>
#include <mutex>

namespace bbb {
namespace {

constexpr uint32_t kLdpcMaxLds = 112 * 1024;

__device__ __forceinline__ uint32_t ldpc_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d);
    return v;
}

// the hard decisions of P[0 .. vals) as a flat bit array: a ballot per 64 values, one store per word
__device__ __forceinline__ void ldpc_pack_hard(const int16_t *P, uint32_t vals, uint64_t *dst) {
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (uint32_t base = wave * kWave; base < vals; base += kLdpcThreads) {
        const uint32_t q = base + lane;
        const uint64_t mask = __ballot(q < vals && P[q < vals ? q : 0] > 0);
        if (lane == 0) dst[base >> 6] = mask;
    }
}

// the output words that hold bits of [b0, b1): one lane each
__device__ __forceinline__ void ldpc_store_words(const uint64_t *flat, uint64_t *out, uint64_t b0, uint64_t b1, uint64_t item0, uint32_t per,
                                                 uint32_t stride) {
    for (uint64_t W = (b0 >> 6) + threadIdx.x; 64 * W < b1; W += kLdpcThreads) {
        const uint64_t v = ldpc_out_word(flat, W, b0, b1, item0, per, stride);
        if (ldpc_word_inside(W, b0, b1)) out[W] = v;
        else if (v) atomicOr(reinterpret_cast<unsigned long long *>(out) + W, (unsigned long long)v);
    }
}

__device__ __forceinline__ uint32_t ldpc_clamp_pair(uint32_t w) {
    // two int16 in a word: -32768 becomes -32767
    if ((w & 0xFFFFu) == 0x8000u) w |= 1u;
    if ((w >> 16) == 0x8000u) w |= 0x10000u;
    return w;
}

__global__ __launch_bounds__(kLdpcThreads) void ldpc_decode_kernel(LdpcLaunch a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const LdpcCode &c = a.code;
    const LdpcLds L = ldpc_lds(c);
    int16_t *Pb = reinterpret_cast<int16_t *>(lds + L.P);
    uint2 *rec = reinterpret_cast<uint2 *>(lds + L.rec);
    uint8_t *i1v = lds + L.i1;
    uint64_t *orig = reinterpret_cast<uint64_t *>(lds + L.orig), *fin = reinterpret_cast<uint64_t *>(lds + L.fin);
    int32_t *iters = reinterpret_cast<int32_t *>(lds + L.tab), *bad = iters + kLdpcMaxGroup;
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1);
    const uint32_t Z = c.Z, J = c.J, n = c.n, m = c.m, k = c.k, G = c.group;
    uint32_t n_words = 0, n_clean = 0, n_failed = 0, n_iter = 0, my_bits = 0;    // the first four are the same in every lane
    const uint64_t ngrp = (a.ncodewords + G - 1) / G;
    for (uint64_t grp = blockIdx.x; grp < ngrp; grp += gridDim.x) {
        const uint64_t cw0 = grp * G;
        const uint32_t ng = (uint32_t)min((uint64_t)G, a.ncodewords - cw0), vals = ng * n, nchk = ng * Z;
        // ---- stage: value q of the group at P[q]
        uint32_t sh = 0;
        if (a.format == BBB_CONV_SOFT16) {
            const int16_t *src = reinterpret_cast<const int16_t *>(a.in) + a.in_first + cw0 * n;
            sh = (uint32_t)((uintptr_t)src & 15u) / 2u;
            const uint32_t head = min(vals, (8u - sh) & 7u), nvec = (vals - head) / 8u, tail0 = head + nvec * 8u;
            int16_t *P = Pb + sh;
            if (t < head) P[t] = (int16_t)ldpc_clamp(src[t]);
            for (uint32_t i = t; i < nvec; i += kLdpcThreads) {
                uint4 v = *reinterpret_cast<const uint4 *>(src + head + 8u * i);
                v.x = ldpc_clamp_pair(v.x);
                v.y = ldpc_clamp_pair(v.y);
                v.z = ldpc_clamp_pair(v.z);
                v.w = ldpc_clamp_pair(v.w);
                *reinterpret_cast<uint4 *>(P + head + 8u * i) = v;
            }
            if (t < vals - tail0) P[tail0 + t] = (int16_t)ldpc_clamp(src[tail0 + t]);
        } else {
            const uint64_t *src = reinterpret_cast<const uint64_t *>(a.in);
            const uint64_t bit0 = a.in_first + cw0 * n;
            const int16_t mag = (int16_t)c.hard_mag;
            for (uint32_t q = t; q < vals; q += kLdpcThreads) {
                const uint64_t b = bit0 + q;
                Pb[q] = (src[b >> 6] >> (b & 63u) & 1u) ? mag : (int16_t)-mag;
            }
        }
        int16_t *P = Pb + sh;
        if (t < ng) {
            iters[t] = kLdpcRunning;
            bad[t] = 0;
        }
        // ---- the lane's checks: row cr of codeword cg of the group, one per round
        uint32_t cg[kLdpcRounds], cr[kLdpcRounds];
        bool have[kLdpcRounds];
#pragma unroll
        for (uint32_t rd = 0; rd < kLdpcRounds; ++rd) {
            const uint32_t q = t + kLdpcThreads * rd;
            have[rd] = q < nchk;
            cg[rd] = have[rd] ? q / Z : 0u;
            cr[rd] = have[rd] ? q - cg[rd] * Z : 0u;
        }
        __syncthreads();
        // the flags of the codewords with a check that is not satisfied: by ballot where a wave holds one codeword
        auto syndrome = [&]() {
            uint32_t fail[kLdpcRounds];
#pragma unroll
            for (uint32_t rd = 0; rd < kLdpcRounds; ++rd) {
                fail[rd] = 0;
                if (have[rd] && iters[cg[rd]] == kLdpcRunning)
                    for (uint32_t j = 0; j < J; ++j) fail[rd] |= ldpc_parity(c, j, cr[rd], P + cg[rd] * n);
            }
#pragma unroll
            for (uint32_t rd = 0; rd < kLdpcRounds; ++rd) {
                if (G == 1) {
                    if (__ballot(fail[rd] != 0) && lane == 0) bad[0] = 1;
                } else if (fail[rd]) {
                    bad[cg[rd]] = 1;
                }
            }
        };
        ldpc_pack_hard(P, vals, orig);
        syndrome();
        __syncthreads();
        if (t < ng && !bad[t]) iters[t] = 0;
        __syncthreads();
        // ---- the iterations
        for (uint32_t it = 0; it < c.max_iter; ++it) {
            uint32_t any = 0;
            for (uint32_t g = 0; g < ng; ++g) any |= (uint32_t)(iters[g] == kLdpcRunning);
            if (!any) break;
            if (t < ng) bad[t] = 0;
            for (uint32_t j = 0; j < J; ++j) {
#pragma unroll
                for (uint32_t rd = 0; rd < kLdpcRounds; ++rd)
                    if (have[rd] && iters[cg[rd]] == kLdpcRunning) {
                        const uint32_t at = cg[rd] * m + j * Z + cr[rd];
                        uint32_t w0 = 0, mask = 0, i1 = 0;
                        if (it) {
                            const uint2 r = rec[at];
                            w0 = r.x;
                            mask = r.y;
                            i1 = i1v[at];
                        }
                        ldpc_check(c, j, cr[rd], it == 0, P + cg[rd] * n, w0, mask, i1);
                        rec[at] = make_uint2(w0, mask);
                        i1v[at] = (uint8_t)i1;
                    }
                __syncthreads();
            }
            syndrome();
            __syncthreads();
            if (t < ng && iters[t] == kLdpcRunning && !bad[t]) iters[t] = (int32_t)(it + 1);
            __syncthreads();
        }
        if (t < ng && iters[t] == kLdpcRunning) iters[t] = (int32_t)kLdpcFailed;
        ldpc_pack_hard(P, vals, fin);
        __syncthreads();
        // ---- the outputs
        for (uint32_t g = 0; g < ng; ++g) {
            const int32_t v = iters[g];
            ++n_words;
            if (v == 0) ++n_clean;
            else if (v == (int32_t)kLdpcFailed) ++n_failed;
            else n_iter += (uint32_t)v;
        }
        if (a.iters && t < ng) a.iters[cw0 + t] = (uint8_t)iters[t];
        for (uint32_t w = t; w < (vals + 63u) / 64u; w += kLdpcThreads) my_bits += ldpc_corrected(orig[w] ^ fin[w], w, n, vals, iters);
        ldpc_store_words(fin, a.out, cw0 * k, (cw0 + ng) * k, cw0, k, n);
        __syncthreads();                           // the LDS is read before the next group's values land in it
    }
    if (a.stats) {
        const uint32_t bits = ldpc_wave_sum(my_bits);
        unsigned long long *st = reinterpret_cast<unsigned long long *>(a.stats);
        if (t == 0 && n_words) {
            atomicAdd(st + 0, (unsigned long long)n_words);
            if (n_clean) atomicAdd(st + 1, (unsigned long long)n_clean);
            if (n_failed) atomicAdd(st + 2, (unsigned long long)n_failed);
            if (n_iter) atomicAdd(st + 3, (unsigned long long)n_iter);
        }
        if (lane == 0 && bits) atomicAdd(st + 4, (unsigned long long)bits);
    }
}

// ---- the encoder ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLdpcThreads) void ldpc_encode_kernel(LdpcLaunch a) {
    __shared__ int16_t x[kLdpcMaxN];               // a bit per entry, as the decoder's posteriors: 1 or 0
    __shared__ uint64_t flat[kLdpcMaxN / 64];
    const LdpcCode &c = a.code;
    const uint32_t t = threadIdx.x, Z = c.Z, n = c.n, k = c.k;
    const uint64_t *src = reinterpret_cast<const uint64_t *>(a.in);
    for (uint64_t w = blockIdx.x; w < a.ncodewords; w += gridDim.x) {
        for (uint32_t i = t; i < k; i += kLdpcThreads) {
            const uint64_t b = w * k + i;
            x[i] = (int16_t)(src[b >> 6] >> (b & 63u) & 1u);
        }
        __syncthreads();
        for (uint32_t j = c.J; j-- > 0;) {
            const uint32_t d = ldpc_diag(c, j);
            for (uint32_t r = t; r < Z; r += kLdpcThreads) {
                uint32_t v = 0;
                for (uint32_t e = 0; e < c.deg[j]; ++e)
                    if (e != d) v ^= (uint32_t)x[ldpc_var(c, j, e, r)];
                x[ldpc_var(c, j, d, r)] = (int16_t)v;
            }
            __syncthreads();
        }
        ldpc_pack_hard(x, n, flat);
        __syncthreads();
        ldpc_store_words(flat, a.out, w * n, (w + 1) * n, w, n, n);
        __syncthreads();
    }
}

// the decoder takes more dynamic LDS than a kernel may have unasked
int ldpc_lds_attribute() {
    static std::mutex mu;
    static bool attr_set[64] = {false};
    int dev = 0;
    BBB_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> g(mu);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        BBB_HIP(hipFuncSetAttribute((const void *)ldpc_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdpcMaxLds));
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    return BBB_OK;
}

}  // namespace

// The cap of the decoder's grid: eight workgroups a compute unit, two turns of the four that are resident at once
// (tests/test_gpu_ldpc.py names this factor).
int ldpc_decode_launch(const LdpcLaunch &a, int cus, hipStream_t st) {
    const LdpcLds L = ldpc_lds(a.code);
    if (L.bytes > kLdpcMaxLds) return fail(BBB_EINVAL, "the code does not fit the decoder's LDS");
    int rc = ldpc_lds_attribute();
    if (rc) return rc;
    const uint64_t ngrp = (a.ncodewords + a.code.group - 1) / a.code.group;
    const unsigned grid = (unsigned)std::min<uint64_t>(ngrp, (uint64_t)std::max(1, cus) * 8);
    BBB_HIP(hipMemsetAsync(a.out, 0, 8 * ((a.ncodewords * a.code.k + 63) / 64), st));
    ldpc_decode_kernel<<<grid, kLdpcThreads, L.bytes, st>>>(a);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

int ldpc_encode_launch(const LdpcLaunch &a, int cus, hipStream_t st) {
    const unsigned grid = (unsigned)std::min<uint64_t>(a.ncodewords, (uint64_t)std::max(1, cus) * 16);
    BBB_HIP(hipMemsetAsync(a.out, 0, 8 * ((a.ncodewords * a.code.n + 63) / 64), st));
    ldpc_encode_kernel<<<grid, kLdpcThreads, 0, st>>>(a);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
