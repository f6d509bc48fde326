// carrier_kernels.hip -- the exact carrier recovery over int16 (I, Q) pairs (include/bbb.h, bbb_carrier_run).
//
//   SR_j = sum(I I - Q Q)   SI_j = 2 sum(I Q)   h_j = (CORDIC phase of (SR_j, SI_j) >> s) / 2   est_j = h_j + 32768 b_j
// The unwrap is a serial loop over the blocks, but b_j = b_(j-1) XOR f_j with f_j a function of h_j and h_(j-1) alone
// (carrier_common.hpp): the state is one bit and the loop a prefix XOR.  Five kernels, queued back to back, none of which
// waits on another workgroup:
//   * carrier_sum_kernel: a workgroup takes a tile of floor(2048 / L) blocks, a thread squares its 8 pairs into an int64 pair,
//     the L / 8 threads of a block join by shuffles and then through LDS, one lane per block normalises, runs ddc_polar and
//     stores h_j.  Integer sums: the order does not matter.
//   * carrier_flag_kernel: a workgroup per chunk of blocks, a thread 8 consecutive blocks a turn: f_j, its prefix XOR inside
//     the thread, the threads' parities by ballot and popcount parity, e_j = h_j | 32768 * (the prefix XOR inside the chunk);
//     the chunk's parity; what the workgroup counted for stats_dev (f alone: none of the counters needs b).
//   * carrier_chain_kernel (one workgroup): threads XOR the parities of their share of the chunks, one thread chains the 256
//     shares from the state's bit, every thread replays its share: the start bit of every chunk.  It writes the state words and adds up the counters.
//   * carrier_est_kernel: est_j = e_j XOR 32768 * (the chunk's start bit), in place, and phase_dev.
//   * carrier_rotate_kernel: re-reads the tile, looks up (c, s) of its block's est_j in the ROM (in LDS, filled from the
//     kernel's arguments), turns its 8 pairs back, saturates and stores: pairs and soft values with 16-byte stores where
//     aligned, and the 8 decisions as ONE BYTE -- a tile starts at a multiple of 8 pairs, so no two threads share a byte.
// The result never depends on the data or on chunk_blocks.
#include "carrier_launch.hpp"

#include <algorithm>

namespace bbb {
namespace {

constexpr int kCarrierWaves = kCarrierThreads / kWave;

// a thread's 8 pairs, a word a pair: I in the low half
struct CarrierRegs {
    uint4 lo, hi;
};

// the pairs [p0, p0 + 8) with zeros from g.nin on; p0 is a multiple of 8
__device__ __forceinline__ CarrierRegs carrier_load(const CarrierLaunch &a, uint64_t p0, bool active) {
    CarrierRegs r;
    r.lo = r.hi = make_uint4(0, 0, 0, 0);
    if (!active || p0 >= a.g.nin) return r;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(a.in) + p0;
    if (a.in_vec && p0 + 8 <= a.g.nin) {
        r.lo = *reinterpret_cast<const uint4 *>(w);
        r.hi = *reinterpret_cast<const uint4 *>(w + 4);
        return r;
    }
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = p0 + k < a.g.nin ? w[k] : 0u;
    r.lo = make_uint4(v[0], v[1], v[2], v[3]);
    r.hi = make_uint4(v[4], v[5], v[6], v[7]);
    return r;
}
__device__ __forceinline__ void carrier_words(const CarrierRegs &r, uint32_t (&v)[8]) {
    v[0] = r.lo.x, v[1] = r.lo.y, v[2] = r.lo.z, v[3] = r.lo.w;
    v[4] = r.hi.x, v[5] = r.hi.y, v[6] = r.hi.z, v[7] = r.hi.w;
}
__device__ __forceinline__ int pair_i(uint32_t w) { return (int)(int16_t)(w & 0xFFFFu); }
__device__ __forceinline__ int pair_q(uint32_t w) { return (int)w >> 16; }

// the first block and the blocks of a tile
struct CarrierTile {
    uint64_t j0, base;
    uint32_t nblk;
};
__device__ __forceinline__ CarrierTile carrier_tile(const CarrierGeom &g, uint32_t G, uint64_t tile) {
    CarrierTile t;
    t.j0 = tile * G;
    t.base = t.j0 * g.L;
    const uint64_t left = g.nblocks - t.j0;
    t.nblk = left < G ? (uint32_t)left : G;
    return t;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int d = kWave / 2; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

__global__ __launch_bounds__(kCarrierThreads) void carrier_sum_kernel(CarrierLaunch a) {
    __shared__ long long part_r[kCarrierThreads], part_i[kCarrierThreads];
    const CarrierGeom &g = a.g;
    const uint32_t t = threadIdx.x, L8 = g.L / 8, G = carrier_blocks_per_tile(g.L), fold = carrier_fold(g.L), per = L8 / fold;
    const uint64_t ntiles = carrier_ntiles(g);
    if (blockIdx.x >= ntiles) return;
    const bool owner = t < G * L8;
    uint32_t nzero = 0;
    CarrierRegs regs = carrier_load(a, carrier_tile(g, G, blockIdx.x).base + 8 * t, owner);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const CarrierTile tl = carrier_tile(g, G, tile);
        uint32_t v[8];
        carrier_words(regs, v);
        if (tile + gridDim.x < ntiles) regs = carrier_load(a, carrier_tile(g, G, tile + gridDim.x).base + 8 * t, owner);
        int64_t sr = 0, siq = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) carrier_square(pair_i(v[k]), pair_q(v[k]), sr, siq);
        long long wr = sr, wi = siq;
        for (uint32_t d = fold >> 1; d; d >>= 1) {
            wr += __shfl_xor(wr, (int)d);
            wi += __shfl_xor(wi, (int)d);
        }
        if (t % fold == 0) {
            part_r[t / fold] = wr;
            part_i[t / fold] = wi;
        }
        __syncthreads();
        if (t < tl.nblk) {
            int64_t br = 0, bi = 0;
            for (uint32_t k = 0; k < per; ++k) {
                br += part_r[t * per + k];
                bi += part_i[t * per + k];
            }
            bool zero;
            a.h[tl.j0 + t] = (uint16_t)carrier_h(br, bi, &zero);
            nzero += zero;
        }
        __syncthreads();                           // the parts are written again in the next turn
    }
    if (a.stats) {
        const long long n = wave_sum((long long)nzero);
        if ((t & (kWave - 1)) == 0 && n) atomicAdd((unsigned long long *)a.stats + 2, (unsigned long long)n);
    }
}

__global__ __launch_bounds__(kCarrierThreads) void carrier_flag_kernel(CarrierLaunch a) {
    __shared__ uint32_t wpar[kCarrierWaves];
    const CarrierGeom &g = a.g;
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const uint32_t hfirst = carrier_state_est(a.state[0], a.init_phase) & 0x7FFFu;      // h_(-1) of the call's block 0
    uint32_t nflip = 0;
    long long steps = 0;
    for (uint64_t c = blockIdx.x; c < g.nchunks; c += gridDim.x) {
        const uint64_t j_lo = c * g.chunk, j_hi = min(g.nblocks, j_lo + g.chunk);
        uint32_t carry = 0;
        // a turn takes kCarrierFlagTurn blocks, a thread kCarrierFlagPer consecutive ones: one round of loads a turn
        for (uint64_t j0 = j_lo; j0 < j_hi; j0 += kCarrierFlagTurn) {
            const uint64_t jt = j0 + (uint64_t)kCarrierFlagPer * t;
            uint32_t hv[kCarrierFlagPer + 1], pre[kCarrierFlagPer], run = 0;
            hv[0] = jt < j_hi ? (jt ? a.h[jt - 1] : hfirst) : 0u;
#pragma unroll
            for (uint32_t k = 0; k < kCarrierFlagPer; ++k) hv[k + 1] = jt + k < j_hi ? a.h[jt + k] : 0u;
#pragma unroll
            for (uint32_t k = 0; k < kCarrierFlagPer; ++k) {
                if (jt + k < j_hi) {
                    const uint32_t f = carrier_flip(hv[k + 1], hv[k]);
                    steps += carrier_step(hv[k + 1], hv[k], f);
                    nflip += f;
                    run ^= f;
                }
                pre[k] = run;
            }
            const unsigned long long bal = __ballot(run != 0);
            const uint32_t excl = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)) & 1u;
            if (lane == 0) wpar[wv] = (uint32_t)__popcll(bal) & 1u;
            __syncthreads();
            uint32_t before = 0, total = 0;
#pragma unroll
            for (int k = 0; k < kCarrierWaves; ++k) {
                before ^= k < (int)wv ? wpar[k] : 0u;
                total ^= wpar[k];
            }
            const uint32_t base = excl ^ before ^ carry;
#pragma unroll
            for (uint32_t k = 0; k < kCarrierFlagPer; ++k)
                if (jt + k < j_hi) a.e[jt + k] = (uint16_t)(hv[k + 1] | (pre[k] ^ base) << 15);
            carry ^= total;
            __syncthreads();                       // wpar is written again in the next turn
        }
        if (t == 0) a.cpar[c] = (uint8_t)carry;
    }
    // what this workgroup counted goes to its own two words: the chain kernel adds them up (thousands of atomics on two
    // addresses would take longer than the pass)
    __shared__ long long wn[kCarrierWaves], ws[kCarrierWaves];
    const long long n = wave_sum((long long)nflip), s = wave_sum(steps);
    if (lane == 0) {
        wn[wv] = n;
        ws[wv] = s;
    }
    __syncthreads();
    if (t == 0) {
        long long tn = 0, ts = 0;
#pragma unroll
        for (int k = 0; k < kCarrierWaves; ++k) {
            tn += wn[k];
            ts += ws[k];
        }
        a.wsum[2 * blockIdx.x] = (uint64_t)tn;
        a.wsum[2 * blockIdx.x + 1] = (uint64_t)ts;
    }
}

__global__ __launch_bounds__(kCarrierThreads) void carrier_chain_kernel(CarrierLaunch a) {
    __shared__ uint8_t spar[kCarrierThreads], start[kCarrierThreads];
    __shared__ uint32_t endb;
    const CarrierGeom &g = a.g;
    const uint32_t t = threadIdx.x;
    const uint64_t share = carrier_chain_share(g.nchunks), lo = min(g.nchunks, t * share), hi = min(g.nchunks, lo + share);
    // the state words are read by every thread HERE, in front of the first barrier, and written by thread 0 behind the
    // second: no load of them can come after the store
    const uint64_t s0 = a.state[0], s1 = a.state[1];
    uint32_t p = 0;
    for (uint64_t c = lo; c < hi; ++c) p ^= a.cpar[c];
    spar[t] = (uint8_t)p;
    __syncthreads();
    if (t == 0) {
        uint32_t b = carrier_state_est(s0, a.init_phase) >> 15;
        for (int k = 0; k < kCarrierThreads; ++k) {
            start[k] = (uint8_t)b;
            b ^= spar[k];
        }
        endb = b;
    }
    __syncthreads();
    uint32_t b = start[t];
    for (uint64_t c = lo; c < hi; ++c) {
        a.cstart[c] = (uint8_t)b;
        b ^= a.cpar[c];
    }
    // the flag kernel's counts, a share of its workgroups a thread
    __shared__ long long wn[kCarrierWaves], ws[kCarrierWaves];
    long long cn = 0, cs = 0;
    for (uint32_t k = t; k < a.nflag; k += kCarrierThreads) {
        cn += (long long)a.wsum[2 * k];
        cs += (long long)a.wsum[2 * k + 1];
    }
    cn = wave_sum(cn);
    cs = wave_sum(cs);
    if ((t & (kWave - 1)) == 0) {
        wn[t / kWave] = cn;
        ws[t / kWave] = cs;
    }
    __syncthreads();
    if (t == 0) {
        if (g.nblocks) a.state[0] = kCarrierStarted | (a.e[g.nblocks - 1] & 0x7FFFu) | endb << 15;
        a.state[1] = s1 + g.nin;
        if (a.stats) {
            long long tn = 0, ts = 0;
#pragma unroll
            for (int k = 0; k < kCarrierWaves; ++k) {
                tn += wn[k];
                ts += ws[k];
            }
            a.stats[0] += g.nblocks;
            a.stats[1] += (uint64_t)tn;
            a.stats[3] += (uint64_t)ts;
        }
    }
}

__global__ __launch_bounds__(kCarrierThreads) void carrier_est_kernel(CarrierLaunch a) {
    const CarrierGeom &g = a.g;
    for (uint64_t c = blockIdx.x; c < g.nchunks; c += gridDim.x) {
        const uint64_t j_lo = c * g.chunk, j_hi = min(g.nblocks, j_lo + g.chunk);
        const uint32_t b = a.cstart[c];
        for (uint64_t j = j_lo + threadIdx.x; j < j_hi; j += kCarrierThreads) {
            const uint16_t est = (uint16_t)(a.e[j] ^ b << 15);
            a.e[j] = est;
            if (a.phase) a.phase[j] = est;
        }
    }
}

__global__ __launch_bounds__(kCarrierThreads) void carrier_rotate_kernel(CarrierLaunch a, CarrierRom rom) {
    __shared__ uint32_t rom_lds[512];
    const CarrierGeom &g = a.g;
    const uint32_t t = threadIdx.x, L8 = g.L / 8, G = carrier_blocks_per_tile(g.L), jb = t / L8;
    const uint64_t ntiles = carrier_ntiles(g);
    if (blockIdx.x >= ntiles) return;
    for (uint32_t i = t; i < 512; i += kCarrierThreads) rom_lds[i] = reinterpret_cast<const uint32_t *>(rom.v)[i];
    __syncthreads();
    const int16_t *rom_l = reinterpret_cast<const int16_t *>(rom_lds);
    const bool owner = t < G * L8;
    const uint64_t out_bytes = carrier_bit_words(g.nblocks, g.L) * 8;
    CarrierRegs regs = carrier_load(a, carrier_tile(g, G, blockIdx.x).base + 8 * t, owner);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const CarrierTile tl = carrier_tile(g, G, tile);
        const bool active = jb < tl.nblk;
        const uint32_t est = active ? a.e[tl.j0 + jb] : 0u;
        uint32_t v[8];
        carrier_words(regs, v);
        if (tile + gridDim.x < ntiles) regs = carrier_load(a, carrier_tile(g, G, tile + gridDim.x).base + 8 * t, owner);
        if (active) {
            const int c = rom_l[carrier_adr_cos(est)], s = rom_l[carrier_adr_sin(est)];
            const uint64_t p0 = tl.base + 8 * t;
            const uint32_t nvalid = p0 >= g.nin ? 0u : (uint32_t)min((uint64_t)8, g.nin - p0);
            uint32_t w[8], sv[4], byte = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int io, qo;
                carrier_rotate(pair_i(v[k]), pair_q(v[k]), c, s, io, qo);
                w[k] = ((uint32_t)io & 0xFFFFu) | (uint32_t)qo << 16;
                if (k & 1) sv[k / 2] |= (uint32_t)io << 16;
                else sv[k / 2] = (uint32_t)io & 0xFFFFu;
                byte |= (uint32_t)carrier_decide(io, a.threshold, a.strict != 0) << k;
            }
            if (a.iq) {
                uint32_t *o = reinterpret_cast<uint32_t *>(a.iq) + p0;
                if (a.iq_vec && nvalid == 8) {
                    *reinterpret_cast<uint4 *>(o) = make_uint4(w[0], w[1], w[2], w[3]);
                    *reinterpret_cast<uint4 *>(o + 4) = make_uint4(w[4], w[5], w[6], w[7]);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if ((uint32_t)k < nvalid) o[k] = w[k];
                }
            }
            if (a.soft) {
                int16_t *o = a.soft + p0;
                if (a.soft_vec && nvalid == 8) {
                    *reinterpret_cast<uint4 *>(o) = make_uint4(sv[0], sv[1], sv[2], sv[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if ((uint32_t)k < nvalid) o[k] = (int16_t)(sv[k / 2] >> (16 * (k & 1)));
                }
            }
            if (a.bits) reinterpret_cast<uint8_t *>(a.bits)[p0 / 8] = (uint8_t)(byte & ((1u << nvalid) - 1u));
        }
        // the bytes between the last block and the end of the last word
        if (a.bits && tile == ntiles - 1 && t < 8) {
            const uint64_t at = g.nblocks * L8 + t;
            if (at < out_bytes) reinterpret_cast<uint8_t *>(a.bits)[at] = 0;
        }
    }
}

}  // namespace

int carrier_launch(const CarrierLaunch &a, const CarrierRom &rom, int cus, hipStream_t st) {
    const uint64_t cap = (uint64_t)std::max(1, cus) * kCarrierGridPerCu;
    const CarrierGeom &g = a.g;
    const unsigned tiles = (unsigned)std::min(carrier_ntiles(g), cap), chunks = a.nflag;      // a.nflag = min(nchunks, cap): the flag kernel's words
    if (g.nblocks) {
        carrier_sum_kernel<<<tiles, kCarrierThreads, 0, st>>>(a);
        carrier_flag_kernel<<<chunks, kCarrierThreads, 0, st>>>(a);
    }
    carrier_chain_kernel<<<1, kCarrierThreads, 0, st>>>(a);
    if (g.nblocks) {
        carrier_est_kernel<<<chunks, kCarrierThreads, 0, st>>>(a);
        if (a.iq || a.bits || a.soft) carrier_rotate_kernel<<<tiles, kCarrierThreads, 0, st>>>(a, rom);
    }
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
