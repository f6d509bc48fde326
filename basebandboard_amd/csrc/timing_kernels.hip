// timing_kernels.hip -- the exact symbol timing recovery over int16 samples (include/bbb.h, bbb_timing_run).
//
//   a(n) = acc(n)      E_j[p] = sum_i |a(j L P + i P + p) - threshold|      the tracker moves its phase by at most one per block
// The tracker is a serial loop over the blocks, but what a block does to the phase depends on the block's metric alone: a
// block is a MAP of the P phases onto themselves (timing_common.hpp), and maps compose.  Five kernels, queued back to back:
//   * timing_metric_kernel: a workgroup stages a tile of 2048 samples and the history in front of it (fir_common.hpp's
//     image), fir_block8 gives every thread eight filtered samples, their |a - threshold| go into LDS, and `split` lanes per
//     (block, phase) pair add up the pair's terms, a stride of P apart -- no atomics, a fixed order.  A block of up to a tile:
//     the tile holds several whole blocks.  A longer block: the sums run on over its tiles in registers.  The block's map and,
//     for the call's first block, its arg-max are all that reaches memory.
//   * timing_chunk_kernel: a chunk of blocks is walked from every start phase at once, one lane per phase, over maps staged
//     in LDS: the chunk's map and the bits it emits from every start.
//   * timing_chain_kernel (one workgroup): threads compose the maps of their share of the chunks, one thread chains the
//     shares, and every thread replays its share from its true start: every chunk's start phase and output bit.  It
//     writes the state words and the bit count.
//   * timing_walk_kernel: every chunk is walked once more from its true start by one lane: phi_j, the wrap and the output
//     bit of every block, and the counters.
//   * timing_gather_kernel: a tile's instants are consecutive output bits; a thread takes one through fir_point, a wave's
//     ballot is shifted into the one or two output words it covers.  A word that the ballot covers whole is stored, a shared
//     one is ORed into the zeroed output.
// The filtered samples never reach memory.  The result never depends on the data or on chunk_blocks.
#include "timing_launch.hpp"
#include "fir_common.hpp"

#include <algorithm>

namespace bbb {
namespace {

static_assert(kTimingTile == (uint32_t)kFirTile && kTimingThreads == kFirThreads, "the passes stage fir_common.hpp's image");

constexpr int kTimingMaxSeg = 96;                  // blocks of a tile: at most 2048 / (8 * 3) = 85

struct TimingIn {                                  // what fir_load8 reads
    const int16_t *in;
    uint64_t nin;
    uint32_t nbefore;
    int in_vec;
};

// a tile's samples on their way into the image: loaded while the tile before is worked on, as fir_kernel does
struct TimingRegs {
    uint4 own, lead;
};
__device__ __forceinline__ TimingRegs timing_load(const TimingLaunch &a, uint64_t base) {
    const int t = threadIdx.x;
    const TimingIn src{a.in, a.g.nin, a.nbefore, a.in_vec && !(base & 7)};
    TimingRegs r;
    r.own = fir_load8(src, (int64_t)base + 8 * t);
    r.lead = t < (int)a.ngroups ? fir_load8(src, (int64_t)base - 8 * (t + 1)) : make_uint4(0, 0, 0, 0);
    return r;
}
__device__ __forceinline__ void timing_commit(const TimingLaunch &a, uint32_t *img, const TimingRegs &r) {
    const int t = threadIdx.x;
    __syncthreads();                               // the readers of the tile before are done
    *reinterpret_cast<uint4 *>(img + kFirHist / 2 + 4 * t) = r.own;
    if (t < (int)a.ngroups) *reinterpret_cast<uint4 *>(img + kFirHist / 2 - 4 * (t + 1)) = r.lead;
    __syncthreads();
}

struct MetricShared {
    __attribute__((aligned(16))) uint32_t img[kFirLdsWords];
    __attribute__((aligned(16))) uint32_t vals[kTimingTile];
    uint64_t E[kTimingThreads];
};

__global__ __launch_bounds__(kTimingThreads) void timing_metric_kernel(TimingLaunch a) {
    __shared__ MetricShared S;
    const TimingGeom &g = a.g;
    const uint32_t t = threadIdx.x, T = timing_tiles_per_block(g.LP);
    const uint32_t pair = t / a.split, s = t % a.split, jb = pair / g.P, p = pair % g.P;
    const uint64_t ngroups = timing_ngroups(g);
    if (blockIdx.x >= ngroups) return;
    TimingRegs regs = timing_load(a, timing_tile(g, (uint64_t)blockIdx.x * T).base);
    for (uint64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        uint64_t sum = 0;
        TimingTile tl;
        for (uint32_t o = 0; o < T; ++o) {
            tl = timing_tile(g, grp * T + o);
            timing_commit(a, S.img, regs);
            if (o + 1 < T) regs = timing_load(a, timing_tile(g, grp * T + o + 1).base);
            else if (grp + gridDim.x < ngroups) regs = timing_load(a, timing_tile(g, (grp + gridDim.x) * T).base);
            int acc[8];
            fir_block8(S.img, (int)t, a.ngroups, a.taps, acc);
            uint32_t v[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = tl.base + 8 * t + r < g.nin ? timing_term(acc[r], a.threshold) : 0u;
            *reinterpret_cast<uint4 *>(S.vals + 8 * t) = make_uint4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<uint4 *>(S.vals + 8 * t + 4) = make_uint4(v[4], v[5], v[6], v[7]);
            __syncthreads();
            if (jb < tl.nblk) {
                uint32_t k0, kend;
                timing_pair_span(g, tl, jb, p, k0, kend);
                for (uint32_t k = k0 + s * g.P; k < kend; k += a.split * g.P) sum += S.vals[k];
            }
        }
        for (uint32_t d = a.split >> 1; d; d >>= 1) sum += __shfl_xor((unsigned long long)sum, (int)d);
        if (s == 0 && jb < tl.nblk) S.E[pair] = sum;
        __syncthreads();                           // (E and vals are written again behind the barriers of the next commit)
        if (t < tl.nblk * g.P) {
            const uint32_t b = t / g.P, phi = t % g.P;
            a.mv[(tl.j0 + b) * g.P + phi] = (uint8_t)(timing_move_at(S.E + b * g.P, g.P, phi, g.h) + 1);
        }
        if (t == 0 && tl.j0 == 0) a.hdr[1] = timing_argmax(S.E, g.P);
    }
}

// n bytes of move maps into LDS
__device__ __forceinline__ void timing_stage_maps(uint8_t *stage, const uint8_t *src, uint32_t n) {
    const uint32_t t = threadIdx.x;
    __syncthreads();                               // the walk of the maps before is done
    if (!((uintptr_t)src & 3)) {
        for (uint32_t i = t; i < n / 4; i += kTimingThreads) reinterpret_cast<uint32_t *>(stage)[i] = reinterpret_cast<const uint32_t *>(src)[i];
        for (uint32_t i = (n & ~3u) + t; i < n; i += kTimingThreads) stage[i] = src[i];
    } else {
        for (uint32_t i = t; i < n; i += kTimingThreads) stage[i] = src[i];
    }
    __syncthreads();
}

__global__ __launch_bounds__(kTimingThreads) void timing_chunk_kernel(TimingLaunch a) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kTimingStage];
    const TimingGeom &g = a.g;
    const uint32_t t = threadIdx.x, P = g.P, sb = kTimingStage / P;
    const bool unlocked = !(a.state[0] & kTimingLocked);
    const uint32_t first_phi = a.init_phase < P ? a.init_phase : (uint32_t)a.hdr[1];
    for (uint64_t c = blockIdx.x; c < g.nchunks; c += gridDim.x) {
        const uint64_t j_lo = c * g.chunk, j_hi = min(g.nblocks, j_lo + g.chunk);
        uint32_t phi = t < P ? t : 0, nb = 0;
        for (uint64_t j0 = j_lo; j0 < j_hi; j0 += sb) {
            const uint32_t n = (uint32_t)min((uint64_t)sb, j_hi - j0);
            timing_stage_maps(stage, a.mv + j0 * P, n * P);
            if (t < P) {
                for (uint32_t b = 0; b < n; ++b) {
                    int m, w;
                    nb += timing_walk_block(g, j0 + b, unlocked && j0 + b == 0, first_phi, stage[b * P + phi], phi, m, w);
                }
            }
        }
        if (t < P) {
            a.cmap[c * P + t] = (uint8_t)phi;
            a.cbits[c * P + t] = nb;
        }
    }
}

__global__ __launch_bounds__(kTimingThreads) void timing_chain_kernel(TimingLaunch a) {
    __shared__ uint64_t totbits[kTimingChainSlots];
    __shared__ uint64_t soff[kTimingThreads];
    __shared__ uint8_t totmap[kTimingChainSlots];
    __shared__ uint8_t start[kTimingThreads];
    __shared__ uint64_t total;
    __shared__ uint32_t endphi;
    const TimingGeom &g = a.g;
    const uint32_t t = threadIdx.x, P = g.P, T = timing_chain_threads(P);
    const uint64_t share = timing_chain_share(g.nchunks, P), lo = min(g.nchunks, t * share), hi = min(g.nchunks, lo + share);
    // the state words are read by every thread HERE, in front of the first barrier, and written by thread 0 behind the
    // second: no load of them can come after the store
    const uint64_t s0 = a.state[0], s1 = a.state[1];
    if (t < T) {
        for (uint32_t phi0 = 0; phi0 < P; ++phi0) {
            uint32_t phi = phi0;
            uint64_t nb = 0;
            for (uint64_t c = lo; c < hi; ++c) timing_compose(a.cmap, a.cbits, c, P, phi, nb);
            totmap[t * P + phi0] = (uint8_t)phi;
            totbits[t * P + phi0] = nb;
        }
    }
    __syncthreads();
    if (t == 0) {
        uint32_t phi = timing_state_phi(s0, P);
        uint64_t off = 0;
        for (uint32_t k = 0; k < T; ++k) {
            start[k] = (uint8_t)phi;
            soff[k] = off;
            off += totbits[k * P + phi];
            phi = totmap[k * P + phi];
        }
        total = off;
        endphi = phi;
    }
    __syncthreads();
    if (t < T) {
        uint32_t phi = start[t];
        uint64_t off = soff[t];
        for (uint64_t c = lo; c < hi; ++c) {
            a.cstart[c] = (uint8_t)phi;
            a.coff[c] = off;
            timing_compose(a.cmap, a.cbits, c, P, phi, off);
        }
    }
    if (t == 0) {
        a.hdr[0] = !(s0 & kTimingLocked);
        a.state[0] = g.nblocks ? kTimingLocked | endphi : s0;
        a.state[1] = s1 + total;
        *a.nbits = total;
        if (a.stats) a.stats[0] += g.nblocks;
    }
}

__global__ __launch_bounds__(kTimingThreads) void timing_walk_kernel(TimingLaunch a) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kTimingStage];
    const TimingGeom &g = a.g;
    const uint32_t t = threadIdx.x, P = g.P, sb = kTimingStage / P;
    const bool unlocked = a.hdr[0] != 0;
    const uint32_t first_phi = a.init_phase < P ? a.init_phase : (uint32_t)a.hdr[1];
    for (uint64_t c = blockIdx.x; c < g.nchunks; c += gridDim.x) {
        const uint64_t j_lo = c * g.chunk, j_hi = min(g.nblocks, j_lo + g.chunk);
        uint32_t phi = a.cstart[c], moves = 0, up = 0, dn = 0;
        uint64_t off = a.coff[c];
        for (uint64_t j0 = j_lo; j0 < j_hi; j0 += sb) {
            const uint32_t n = (uint32_t)min((uint64_t)sb, j_hi - j0);
            timing_stage_maps(stage, a.mv + j0 * P, n * P);
            if (t == 0) {
                for (uint32_t b = 0; b < n; ++b) {
                    const uint64_t j = j0 + b;
                    int m, w;
                    const uint32_t cnt = timing_walk_block(g, j, unlocked && j == 0, first_phi, stage[b * P + phi], phi, m, w);
                    if (a.phase) a.phase[j] = (uint8_t)phi;
                    a.boff[j] = off;
                    a.binfo[j] = timing_info(phi, w);
                    off += cnt;
                    moves += m != 0;
                    up += w > 0;
                    dn += w < 0;
                }
            }
        }
        if (t == 0 && a.stats) {
            if (moves) atomicAdd((unsigned long long *)a.stats + 1, (unsigned long long)moves);
            if (up) atomicAdd((unsigned long long *)a.stats + 2, (unsigned long long)up);
            if (dn) atomicAdd((unsigned long long *)a.stats + 3, (unsigned long long)dn);
        }
    }
}

struct GatherShared {
    __attribute__((aligned(16))) uint32_t img[kFirLdsWords];
    uint64_t seg_start[kTimingMaxSeg + 1];         // the output bit of a block's first instant in this tile; [nblk]: the tile's end
    int seg_ilo[kTimingMaxSeg];
    uint32_t seg_phi[kTimingMaxSeg];
};

__global__ __launch_bounds__(kTimingThreads) void timing_gather_kernel(TimingLaunch a, uint64_t max_bits) {
    __shared__ GatherShared S;
    const TimingGeom &g = a.g;
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const int ng = (int)a.ngroups;
    const uint64_t ntiles = timing_ntiles(g);
    if (blockIdx.x >= ntiles) return;
    TimingRegs regs = timing_load(a, timing_tile(g, blockIdx.x).base);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const TimingTile tl = timing_tile(g, tile);
        // a block's record: asked for in front of the commit's barriers
        uint64_t off = 0;
        uint16_t info = 0;
        if (t < tl.nblk) {
            off = a.boff[tl.j0 + t];
            info = a.binfo[tl.j0 + t];
        }
        timing_commit(a, S.img, regs);             // (the readers of the segments before are done as well)
        if (tile + gridDim.x < ntiles) regs = timing_load(a, timing_tile(g, tile + gridDim.x).base);
        if (t < tl.nblk) {
            const uint32_t phi = timing_info_phi(info);
            const int w = timing_info_wrap(info);
            int ilo, ihi;
            timing_tile_instants(g, tl, tl.j0 + t, phi, w, ilo, ihi);
            S.seg_start[t] = off + (uint64_t)(ilo - w);
            S.seg_ilo[t] = ilo;
            S.seg_phi[t] = phi;
            if (t == tl.nblk - 1) S.seg_start[tl.nblk] = off + (uint64_t)(ihi - w);
        }
        __syncthreads();
        const uint64_t lo = S.seg_start[0];
        const uint32_t n = (uint32_t)(S.seg_start[tl.nblk] - lo);
        for (uint32_t r0 = 0; r0 < n; r0 += kTimingThreads) {
            const uint32_t r = r0 + t;
            const bool valid = r < n && lo + r < max_bits;
            bool bit = false;
            if (valid) {
                uint32_t b0 = 0, b1 = tl.nblk;                   // the last block that starts at or before r
                while (b1 - b0 > 1) {
                    const uint32_t mid = (b0 + b1) / 2;
                    if ((uint32_t)(S.seg_start[mid] - lo) <= r) b0 = mid;
                    else b1 = mid;
                }
                const int i = S.seg_ilo[b0] + (int)(r - (uint32_t)(S.seg_start[b0] - lo));
                const int k = (int)(b0 * g.LP) - (int)tl.off + (int)S.seg_phi[b0] + i * (int)g.P;      // in [-1, 2048)
                int acc1[1] = {0};
                const uint32_t *const img[1] = {S.img};
                fir_point(img, k + kFirHist - 1, ng, a.taps, acc1);
                bit = a.strict ? acc1[0] > a.threshold : acc1[0] >= a.threshold;
                if (a.soft) {
                    if (a.soft_bytes == 2) reinterpret_cast<int16_t *>(a.soft)[lo + r] = (int16_t)sat16(acc1[0] >> a.shift);
                    else reinterpret_cast<int32_t *>(a.soft)[lo + r] = acc1[0];
                }
            }
            const unsigned long long bal = __ballot(bit), vmask = __ballot(valid);
            if (lane == 0 && vmask) {
                const uint64_t pos = lo + r0 + (uint64_t)wv * kWave;
                const unsigned sh = (unsigned)(pos & 63);
                unsigned long long *word = reinterpret_cast<unsigned long long *>(a.bits) + (pos >> 6);
                if (sh == 0 && vmask == ~0ull) *word = bal;
                else {
                    if (bal << sh) atomicOr(word, bal << sh);
                    if (sh && (bal >> (64 - sh))) atomicOr(word + 1, bal >> (64 - sh));
                }
            }
        }
    }
}

}  // namespace

int timing_launch(const TimingLaunch &a, int cus, hipStream_t st) {
    const uint64_t cap = (uint64_t)std::max(1, cus) * 8;
    const TimingGeom &g = a.g;
    uint64_t nblocks, nconsumed, max_bits;
    timing_plan(g.P, g.L, g.nin, true, nblocks, nconsumed, max_bits);
    if (g.nblocks) {
        timing_metric_kernel<<<(unsigned)std::min(timing_ngroups(g), cap), kTimingThreads, 0, st>>>(a);
        timing_chunk_kernel<<<(unsigned)std::min(g.nchunks, cap), kTimingThreads, 0, st>>>(a);
    }
    timing_chain_kernel<<<1, kTimingThreads, 0, st>>>(a);
    if (g.nblocks) {
        timing_walk_kernel<<<(unsigned)std::min(g.nchunks, cap), kTimingThreads, 0, st>>>(a);
        timing_gather_kernel<<<(unsigned)std::min(timing_ntiles(g), cap), kTimingThreads, 0, st>>>(a, max_bits);
    }
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
