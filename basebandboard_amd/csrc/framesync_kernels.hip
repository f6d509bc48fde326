// framesync_kernels.hip -- the frame synchroniser on the device (include/bbb.h, bbb_framesync_run, bbb_frame_extract and
// bbb_frame_attach).  framesync_common.hpp has the per-lane core.
//
// The search pass (all compute units).  A lane owns a word of 64 positions: from the data's word and the next one (the lane
// above's, by a shuffle) it makes the 64 windows by funnel shifts, XORs the marker, counts bits and compares, and stores ONE word
// of the candidate plane: bit i set where position 64 j + i is within tol_search in an allowed polarity and its marker lies
// inside the data.  A workgroup that found a candidate sets its bit of the tile flags.  Nothing else reaches memory.
//
// The chain pass (one workgroup) is the machine itself, exact whatever the data.
//   SEARCH  the lanes scan the tile flags from s, then the flagged tile's candidate words; a lane that holds candidates tests
//           their confirmations in order, straight from the data, until one is confirmed or cannot be decided yet; the smallest
//           such position wins by a reduction, and the candidates below it are the rejected ones.
//   LOCK    a round takes up to kFsBatch frames, four a lane with their loads in flight together; a wave's ballot gives the
//           misses of 64 consecutive frames, the masks meet in LDS, a lane that missed looks back over w frames for the run
//           that loses the lock, the first such frame ends the round and the records before it are written in order.
// Its time is rounds: a LOCK round per kFsBatch frames, a SEARCH round per flagged tile passed over (plus 64 candidates times v
// distances in one lane where a tile is full of rejected candidates), and one per change of mode.
//
// Extract: a lane makes one aligned 8-byte word of the output from the record it falls into (a funnel shift from the unaligned
// bit position, complement, table XOR); words that straddle two payloads go byte by byte.  Attach walks the other way round,
// one word of the packed output a lane.
#include "framesync_launch.hpp"

#include <algorithm>

namespace bbb {
namespace {

constexpr unsigned long long kFsNone = ~0ull;

// ---- the search pass ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kFsThreads) void fs_search_kernel(FsLaunch a) {
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1);
    const uint64_t nwords = fs_words(a.nbits), ntiles = fs_tiles(a.nbits);
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t j = tile * kFsTileWords + t;
        uint64_t cand = 0;
        const uint64_t w0 = j < nwords ? a.in[j] : 0;
        uint64_t w1 = (uint64_t)__shfl_down((unsigned long long)w0, 1);
        if (lane == kWave - 1) w1 = j + 1 < nwords ? a.in[j + 1] : 0;
        if (j < nwords) {
            const uint64_t valid = fs_valid_mask(j, a.nbits, a.c.M);
            if (valid) cand = fs_candidate_word(w0, w1, a.c) & valid;
            a.plane[j] = cand;
        }
        if (__syncthreads_or(cand != 0) && t == 0) atomicOr((unsigned long long *)&a.flags[tile >> 6], 1ull << (tile & 63));
    }
}

// ---- the chain pass -------------------------------------------------------------------------------------------------------------
struct FsShared {
    unsigned long long mm[kFsMaskWords];
    unsigned long long vmin;
    unsigned long long sum[2];
};

__device__ __forceinline__ unsigned long long fs_block_min(unsigned long long v, FsShared &sh) {
    if (threadIdx.x == 0) sh.vmin = kFsNone;
    __syncthreads();
    if (v != kFsNone) atomicMin(&sh.vmin, v);
    __syncthreads();
    const unsigned long long r = sh.vmin;
    __syncthreads();
    return r;
}

__device__ __forceinline__ void fs_block_sum2(unsigned long long &x, unsigned long long &y, FsShared &sh) {
    if (threadIdx.x == 0) sh.sum[0] = sh.sum[1] = 0;
    __syncthreads();
    if (x) atomicAdd(&sh.sum[0], x);
    if (y) atomicAdd(&sh.sum[1], y);
    __syncthreads();
    x = sh.sum[0];
    y = sh.sum[1];
    __syncthreads();
}

__global__ __launch_bounds__(kFsThreads) void fs_chain_kernel(FsLaunch a) {
    __shared__ FsShared sh;
    const uint32_t t = threadIdx.x, lane = t & (kWave - 1), wv = t / kWave;
    const FsCfg &c = a.c;
    const uint64_t n = a.nbits, nwords = fs_words(n), ntiles = fs_tiles(n), nfw = fs_flag_words(n);
    const uint64_t word0 = a.state[0], P = a.state[1];
    FsWord0 s = fs_unpack(word0);
    __syncthreads();                               // every lane has read the state before lane 0 can write it
    if (P < a.first_bit) {                         // the data begin behind the state's position: the flag and nothing else
        if (t == 0) a.state[0] = word0 | BBB_FRAMESYNC_ERROR;
        return;
    }
    // every lane carries the same machine: what differs between lanes meets in LDS and is read back by all
    uint64_t r = P - a.first_bit;                  // the position relative to the data; may lie beyond them
    uint64_t emitted = 0, fly = 0, acq = 0, losses = 0, rej = 0, mbe = 0;
    for (;;) {
        if (s.mode == kFsModeLock) {
            const uint64_t K = fs_lock_steps(r, n, c);
            if (!K) break;
            const uint32_t B = (uint32_t)min(K, (uint64_t)kFsBatch);
            uint32_t d[4];
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t j = t + kFsThreads * q;
                d[q] = j < B ? fs_dist(a.in, r + (uint64_t)j * c.F, s.pol, c) : 0u;
            }
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const unsigned long long bm = __ballot(d[q] > c.tol_lock);
                if (lane == 0) sh.mm[4 * q + wv] = bm;
            }
            __syncthreads();
            unsigned long long mine = kFsNone;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t j = t + kFsThreads * q;
                if (d[q] > c.tol_lock && mine == kFsNone && fs_miss_run((const uint64_t *)sh.mm, (int32_t)j, s.misses, c.w) > c.w) mine = j;
            }
            const uint32_t carried = fs_miss_run((const uint64_t *)sh.mm, (int32_t)B - 1, s.misses, c.w);
            const unsigned long long first_loss = fs_block_min(mine, sh);      // its barriers also free mm for the next round
            const uint32_t L = first_loss == kFsNone ? B : (uint32_t)first_loss;
            unsigned long long nfly = 0, nerr = 0;
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t j = t + kFsThreads * q;
                if (j < L) {
                    const bool miss = d[q] > c.tol_lock;
                    const uint64_t idx = emitted + j;
                    if (idx < a.max_frames) {
                        a.pos[idx] = a.first_bit + r + (uint64_t)j * c.F;
                        a.meta[idx] = fs_meta(d[q], s.pol, miss, s.fresh && j == 0);
                    }
                    nfly += miss;
                    if (!miss) nerr += d[q];
                }
            }
            fs_block_sum2(nfly, nerr, sh);
            fly += nfly;
            mbe += nerr;
            emitted += L;
            if (L) s.fresh = 0;
            r += (uint64_t)L * c.F;
            if (L < B) {
                s.mode = kFsModeSearch;
                s.misses = 0;
                ++losses;
            } else {
                s.misses = carried;
            }
        } else {
            if (!fs_search_open(r, n, c)) break;
            // the first flagged tile at or behind r's
            const uint64_t tile0 = (r >> 6) / kFsTileWords;
            unsigned long long tile = kFsNone;
            for (uint64_t base = tile0 >> 6; base < nfw && tile == kFsNone; base += kFsThreads) {
                const uint64_t i = base + t;
                uint64_t f = i < nfw ? a.flags[i] : 0;
                if (i == tile0 >> 6) f &= ~0ull << (tile0 & 63);
                tile = fs_block_min(f ? i * 64 + (uint64_t)__builtin_ctzll(f) : kFsNone, sh);
            }
            if (tile == kFsNone || tile >= ntiles) {
                r = n - c.M + 1;                   // no candidate up to the last position that can be one
                break;
            }
            const uint64_t j = tile * kFsTileWords + t;
            uint64_t cw = j < nwords ? a.plane[j] & fs_from_mask(j, r) : 0;
            unsigned long long res = kFsNone, myrej = 0;
            while (cw) {
                const uint64_t p = 64 * j + (uint64_t)__builtin_ctzll(cw);
                cw &= cw - 1;
                if (!a.final && !fs_candidate_open(p, n, c)) {
                    res = p << 2 | 3;
                    break;
                }
                const uint32_t pol = fs_candidate(fs_dist0(a.in, p, c), c) - 1;
                if (fs_confirm(a.in, p, pol, n, c)) {
                    res = p << 2 | (1 + pol);
                    break;
                }
                ++myrej;
            }
            const unsigned long long win = fs_block_min(res, sh);
            // the candidates below the winner were rejected: all those of the lanes below its lane, and its own before it
            unsigned long long nrej = win == kFsNone || j <= (win >> 2) >> 6 ? myrej : 0, unused = 0;
            fs_block_sum2(nrej, unused, sh);
            rej += nrej;
            if (win == kFsNone) {
                r = (tile + 1) * kFsTileBits;      // on to the next tile; r stays a position: the loop's head checks it
                if (!fs_search_open(r, n, c)) {
                    r = n - c.M + 1;
                    break;
                }
                continue;
            }
            r = win >> 2;
            if ((win & 3) == 3) break;             // not decidable yet: the state waits here
            s.mode = kFsModeLock;
            s.pol = (uint32_t)(win & 3) - 1;
            s.misses = 0;
            s.fresh = 1;
            ++acq;
        }
    }
    if (t == 0) {
        if (emitted > a.max_frames) s.overflow = 1;
        a.state[0] = fs_pack(s, emitted);
        a.state[1] = a.first_bit + r;
        a.state[2] += emitted;
        a.state[3] += fly;
        a.state[4] += acq;
        a.state[5] += losses;
        a.state[6] += rej;
        a.state[7] += mbe;
    }
}

// ---- extract and attach ---------------------------------------------------------------------------------------------------------
// the table's `period` bytes in LDS; the per-lane core wraps its index itself
__device__ __forceinline__ void fs_table_to_lds(const FsRand &R, uint8_t *tab2) {
    for (uint32_t i = threadIdx.x; i < R.period; i += blockDim.x) tab2[i] = R.tab[i];
    __syncthreads();
}

__global__ __launch_bounds__(kFsThreads) void fs_extract_kernel(FsLaunch a) {
    __shared__ uint8_t tab2[256];
    fs_table_to_lds(a.rnd, tab2);
    const FsCfg &c = a.c;
    const uint32_t PB = c.payload_bytes, period = a.rnd.period;
    const uint64_t count = min(a.state[0] >> 32, a.max_frames), total = count * PB;
    // the record's frame relative to the data, or kFsNone where it does not lie inside them
    auto frame_at = [&](uint64_t fi) -> uint64_t {
        const uint64_t p = a.pos[fi];
        return p >= a.first_bit && p - a.first_bit + c.F <= a.nbits ? p - a.first_bit : kFsNone;
    };
    for (uint64_t q = (uint64_t)blockIdx.x * kFsThreads + threadIdx.x; 8 * q < total; q += (uint64_t)gridDim.x * kFsThreads) {
        const uint64_t b = 8 * q;
        const uint32_t nb = (uint32_t)min((uint64_t)8, total - b);
        const uint64_t fi = total >> 32 ? b / PB : (uint64_t)((uint32_t)b / PB);
        const uint32_t off = (uint32_t)(b - fi * PB);
        uint64_t x = 0;
        if (off + nb <= PB) {
            const uint64_t p = frame_at(fi);
            if (p != kFsNone) x = fs_payload_word(a.in, p, off, nb, a.meta[fi] >> 8 & 1, c, tab2, period);
        } else {
            uint64_t f = fi;
            uint32_t o = off;
            for (uint32_t k = 0; k < nb; ++k) {
                const uint64_t p = frame_at(f);
                if (p != kFsNone) x |= fs_payload_word(a.in, p, o, 1, a.meta[f] >> 8 & 1, c, tab2, period) << (8 * k);
                if (++o == PB) {
                    o = 0;
                    ++f;
                }
            }
        }
        if (nb == 8) {
            *reinterpret_cast<uint64_t *>(a.out_bytes + b) = x;
        } else {
            for (uint32_t k = 0; k < nb; ++k) a.out_bytes[b + k] = (uint8_t)(x >> (8 * k));
        }
    }
}

__global__ __launch_bounds__(kFsThreads) void fs_attach_kernel(FsLaunch a) {
    __shared__ uint8_t tab2[256];
    fs_table_to_lds(a.rnd, tab2);
    const FsCfg &c = a.c;
    const uint64_t total = a.nframes * c.F, nwords = fs_words(total);
    for (uint64_t g = (uint64_t)blockIdx.x * kFsThreads + threadIdx.x; g < nwords; g += (uint64_t)gridDim.x * kFsThreads) {
        uint64_t fi = 64 * g / c.F;
        uint32_t o = (uint32_t)(64 * g - fi * c.F), filled = 0;
        uint64_t x = 0;
        while (filled < 64 && fi < a.nframes) {
            const uint32_t take = min(64u - filled, c.F - o);
            x |= fs_frame_bits(a.payload, fi, o, take, c, tab2, a.rnd.period) << filled;
            filled += take;
            o += take;
            if (o == c.F) {
                o = 0;
                ++fi;
            }
        }
        a.out_words[g] = x;
    }
}

unsigned fs_grid(uint64_t items, int cus) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + kFsThreads - 1) / kFsThreads, (uint64_t)std::max(1, cus) * 16));
}

}  // namespace

int fs_run_launch(const FsLaunch &a, int cus, hipStream_t st) {
    if (a.nbits) {
        BBB_HIP(hipMemsetAsync(a.flags, 0, 8 * fs_flag_words(a.nbits), st));
        fs_search_kernel<<<fs_grid(fs_words(a.nbits), cus), kFsThreads, 0, st>>>(a);
        BBB_HIP(hipGetLastError());
    }
    fs_chain_kernel<<<1, kFsThreads, 0, st>>>(a);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

int fs_extract_launch(const FsLaunch &a, int cus, hipStream_t st) {
    fs_extract_kernel<<<fs_grid(a.max_frames * a.c.payload_bytes / 8 + 1, cus), kFsThreads, 0, st>>>(a);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

int fs_attach_launch(const FsLaunch &a, int cus, hipStream_t st) {
    fs_attach_kernel<<<fs_grid(fs_words(a.nframes * a.c.F), cus), kFsThreads, 0, st>>>(a);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
