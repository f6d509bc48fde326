// dfe_kernels.hip -- the exact decision-feedback equalizer over int16 samples (include/bbb.h, bbb_dfe_run).
//
//   a[k] = acc(phase + k * decim)      v[k] = a[k] - sum_{i < nfb} fb[i] d[k - 1 - i]      bit[k] = v[k] >= threshold
// A decision depends on the nfb decisions before it, so the symbols cannot simply be handed out to threads.  What can be is
// the symbol's MAP (dfe_common.hpp): the NS = 2^nfb states it may be entered in onto the states it leaves, NS nibbles of one
// 64-bit word.  A workgroup walks a run of symbols in the filter's steps (the 2048 inputs of a step and the history in front
// of them in LDS, fir_common.hpp's image; fir_point gives a thread the feed-forward sum of one symbol) and every step in
// rounds of 256 symbols:
//   * a lane forms its symbol's decisions under every state, D, and from them its map;
//   * the wave scans the maps (Kogge-Stone over __shfl_up: six composes), its last lane leaves the wave's total in LDS;
//   * after one barrier every thread takes the round's start state through the totals of the waves in front of it and
//     through its exclusive prefix: that is the state its symbol is entered in; the bit is read out of D, a ballot packs
//     64 of them, the soft value is a - F(state);
//   * every thread carries the round's start state on through the four totals.  Thread h < NS carries a second state the
//     same way, the one a walk entered in state h would be in: the NS of them are the walk's map, at no compose at all.
// At decim 1 a step holds 2048 symbols and the block form takes it in ONE round: fir_block8 gives a thread the sums of its eight
// consecutive symbols, the thread composes their eight maps itself, the scan and the chain run over the threads' totals as
// above, and the thread then walks its eight symbols from its start state: one byte of the packed output.  That is 14
// composes for eight symbols where eight rounds of the point form would take 48.
// Nothing but bits, soft values and two words per region reaches memory.
//
// Regions (dfe_common.hpp has the rules): dfe_region_kernel gives every region its warm-up, a proven or speculated start and
// its outputs from that start; dfe_chain_kernel (one workgroup) composes the regions' maps into every region's true start,
// lists the regions that started wrong and writes the call's final state; dfe_repair_kernel walks the listed regions again
// from their true start.  The three are queued back to back; the scheme is exact whatever the data are, and costs one more
// walk only of the regions whose speculation failed.
#include "dfe_launch.hpp"
#include "fir_common.hpp"

#include <algorithm>

namespace bbb {
namespace {

static_assert(kDfeStepSamples == kFirTile && kDfeThreads == kFirThreads, "the walk stages fir_common.hpp's image");

struct DfeShared {
    __attribute__((aligned(16))) uint32_t img[kFirLdsWords];
    uint64_t tot[2][kDfeThreads / kWave];          // the waves' totals of a round; rounds alternate between the two rows
    uint32_t ends[1 << kDfeMaxFb];                 // thread h's second state at the end of a walk
};

constexpr int kMaps = 0, kWrite = 1, kRewrite = 2;

// The symbols [k_lo, k_hi), k_lo < k_hi, entered in state s; s and m2 (the thread's second state) leave as they are behind
// k_hi - 1.  kMaps: no output (a warm-up).  kWrite: bits into the zeroed output, soft values.  kRewrite: the same over what
// an earlier walk of these symbols wrote.
template <int NS, int MODE, bool BLOCK>
__device__ __forceinline__ void dfe_walk(const DfeLaunch &a, DfeShared &S, uint64_t k_lo, uint64_t k_hi, uint32_t &s, uint32_t &m2) {
    const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave, ng = (int)a.ngroups;
    const uint64_t step_lo = (a.phase + k_lo * a.decim) / kFirTile, step_hi = (a.phase + (k_hi - 1) * a.decim) / kFirTile;
    // a step's samples are loaded while the step before it is walked, as fir_kernel does
    uint4 own, lead;
    auto load = [&](uint64_t step) {
        own = fir_load8(a, (int64_t)(step * kFirTile) + 8 * t);
        lead = t < ng ? fir_load8(a, (int64_t)(step * kFirTile) - 8 * (t + 1)) : make_uint4(0, 0, 0, 0);
    };
    load(step_lo);
    for (uint64_t step = step_lo; step <= step_hi; ++step) {
        const uint64_t base = step * kFirTile;
        __syncthreads();                           // the image's readers of the step before are done
        *reinterpret_cast<uint4 *>(S.img + kFirHist / 2 + 4 * t) = own;
        if (t < ng) *reinterpret_cast<uint4 *>(S.img + kFirHist / 2 - 4 * (t + 1)) = lead;
        if (step < step_hi) load(step + 1);
        __syncthreads();
        uint64_t q_lo, q_hi;
        dfe_step_symbols(base, a.decim, a.phase, k_lo, k_hi, q_lo, q_hi);
        // what every form does with its lane's total m of a round: the scan, the waves' totals, the carried states; returns the
        // state in front of the lane's first symbol
        auto chain = [&](uint64_t m, int row) {
            if constexpr (NS > 1) {
#pragma unroll
                for (int d = 1; d < kWave; d <<= 1) {
                    const uint64_t before = __shfl_up((unsigned long long)m, d);
                    if (lane >= d) m = dfe_compose<NS>(before, m);
                }
            }
            uint64_t excl = __shfl_up((unsigned long long)m, 1);
            if (lane == 0) excl = dfe_identity<NS>();
            if (lane == kWave - 1) S.tot[row][w] = m;
            __syncthreads();
            // (a thread of the round after next writes this row again behind the next round's barrier)
            uint32_t sw = s;
#pragma unroll
            for (int j = 0; j < kDfeThreads / kWave; ++j) {
                const uint64_t tj = S.tot[row][j];
                if (j < w) sw = dfe_apply(tj, sw);
                s = dfe_apply(tj, s);
                m2 = dfe_apply(tj, m2);
            }
            return dfe_apply(excl, sw);
        };
        auto put_soft = [&](uint64_t q, int acc, uint32_t state) {
            const int v = dfe_v(acc, a.rule, state);
            if (a.soft_bytes == 2) reinterpret_cast<int16_t *>(a.soft)[q] = (int16_t)sat16(v >> a.shift);
            else reinterpret_cast<int32_t *>(a.soft)[q] = v;
        };
        if constexpr (BLOCK) {
            // decim 1: symbol q is input q, the thread's are q0 + r, r in [lo, hi)
            const uint64_t q0 = base + 8 * (uint64_t)t;
            const int lo = (int)min((uint64_t)8, q_lo > q0 ? q_lo - q0 : 0), hi = (int)min((uint64_t)8, q_hi > q0 ? q_hi - q0 : 0);
            int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (lo < hi) fir_block8(S.img, t, (unsigned)ng, a.taps, acc);
            uint32_t D[8];
            uint64_t m = dfe_identity<NS>();
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                D[r] = dfe_decisions<NS>(acc[r], a.rule);
                if (r >= lo && r < hi) m = dfe_compose<NS>(m, dfe_map<NS>(D[r]));
            }
            uint32_t mine = chain(m, 0);
            if constexpr (MODE != kMaps) {
                uint32_t byte = 0;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    if (r >= lo && r < hi) {
                        const uint32_t bit = D[r] >> mine & 1;
                        byte |= bit << r;
                        if (a.soft) put_soft(q0 + r, acc[r], mine);
                        mine = (mine << 1 | bit) & (uint32_t)(NS - 1);
                    }
                }
                if (lo < hi) {
                    const uint32_t mask = (1u << hi) - (1u << lo);
                    if (mask == 0xFFu) reinterpret_cast<uint8_t *>(a.bits)[q0 >> 3] = (uint8_t)byte;
                    else {
                        // a byte that two regions share, or the record's last: into its dword
                        unsigned *word = reinterpret_cast<unsigned *>(a.bits) + (q0 >> 5);
                        const unsigned sh = (unsigned)(q0 >> 3 & 3) * 8;
                        if constexpr (MODE == kRewrite) atomicAnd(word, ~(mask << sh));
                        atomicOr(word, byte << sh);
                    }
                }
            }
        } else {
            int row = 0;
            for (uint64_t rb = q_lo & ~63ull; rb < q_hi; rb += kDfeThreads, row ^= 1) {
                const uint64_t q = rb + (uint64_t)t;
                const bool valid = q >= q_lo && q < q_hi;
                int acc1[1] = {0};
                const uint32_t *const img[1] = {S.img};
                if (valid) fir_point(img, (int)(a.phase + q * a.decim - base) + kFirHist - 1, ng, a.taps, acc1);
                const uint32_t D = dfe_decisions<NS>(acc1[0], a.rule);
                const uint32_t mine = chain(valid ? dfe_map<NS>(D) : dfe_identity<NS>(), row);
                if constexpr (MODE != kMaps) {
                    const unsigned long long bits = __ballot(valid && (D >> mine & 1)), vmask = __ballot(valid);
                    if (lane == 0 && vmask) {
                        unsigned long long *word = reinterpret_cast<unsigned long long *>(a.bits) + ((rb >> 6) + (uint64_t)w);
                        if (vmask == ~0ull) *word = bits;
                        else {
                            if constexpr (MODE == kRewrite) atomicAnd(word, ~vmask);
                            atomicOr(word, bits);
                        }
                    }
                    if (valid && a.soft) put_soft(q, acc1[0], mine);
                }
            }
        }
    }
}

// the walk's map from the threads' second states
template <int NS>
__device__ __forceinline__ uint64_t dfe_gather(DfeShared &S, uint32_t m2) {
    if (threadIdx.x < NS) S.ends[threadIdx.x] = m2;
    __syncthreads();                               // (the next gather's writes come behind the barriers of a walk)
    uint64_t m = 0;
#pragma unroll
    for (int h = 0; h < NS; ++h) m |= (uint64_t)S.ends[h] << (4 * h);
    return m;
}

template <int NS, bool BLOCK>
__global__ __launch_bounds__(kDfeThreads) void dfe_region_kernel(DfeLaunch a) {
    __shared__ DfeShared S;
    const uint32_t first = *a.state & (uint32_t)(NS - 1), h = threadIdx.x & (NS - 1);
    for (uint64_t r = blockIdx.x; r < a.nreg; r += gridDim.x) {
        const uint64_t r_lo = r * a.region, r_hi = min(a.nsym, r_lo + a.region);
        uint32_t start = first;
        bool proven = true;
        if (r) {
            uint32_t s = 0, m2 = h;
            dfe_walk<NS, kMaps, BLOCK>(a, S, r_lo > a.warmup ? r_lo - a.warmup : 0, r_lo, s, m2);
            start = dfe_start<NS>(dfe_gather<NS>(S, m2), proven);
        }
        uint32_t s = start, m2 = h;
        dfe_walk<NS, kWrite, BLOCK>(a, S, r_lo, r_hi, s, m2);
        const uint64_t mr = dfe_gather<NS>(S, m2);
        if (threadIdx.x == 0) {
            a.rec[2 * r] = mr;
            a.rec[2 * r + 1] = dfe_info(start, proven);
        }
    }
}

template <int NS>
__global__ __launch_bounds__(kDfeChainThreads) void dfe_chain_kernel(DfeLaunch a) {
    __shared__ uint64_t tot[kDfeChainThreads];
    __shared__ unsigned nwrong, nunproven;
    const unsigned t = threadIdx.x;
    const uint64_t per = dfe_chain_share(a.nreg), lo = min(a.nreg, t * per), hi = min(a.nreg, lo + per);
    if (t == 0) nwrong = nunproven = 0;
    // the call's state word is read by every thread HERE, in front of the first barrier, and written by the last thread behind
    // the second: no load of it can come after the store
    uint32_t s = *a.state & (uint32_t)(NS - 1);
    tot[t] = dfe_chain_total<NS>(a.rec, lo, hi);
    __syncthreads();
    for (unsigned j = 0; j < t; ++j) s = dfe_apply(tot[j], s);
    uint32_t unproven = 0;
    s = dfe_chain_replay(a.rec, lo, hi, s, unproven, [&](uint64_t r, uint32_t true_start) {
        a.flagged[atomicAdd(&nwrong, 1u)] = dfe_flag(r, true_start);
    });
    if (unproven) atomicAdd(&nunproven, unproven);
    __syncthreads();
    if (t == kDfeChainThreads - 1) *a.state = s;   // behind the last thread's share: behind the call's last symbol
    if (t == 0) {
        a.flagged[a.nreg] = nwrong;
        if (a.stats) {
            a.stats[0] += a.nreg;
            a.stats[1] += nunproven;
            a.stats[2] += nwrong;
            a.stats[3] += a.nsym;
        }
    }
}

template <int NS, bool BLOCK>
__global__ __launch_bounds__(kDfeThreads) void dfe_repair_kernel(DfeLaunch a) {
    __shared__ DfeShared S;
    const uint64_t n = a.flagged[a.nreg];
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint64_t e = a.flagged[i], r = e & 0xFFFFFFFFull;
        const uint64_t r_lo = r * a.region, r_hi = min(a.nsym, r_lo + a.region);
        uint32_t s = (uint32_t)(e >> 32), m2 = 0;
        dfe_walk<NS, kRewrite, BLOCK>(a, S, r_lo, r_hi, s, m2);
    }
}

template <int NS, bool BLOCK>
int launch_form(const DfeLaunch &a, int cus, hipStream_t st) {
    const unsigned cap = (unsigned)std::max(1, cus) * 8;
    if (a.nreg) dfe_region_kernel<NS, BLOCK><<<(unsigned)std::min<uint64_t>(a.nreg, cap), kDfeThreads, 0, st>>>(a);
    dfe_chain_kernel<NS><<<1, kDfeChainThreads, 0, st>>>(a);
    // region 0 starts from the call's own state: only the regions behind it can have started wrong
    if (a.nreg > 1) dfe_repair_kernel<NS, BLOCK><<<(unsigned)std::min<uint64_t>(a.nreg - 1, cap), kDfeThreads, 0, st>>>(a);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

template <int NS>
int launch(const DfeLaunch &a, int cus, hipStream_t st) {
    return a.decim == 1 ? launch_form<NS, true>(a, cus, st) : launch_form<NS, false>(a, cus, st);
}

}  // namespace

int dfe_launch(const DfeLaunch &a, int cus, hipStream_t st) {
    switch (a.nfb) {
    case 0: return launch<1>(a, cus, st);
    case 1: return launch<2>(a, cus, st);
    case 2: return launch<4>(a, cus, st);
    case 3: return launch<8>(a, cus, st);
    default: return launch<16>(a, cus, st);
    }
}

}  // namespace bbb
