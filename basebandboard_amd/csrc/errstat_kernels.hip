// errstat_kernels.hip -- gap, burst and errored-block statistics of a packed error stream (include/bbb.h, bbb_errstat_*).
//
// The error positions e_0 < e_1 < ... are the set bits of err & ~mask.  Everything the statistics need of an error is its
// predecessor (the gap, the block comparison, whether a burst starts here) and, at an error that starts a burst, the burst it
// closes: its last error is the predecessor, its first the latest earlier burst start, its weight a difference of error counts.
// All three are PREFIX quantities, so nothing is scanned backwards and a zero word costs a load and a compare.
//
// Two launches per call, the data read once:
//   errstat_tile    one workgroup of 4 wavefronts per tile of kErrTileBits.  A wavefront owns kErrWaveBits and walks them in 8
//                   steps of 64 lanes x 2 words, the state between steps in (uniform) registers.  In a step with errors the
//                   predecessor of a lane's lowest error comes from the nearest lower lane that has one (one ballot, one
//                   shuffle), the error count before the lane from a prefix sum of popcounts, the latest burst start before the
//                   lane the same way once the lanes know their own.  Within a lane it is a walk over the set bits.  Every gap
//                   and every burst that lies inside the wavefront's range is binned there, into the workgroup's LDS
//                   histograms; what remains is a summary (Seg): count, first and last error, whether a burst break lies
//                   inside, and the partial bursts at the head and at the tail.  Thread 0 appends the four summaries (binning
//                   what their junctions decide) and writes the tile's; the histograms are flushed once.
//   errstat_stitch  one workgroup over the tile summaries.  Appending summaries is associative, so every thread reduces a
//                   run of them, the 512 aggregates are scanned in two levels behind the carried state (previous error and
//                   open burst, kept in the result on the device), and every thread walks its run again from its exclusive
//                   prefix, now binning what each junction decides.  No lane walks all tiles.  The same launch moves the
//                   carried state and the running position on.
// Ordering between workgroups comes from the two launches on one stream; no workgroup waits for another.
#include "bbb_common.hpp"

namespace bbb {

namespace {

constexpr int kTileThreads = 256;
constexpr int kWaves = 4;
constexpr int kSteps = 8;                          // steps of a wavefront
constexpr uint32_t kStepWords = 128;               // 64 lanes x 2 words
constexpr uint32_t kWaveWords = kSteps * kStepWords;
constexpr uint32_t kTileWords = kWaves * kWaveWords;
constexpr int kStitchThreads = 512;
constexpr int kBins = BBB_ERRSTAT_NBINS;
static_assert(kWaveWords * 64 == kErrWaveBits && kTileWords * 64 == kErrTileBits, "geometry");

struct ErrCfg {
    uint32_t guard, nblock;
    uint64_t block[4];                             // 0: unused
};

// What a run of positions leaves behind once everything interior to it is binned.
struct Seg {
    uint64_t n;                                    // errors; 0: empty, the rest means nothing
    uint64_t first, last;                          // first and last error
    uint64_t head_last, head_w;                    // with brk: last error and weight of the burst the run begins in
    uint64_t tail_first, tail_w;                   // first error and weight of the burst the run ends in (!brk: the whole run)
    uint32_t brk;                                  // a burst break lies inside
    uint32_t anchored;                             // the run begins where the record begins: its head is a whole burst's head
};

__device__ __forceinline__ uint32_t vbin(uint64_t v) { return v < 256 ? (uint32_t)v : 256u + (63u - (uint32_t)__clzll(v)) - 8u; }

__device__ __forceinline__ bool blocks_differ(uint64_t p, uint64_t t, uint64_t g, uint64_t B) { return g >= B || t / B != p / B; }

// LDS scalars of a tile
enum { SC_MAXGAP, SC_BURSTS, SC_BLSUM, SC_MAXBL, SC_MAXBW, SC_EB, SC_N = SC_EB + 4 };

struct NoSink {
    __device__ void first(uint64_t) {}
    __device__ void gap(uint64_t, uint64_t, uint64_t) {}
    __device__ void burst(uint64_t, uint64_t, uint64_t) {}
};

struct LdsSink {                                   // junctions inside a tile: all values below kErrTileBits
    uint32_t *hist, *sc;
    const ErrCfg &cfg;
    __device__ void first(uint64_t) {}
    __device__ void gap(uint64_t p, uint64_t t, uint64_t g) {
        atomicAdd(&hist[vbin(g)], 1u);
        atomicMax(&sc[SC_MAXGAP], (uint32_t)g);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (cfg.block[j] && blocks_differ(p, t, g, cfg.block[j])) atomicAdd(&sc[SC_EB + j], 1u);
    }
    __device__ void burst(uint64_t f, uint64_t l, uint64_t w) {
        const uint32_t len = (uint32_t)(l - f + 1);
        atomicAdd(&hist[kBins + vbin(len)], 1u);
        atomicAdd(&hist[2 * kBins + vbin(w)], 1u);
        atomicAdd(&sc[SC_BURSTS], 1u);
        atomicAdd(&sc[SC_BLSUM], len);
        atomicMax(&sc[SC_MAXBL], len);
        atomicMax(&sc[SC_MAXBW], (uint32_t)w);
    }
};

struct GlobalSink {                                // junctions between tiles and behind the carried state
    bbb_errstat_result *r;
    const ErrCfg &cfg;
    __device__ void first(uint64_t t) {
        r->first_error = t;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (cfg.block[j]) atomicAdd((unsigned long long *)&r->errored_blocks[j], 1ull);
    }
    __device__ void gap(uint64_t p, uint64_t t, uint64_t g) {
        atomicAdd((unsigned long long *)&r->gap_hist[vbin(g)], 1ull);
        atomicMax((unsigned long long *)&r->max_gap, (unsigned long long)g);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (cfg.block[j] && blocks_differ(p, t, g, cfg.block[j])) atomicAdd((unsigned long long *)&r->errored_blocks[j], 1ull);
    }
    __device__ void burst(uint64_t f, uint64_t l, uint64_t w) {
        const uint64_t len = l - f + 1;
        atomicAdd((unsigned long long *)&r->burst_len_hist[vbin(len)], 1ull);
        atomicAdd((unsigned long long *)&r->burst_weight_hist[vbin(w)], 1ull);
        atomicAdd((unsigned long long *)&r->bursts, 1ull);
        atomicAdd((unsigned long long *)&r->burst_len_sum, (unsigned long long)len);
        atomicMax((unsigned long long *)&r->max_burst_len, (unsigned long long)len);
        atomicMax((unsigned long long *)&r->max_burst_weight, (unsigned long long)w);
    }
};

// p := p followed by s.  The junction's gap and the bursts it completes go to the sink: the tail of p when the junction breaks,
// the head of s when s has a break inside, one burst of both when the junction does not break.  A burst whose first error is
// unknown -- it contains the first error of a run that is not anchored -- stays in the summary as its head.
template <class Sink>
__device__ __forceinline__ void seg_append(Seg &p, const Seg &s, uint32_t guard, Sink &sink) {
    if (s.n == 0) return;
    if (p.n == 0) {
        const uint32_t anchored = p.anchored;
        p = s;
        p.anchored = anchored;
        if (anchored) {
            sink.first(s.first);
            if (s.brk) sink.burst(s.first, s.head_last, s.head_w);
        }
        return;
    }
    const uint64_t g = s.first - p.last;
    sink.gap(p.last, s.first, g);
    const bool whole = p.brk || p.anchored;        // the first error of p's tail burst is known
    if (g > guard) {
        if (whole) sink.burst(p.tail_first, p.last, p.tail_w);
        else { p.head_last = p.last; p.head_w = p.n; }
        if (s.brk) sink.burst(s.first, s.head_last, s.head_w);
        p.tail_first = s.tail_first;               // !s.brk: s.first and s.n
        p.tail_w = s.tail_w;
        p.brk = 1;
    } else if (s.brk) {
        if (whole) sink.burst(p.tail_first, s.head_last, p.tail_w + s.head_w);
        else { p.head_last = s.head_last; p.head_w = p.n + s.head_w; }
        p.tail_first = s.tail_first;
        p.tail_w = s.tail_w;
        p.brk = 1;
    } else {
        p.tail_w += s.n;
    }
    p.n += s.n;
    p.last = s.last;
}

__device__ __forceinline__ uint32_t vbin32(uint32_t v) { return v < 256 ? v : 256u + (31u - (uint32_t)__clz(v)) - 8u; }

// the lane's two words of a step: words wi and wi + 1 of err & ~mask, zero beyond nwords, the last word cut at nbits
template <bool VEC, bool MASK>
__device__ __forceinline__ void load_pair(const uint64_t *err, const uint64_t *mask, uint64_t wi, uint64_t nwords, uint64_t last_keep,
                                          uint64_t &w0, uint64_t &w1) {
    w0 = 0;
    w1 = 0;
    if (wi + 1 < nwords) {
        if (VEC) {
            const ulonglong2 e = *reinterpret_cast<const ulonglong2 *>(err + wi);
            w0 = e.x;
            w1 = e.y;
            if (MASK) {
                const ulonglong2 m = *reinterpret_cast<const ulonglong2 *>(mask + wi);
                w0 &= ~m.x;
                w1 &= ~m.y;
            }
        } else {
            w0 = err[wi];
            w1 = err[wi + 1];
            if (MASK) {
                w0 &= ~mask[wi];
                w1 &= ~mask[wi + 1];
            }
        }
        if (wi + 2 == nwords) w1 &= last_keep;
    } else if (wi < nwords) {
        w0 = err[wi];
        if (MASK) w0 &= ~mask[wi];
        w0 &= last_keep;
    }
}

template <bool VEC, bool MASK>
__global__ __launch_bounds__(kTileThreads) void errstat_tile_kernel(const uint64_t *__restrict__ err, const uint64_t *__restrict__ mask,
                                                                     uint64_t nbits, ErrCfg cfg, bbb_errstat_result *res,
                                                                     Seg *__restrict__ segs) {
    __shared__ uint32_t hist[3 * kBins];
    __shared__ uint32_t sc[SC_N];
    __shared__ Seg wseg[kWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t i = tid; i < 3 * kBins; i += kTileThreads) hist[i] = 0;
    if (tid < SC_N) sc[tid] = 0;
    __syncthreads();

    const uint64_t nwords = (nbits + 63) >> 6;
    const uint64_t last_keep = (nbits & 63) ? (1ull << (nbits & 63)) - 1 : ~0ull;
    const uint64_t wbase = (uint64_t)blockIdx.x * kTileWords + (uint64_t)wave * kWaveWords;
    const uint64_t pos0 = res->bits + wbase * 64;  // the position of the wavefront's bit 0; below, positions are rel + 1, 0: none
    const uint32_t guard = cfg.guard;

    // the wavefront's state between steps (uniform)
    uint32_t c_cnt = 0, c_first = 0, c_last = 0;   // errors so far, the first and the last of them
    uint32_t c_fpos = 0, c_fcnt = 0;               // the latest burst start and the errors before it
    uint32_t c_headlast = 0, c_headw = 0;          // the burst closed by the first burst start: its first error is not ours to know
    // the lane's counters
    uint32_t maxgap = 0, nbursts = 0, blsum = 0, maxbl = 0, maxbw = 0, eb[4] = {0, 0, 0, 0};

    uint64_t w0, w1;
    load_pair<VEC, MASK>(err, mask, wbase + 2 * lane, nwords, last_keep, w0, w1);
    for (int s = 0; s < kSteps; ++s) {
        uint64_t n0 = 0, n1 = 0;
        if (s + 1 < kSteps) load_pair<VEC, MASK>(err, mask, wbase + (uint64_t)(s + 1) * kStepWords + 2 * lane, nwords, last_keep, n0, n1);
        const uint32_t c = (uint32_t)__popcll(w0) + (uint32_t)__popcll(w1);
        const uint64_t nz = __ballot(c != 0);
        if (nz) {
            const uint32_t lrel = (uint32_t)s * (kStepWords * 64) + lane * 128;
            uint32_t ls = 0, lf = 0;               // the lane's last and first error
            if (c) {
                ls = lrel + (w1 ? 64u + 63u - (uint32_t)__clzll(w1) : 63u - (uint32_t)__clzll(w0)) + 1;
                lf = lrel + (w0 ? (uint32_t)__builtin_ctzll(w0) : 64u + (uint32_t)__builtin_ctzll(w1)) + 1;
            }
            uint32_t inc = c;                      // errors up to and including the lane
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = __shfl_up(inc, d);
                if ((int)lane >= d) inc += t;
            }
            uint32_t k = c_cnt + inc - c;          // errors of the wavefront before the one at hand
            const uint64_t below = nz & ((1ull << lane) - 1);
            const uint32_t pl = __shfl(ls, below ? 63 - __clzll(below) : 0);
            uint32_t p = below ? pl : c_last;      // the error before the one at hand
            uint32_t fpos = 0, fcnt = 0;           // the lane's latest burst start and the errors before it
            uint32_t fs_p = 0, fs_cnt = 0;         // at the lane's first burst start: the error before it and the errors before
            if (c) {
                uint64_t w = w0;
                uint32_t off = lrel + 1;
                for (int half = 0; half < 2; ++half) {
                    while (w) {
                        const uint32_t t = off + (uint32_t)__builtin_ctzll(w);
                        w &= w - 1;
                        if (p) {
                            const uint32_t g = t - p;
                            atomicAdd(&hist[vbin32(g)], 1u);
                            maxgap = max(maxgap, g);
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (cfg.block[j] && blocks_differ(pos0 + p - 1, pos0 + t - 1, g, cfg.block[j])) ++eb[j];
                            if (g > guard) {       // a burst starts at t and closes the one that ends at p
                                if (fpos) {
                                    const uint32_t len = p - fpos + 1, wt = k - fcnt;
                                    atomicAdd(&hist[kBins + vbin32(len)], 1u);
                                    atomicAdd(&hist[2 * kBins + vbin32(wt)], 1u);
                                    ++nbursts;
                                    blsum += len;
                                    maxbl = max(maxbl, len);
                                    maxbw = max(maxbw, wt);
                                } else {
                                    fs_p = p;
                                    fs_cnt = k;
                                }
                                fpos = t;
                                fcnt = k;
                            }
                        }
                        p = t;
                        ++k;
                    }
                    w = w1;
                    off = lrel + 65;
                }
            }
            const uint64_t hm = __ballot(fpos != 0);
            if (hm) {
                // the burst a lane's first burst start closes began at the latest start below the lane
                const uint64_t hbelow = hm & ((1ull << lane) - 1);
                const int src = hbelow ? 63 - __clzll(hbelow) : 0;
                const uint32_t qpos = __shfl(fpos, src), qcnt = __shfl(fcnt, src);
                const uint32_t bpos = hbelow ? qpos : c_fpos, bcnt = hbelow ? qcnt : c_fcnt;
                if (fs_p && bpos) {
                    const uint32_t len = fs_p - bpos + 1, wt = fs_cnt - bcnt;
                    atomicAdd(&hist[kBins + vbin32(len)], 1u);
                    atomicAdd(&hist[2 * kBins + vbin32(wt)], 1u);
                    ++nbursts;
                    blsum += len;
                    maxbl = max(maxbl, len);
                    maxbw = max(maxbw, wt);
                }
                const int lo = __builtin_ctzll(hm), hi = 63 - __clzll(hm);
                const uint32_t hl = __shfl(fs_p, lo), hw = __shfl(fs_cnt, lo);
                if (!c_fpos) {                     // the wavefront's first burst start: the burst it closes is the head
                    c_headlast = hl;
                    c_headw = hw;
                }
                c_fpos = __shfl(fpos, hi);
                c_fcnt = __shfl(fcnt, hi);
            }
            const uint32_t f0 = __shfl(lf, __builtin_ctzll(nz));
            if (!c_first) c_first = f0;
            c_last = __shfl(ls, 63 - __clzll(nz));
            c_cnt += __shfl(inc, 63);
        }
        w0 = n0;
        w1 = n1;
    }

    if (maxgap) atomicMax(&sc[SC_MAXGAP], maxgap);
    if (nbursts) {
        atomicAdd(&sc[SC_BURSTS], nbursts);
        atomicAdd(&sc[SC_BLSUM], blsum);
        atomicMax(&sc[SC_MAXBL], maxbl);
        atomicMax(&sc[SC_MAXBW], maxbw);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (eb[j]) atomicAdd(&sc[SC_EB + j], eb[j]);
    if (lane == 0) {
        Seg s{};
        s.n = c_cnt;
        if (c_cnt) {
            s.first = pos0 + c_first - 1;
            s.last = pos0 + c_last - 1;
            s.tail_first = s.first;
            s.tail_w = c_cnt;
            if (c_fpos) {
                s.brk = 1;
                s.head_last = pos0 + c_headlast - 1;
                s.head_w = c_headw;
                s.tail_first = pos0 + c_fpos - 1;
                s.tail_w = c_cnt - c_fcnt;
            }
        }
        wseg[wave] = s;
    }
    __syncthreads();
    if (tid == 0) {
        Seg t{};
        LdsSink sink{hist, sc, cfg};
        for (int w = 0; w < kWaves; ++w) seg_append(t, wseg[w], guard, sink);
        segs[blockIdx.x] = t;
        wseg[0] = t;
    }
    __syncthreads();
    if (wseg[0].n == 0) return;                    // (uniform) nothing was counted
    for (uint32_t i = tid; i < 3 * kBins; i += kTileThreads) {
        const uint32_t v = hist[i];
        if (v) atomicAdd((unsigned long long *)&res->gap_hist[0] + i, (unsigned long long)v);   // the three histograms are adjacent
    }
    if (tid == 0) {
        atomicAdd((unsigned long long *)&res->errors, (unsigned long long)wseg[0].n);
        if (sc[SC_MAXGAP]) atomicMax((unsigned long long *)&res->max_gap, (unsigned long long)sc[SC_MAXGAP]);
        if (sc[SC_BURSTS]) {
            atomicAdd((unsigned long long *)&res->bursts, (unsigned long long)sc[SC_BURSTS]);
            atomicAdd((unsigned long long *)&res->burst_len_sum, (unsigned long long)sc[SC_BLSUM]);
            atomicMax((unsigned long long *)&res->max_burst_len, (unsigned long long)sc[SC_MAXBL]);
            atomicMax((unsigned long long *)&res->max_burst_weight, (unsigned long long)sc[SC_MAXBW]);
        }
        for (int j = 0; j < 4; ++j)
            if (sc[SC_EB + j]) atomicAdd((unsigned long long *)&res->errored_blocks[j], (unsigned long long)sc[SC_EB + j]);
    }
}

// the summaries [lo, hi) appended to p, four loads in flight
template <class Sink>
__device__ __forceinline__ void append_run(Seg &p, const Seg *__restrict__ segs, uint32_t lo, uint32_t hi, uint32_t guard, Sink &sink) {
    for (uint32_t i = lo; i < hi; i += 4) {
        Seg s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s[u].n = 0;
            if (i + u < hi) s[u] = segs[i + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) seg_append(p, s[u], guard, sink);
    }
}

__global__ __launch_bounds__(kStitchThreads) void errstat_stitch_kernel(const Seg *__restrict__ segs, uint32_t ntiles, uint64_t nbits,
                                                                         ErrCfg cfg, bbb_errstat_result *res) {
    constexpr int kGroup = 32, kGroups = kStitchThreads / kGroup;
    __shared__ Seg agg[kStitchThreads];
    __shared__ Seg grp[kGroups];
    const uint32_t tid = threadIdx.x, guard = cfg.guard;
    const uint32_t per = (ntiles + kStitchThreads - 1) / kStitchThreads;
    const uint32_t lo = min(tid * per, ntiles), hi = min(lo + per, ntiles);
    NoSink none;
    {
        Seg a{};
        append_run(a, segs, lo, hi, guard, none);
        agg[tid] = a;
    }
    __syncthreads();
    if (tid < kGroups) {
        Seg a{};
        for (int i = 0; i < kGroup; ++i) seg_append(a, agg[tid * kGroup + i], guard, none);
        grp[tid] = a;
    }
    __syncthreads();
    if (tid == 0) {
        Seg run{};                                 // the carried state: the open burst, anchored at the record's beginning
        run.anchored = 1;
        if (res->open_weight) {
            run.n = res->open_weight;
            run.first = run.tail_first = res->open_first;
            run.last = res->open_last;
            run.tail_w = res->open_weight;
        }
        for (int i = 0; i < kGroups; ++i) {
            const Seg t = grp[i];
            grp[i] = run;
            seg_append(run, t, guard, none);
        }
        if (run.n) {
            res->open_first = run.tail_first;
            res->open_last = run.last;
            res->last_error = run.last;
            res->open_weight = run.tail_w;
        }
        res->bits += nbits;
    }
    __syncthreads();
    if (tid < kGroups) {
        Seg run = grp[tid];
        for (int i = 0; i < kGroup; ++i) {
            const Seg t = agg[tid * kGroup + i];
            agg[tid * kGroup + i] = run;
            seg_append(run, t, guard, none);
        }
    }
    __syncthreads();
    Seg p = agg[tid];
    GlobalSink sink{res, cfg};
    append_run(p, segs, lo, hi, guard, sink);
}

__global__ void errstat_skip_kernel(bbb_errstat_result *res, uint64_t nbits) { res->bits += nbits; }

}  // namespace

size_t errstat_scratch_bytes() { return (size_t)(kErrLaunchBits / kErrTileBits) * sizeof(Seg); }

int errstat_launch(const ErrLaunch &a, bbb_errstat_result *res, void *scratch, hipStream_t st) {
    if (a.nbits == 0 || a.nbits > kErrLaunchBits) return fail(BBB_EINVAL, "errstat_launch: nbits out of range");
    ErrCfg cfg{};
    cfg.guard = a.guard;
    cfg.nblock = a.nblock;
    for (uint32_t j = 0; j < 4; ++j) cfg.block[j] = j < a.nblock ? a.block[j] : 0;
    const unsigned ntiles = (unsigned)((a.nbits + kErrTileBits - 1) / kErrTileBits);
    Seg *segs = static_cast<Seg *>(scratch);
    const dim3 grid(ntiles), block(kTileThreads);
    if (a.mask) {
        if (a.vec) errstat_tile_kernel<true, true><<<grid, block, 0, st>>>(a.err, a.mask, a.nbits, cfg, res, segs);
        else errstat_tile_kernel<false, true><<<grid, block, 0, st>>>(a.err, a.mask, a.nbits, cfg, res, segs);
    } else {
        if (a.vec) errstat_tile_kernel<true, false><<<grid, block, 0, st>>>(a.err, a.mask, a.nbits, cfg, res, segs);
        else errstat_tile_kernel<false, false><<<grid, block, 0, st>>>(a.err, a.mask, a.nbits, cfg, res, segs);
    }
    errstat_stitch_kernel<<<1, kStitchThreads, 0, st>>>(segs, ntiles, a.nbits, cfg, res);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

int errstat_skip_launch(bbb_errstat_result *res, uint64_t nbits, hipStream_t st) {
    errstat_skip_kernel<<<1, 1, 0, st>>>(res, nbits);
    BBB_HIP(hipGetLastError());
    return BBB_OK;
}

}  // namespace bbb
