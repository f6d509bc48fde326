// detector_api.hip -- the host scheduler of bbb_prbs_detector_stream (the kernels and what they compute: detector_kernels.hip).
// Host logic only: the geometry of a call, the workspace pool, and the stages a call queues through detector_launch.hpp.
#include "detector_launch.hpp"
#include "dev_buf.hpp"
#include "event.hpp"

#include <deque>
#include <mutex>
#include <string>
#include <vector>

namespace bbb {

typedef unsigned long long u64;

int det_plan(int k, const void *src, uint64_t nbits, uint64_t chunk_bits, uint64_t warm_bits, int ncu, DetPlan *p) {
    if (chunk_bits == 0) {
        // about four waves of lanes per SIMD, but chunks of 4096 ... 32768 bits: the warm-up before every chunk is
        // 1024 bits of extra work, and short inputs should still fill the device.  (Sizing the chunks so that they fill
        // whole generations of resident lanes -- 2 x 38912-bit chunks per lane slot at 1e10 bits instead of 2.33 x 32768 --
        // changed nothing measurable: 0.455-0.46 ms either way.)
        const uint64_t want = (nbits / 262144 + 127) / 128 * 128;
        chunk_bits = want < 4096 ? 4096 : (want > 32768 ? 32768 : want);
        if (want > 32768) {
            // Long streams (round 5; profiles/r05_det_chunk_sweep.log): the fused kernel takes chunks of 512 ... 1024 words, a block
            // four waves x 64 chunks, and all blocks are resident at once -- the kernel then takes as long as the CU with the MOST
            // blocks, so the chunk length is chosen for the smallest (blocks on the fullest CU) x (words per chunk); ties go to the
            // longer chunk (fewer chunk records, fewer speculative starts).  1e10 bits: 640 words (954 blocks on 256 CUs: 4 x 640)
            // where round 4's fixed 512 gave 1192 blocks (5 x 512): 0.277 -> 0.258 ms per call.
            const uint64_t nwords = (nbits + 63) / 64;
            uint64_t best_cost = ~0ull, best_cw = 512;
            for (uint64_t cw = 512; cw <= (uint64_t)kDetFusedMaxChunkWords; cw += 128) {
                const uint64_t nblocks = ((nwords + cw - 1) / cw + 255) / 256;
                const uint64_t cost = ((nblocks + (uint64_t)ncu - 1) / (uint64_t)ncu) * cw;
                if (cost <= best_cost) { best_cost = cost; best_cw = cw; }
            }
            chunk_bits = best_cw * 64;
        }
    }
    if (warm_bits == 0) warm_bits = 1024;
    if (chunk_bits % 64) return fail(BBB_EINVAL, "chunk_bits must be a multiple of 64");
    const u64 nwords = (nbits + 63) / 64;
    const u64 chunk_words = chunk_bits / 64, warm_words = (warm_bits + 63) / 64;
    const u64 nchunks = (nwords + chunk_words - 1) / chunk_words;
    if (nchunks > 0x7fffffffull) return fail(BBB_EINVAL, "too many chunks; raise chunk_bits");
    // one workspace: spec | endst | counts | list | nlist + totals | flags
    const bool kSparse = det_sparse_ok(k);
    const size_t o_spec = 0, o_end = o_spec + nchunks * kDetStateBytes, o_cnt = o_end + nchunks * kDetStateBytes,
                 o_list = o_cnt + nchunks * kDetCountBytes, o_tail = (o_list + 2 * nchunks * sizeof(unsigned) + 7) & ~(size_t)7,
                 o_flags = (o_tail + 16 * sizeof(u64) + 15) & ~(size_t)15, total = o_flags + (kSparse ? ((nwords + 255) / 256) * 4 * sizeof(u64) : 0);
    const unsigned grid = (unsigned)((nchunks + 255) / 256);
    // (the reduce kernel's time is its atomics -- one per block and counter: 512 blocks 11 us, 128 blocks 6 us, 64 too few to
    // stream 20 MB of chunk records; BBB_DET_RGRID: A/B timing, -DBBB_EXPERIMENTS only)
    const unsigned rmax = (unsigned)env_knob("BBB_DET_RGRID", 128);
    const unsigned rgrid = grid < rmax ? grid : rmax;
    // cooperative 128-byte loads need chunks and warm-up in whole 16-word rows on 16-byte aligned data
    const int tiles_ok = chunk_words % 16 == 0 && warm_words % 16 == 0 && warm_words > 0 && ((uintptr_t)src & 15) == 0;
    static const bool dense = env_knob("BBB_DET_DENSE", 0) != 0;          // (A/B timing of the two forms; -DBBB_EXPERIMENTS only)
    const bool sparse = kSparse && !dense && ((uintptr_t)src & 15) == 0;
    const u64 nblk = (nwords + 255) / 256;                        // one wave per 256 words, four waves per block
    const unsigned cgrid = (unsigned)((nblk + 3) / 4 < 8192 ? (nblk + 3) / 4 : 8192);
    static const bool two_kernels = env_knob("BBB_DET_TWO_KERNELS", 0) != 0;      // (A/B timing; -DBBB_EXPERIMENTS only)
    bool fused = false;
    if (chunk_words % 128 == 0 && chunk_words <= (u64)kDetFusedMaxChunkWords && warm_words <= 128 && !two_kernels) fused = sparse;
    *p = DetPlan{nwords, chunk_words, warm_words, nchunks, tiles_ok, sparse, fused, grid, rgrid, cgrid,
                 o_spec, o_end, o_cnt, o_list, o_tail, o_flags, total};
    return BBB_OK;
}

namespace {

// The call's device workspace and its pinned read-back buffer, kept between calls (grow-only, one per concurrent call and
// device).  With a stream-ordered allocation per call the pool gave the 22 MB of a 1e10-bit call back to the driver at every
// synchronisation and fetched them again at the next call, and the totals came back through a pageable bounce buffer: 0.26 ms
// of host time around 0.49 ms of kernels.
// zeroed_at / ev_zero: the 16 tail words at that offset of d are zero once ev_zero has happened -- a call that ends the plain way
// zeroes them for the next one BEHIND its read-back instead of the next call doing so in front of its first kernel
struct DetWorkspace {
    int dev = 0;
    bool busy = false;
    DevBuf<char> d;
    DevBuf<uint64_t, true> h;                     // 16 words: both tails
    Event ev_copy, ev_zero;
    size_t zeroed_at = 0;
    bool zeroed = false;
};
std::mutex g_det_ws_mu;
// (a deque: a slot a call holds stays where it is while another thread appends.  Never destroyed: no HIP call at process exit)
std::deque<DetWorkspace> &g_det_ws = *new std::deque<DetWorkspace>;

// The slot a call holds.  However the call ends, the destructor synchronises the call's stream and hands the slot back; the
// one exit with nothing but the tail's zeroing in flight hands it back itself, without the synchronisation.
struct DetLease {
    DetWorkspace *w = nullptr;
    hipStream_t st = nullptr;
    bool tail_zeroed = false;                     // the previous user left the tail at this call's offset zeroed (behind ev_zero)
    DetLease() = default;
    DetLease(const DetLease &) = delete;
    DetLease &operator=(const DetLease &) = delete;
    ~DetLease() { end(false, 0); }

    int acquire(size_t need, size_t o_tail, hipStream_t s) {
        int dev = 0;
        BBB_HIP(hipGetDevice(&dev));
        bool zero_pending;
        {
            std::lock_guard<std::mutex> g(g_det_ws_mu);
            DetWorkspace *f = nullptr;
            for (DetWorkspace &x : g_det_ws)
                if (!x.busy && x.dev == dev) { f = &x; break; }
            if (!f) {
                DetWorkspace n;
                n.dev = dev;
                int rc;
                if ((rc = n.h.grow(16)) || (rc = n.ev_copy.create()) || (rc = n.ev_zero.create())) return rc;
                g_det_ws.push_back(std::move(n));
                f = &g_det_ws.back();
            }
            if (f->d.cap < need) {
                f->zeroed = false;
                if (const int rc = f->d.grow(need)) return rc;
            }
            f->busy = true;
            w = f;
            st = s;
            tail_zeroed = f->zeroed && f->zeroed_at == o_tail;
            zero_pending = f->zeroed;
            f->zeroed = false;                    // (until this call has ended the way that leaves them zeroed again)
        }
        // The previous user of this workspace left a 128-byte memset queued behind its read-back (ev_zero) and handed the workspace back
        // without waiting for it.  A call with ANOTHER layout (other nbits or chunking: the old tail lies inside this call's chunk
        // records), on another stream, must not start before that memset has run -- round 4's advisor: a late memset zeroing 16 words
        // of the new call's records.  Whoever finds the flag set waits for the event first (same stream: nothing to wait for).
        if (zero_pending) (void)hipStreamWaitEvent(st, w->ev_zero, 0);
        return BBB_OK;
    }
    // the tail at o_tail is zeroed behind ev_zero and nothing else of the call is in flight: no synchronisation
    void hand_back_zeroed(size_t o_tail) { end(true, o_tail); }

private:
    void end(bool leave_zeroed, size_t o_tail) {
        if (!w) return;
        if (!leave_zeroed) (void)hipStreamSynchronize(st);
        std::lock_guard<std::mutex> g(g_det_ws_mu);
        if (leave_zeroed) { w->zeroed = true; w->zeroed_at = o_tail; }
        if (w->d.cap > (size_t)256 << 20) {       // (a very long stream's workspace is not kept: 256 MiB = 1.2e11 bits at the default chunking)
            w->d = DevBuf<char>();
            w->zeroed = false;
        }
        w->busy = false;
        w = nullptr;
    }
};

struct DetResult { uint64_t h[5] = {0, 0, 0, 0, 0}; uint64_t rerun = 0; bool serial = false; };     // h: the four totals, the bad chunks

// everything a call queues and waits for; r when BBB_OK
int det_run(int k, const DetPlan &p, const uint64_t *src, uint64_t nbits, uint64_t *err, uint64_t *reload, hipStream_t st, DetLease &lease,
            DetResult &r) {
    int rc;
    if ((rc = lease.acquire(p.total, p.o_tail, st))) return rc;
    char *const ws = lease.w->d;
    uint64_t *const hh = lease.w->h;
    const DetLaunch a{src, nbits, p.nwords, p.chunk_words, p.warm_words, p.nchunks, (DetState *)(ws + p.o_spec), (DetState *)(ws + p.o_end),
                      (DetCount *)(ws + p.o_cnt), (uint64_t *)(ws + p.o_flags), err, reload, p.tiles_ok};
    unsigned *list = (unsigned *)(ws + p.o_list), *list2 = list + p.nchunks;
    uint64_t *tail = (uint64_t *)(ws + p.o_tail), *tail2 = tail + 8;       // tail[0..3] totals, low half of tail[4] = number of bad chunks
    unsigned *nlist = (unsigned *)(tail + 4), *nlist2 = (unsigned *)(tail2 + 4);
    // the first n listed chunks (n_dev: at most that many, the count read on the device) again from their predecessors' ends,
    // then verify + totals into tail2 -- which returns at once when the device's count is zero
    auto repair = [&](unsigned n, const unsigned *n_dev) {
        if (const int rc2 = det_rerun_launch(k, a, (n + 255) / 256, list, n, n_dev, st)) return rc2;
        return det_reduce_launch(a, p.rgrid, tail2, list2, nlist2, n_dev, st);
    };
    if (p.sparse) {                               // (outputs are written for the words the machine visits)
        if (err) (void)hipMemsetAsync(err, 0, p.nwords * sizeof(u64), st);
        if (reload) (void)hipMemsetAsync(reload, 0, p.nwords * sizeof(u64), st);
    }
    const DetForm form = p.sparse ? (p.fused ? kDetFused : kDetTwoKernels) : (err || reload) ? kDetDenseOut : kDetDenseTotals;
    if ((rc = det_first_pass_launch(k, form, a, p.grid, p.cgrid, st))) return rc;
    uint64_t passes = 0;
    if (env_knob("BBB_DET_ONE_TRIP", 1)) {
        // ONE round trip for the two common outcomes: the chain is consistent as speculated, or it is after the few
        // inconsistent chunks have been run again from their predecessors' end states.  Verify + totals (pass 1), a re-run
        // of at most kSpec listed chunks whose count the device reads itself, verify + totals again (pass 2, which returns
        // at once when pass 1 found nothing) -- all queued before the host looks.
        constexpr unsigned kSpec = 4096;
        if (!lease.tail_zeroed) (void)hipMemsetAsync(tail, 0, 16 * sizeof(u64), st);      // (else: zeroed behind the previous call's read-back; waited for above)
        if ((rc = det_reduce_launch(a, p.rgrid, tail, list, nlist, nullptr, st))) return rc;
        // The repair stages are queued blind only for the dense pass, whose reset-state speculation leaves a few dozen
        // inconsistent chunks on every noisy stream.  The sparse pass starts a chunk from the clean state its flags imply and
        // is consistent as speculated unless an error or a reload sits right on a chunk boundary: there the two idle launches
        // (10 us of a 0.3 ms call) cost more than the second round trip they save, so the host looks first.
        if (!p.sparse && (rc = repair(kSpec, nlist))) return rc;
        hipError_t e = hipMemcpyAsync(hh, tail, 16 * sizeof(u64), hipMemcpyDeviceToHost, st);
        // The host waits for the read-back only; the zeroing of the tail words for the NEXT call is queued behind it and runs
        // while the host returns (5 us of a 0.29 ms call that were in front of the first kernel)
        bool zero_queued = false;
        if (e == hipSuccess && p.sparse) {
            e = hipEventRecord(lease.w->ev_copy, st);
            if (e == hipSuccess) e = hipMemsetAsync(tail, 0, 16 * sizeof(u64), st);
            if (e == hipSuccess) e = hipEventRecord(lease.w->ev_zero, st);
            zero_queued = e == hipSuccess;
            if (e == hipSuccess) e = hipEventSynchronize(lease.w->ev_copy);
        } else if (e == hipSuccess) e = hipStreamSynchronize(st);
        BBB_HIP(e);
        const unsigned nbad1 = (unsigned)(hh[4] & 0xffffffffull), nb = nbad1 < kSpec ? nbad1 : kSpec;
        if (!nbad1) {
            for (int i = 0; i < 5; i++) r.h[i] = hh[i];
            // (nothing of this call but that memset is in flight: the workspace goes back without a stream synchronisation)
            if (zero_queued) lease.hand_back_zeroed(p.o_tail);
            return BBB_OK;
        }
        if (p.sparse) {
            // second trip: the listed chunks again from their predecessors' ends, verify + totals, look again
            if ((rc = repair(nb, nullptr))) return rc;
            e = hipMemcpyAsync(hh, tail, 16 * sizeof(u64), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            BBB_HIP(e);
        }
        r.rerun += nb;
        passes = 1;
        if (nbad1 <= kSpec && !(unsigned)(hh[12] & 0xffffffffull)) {
            for (int i = 0; i < 5; i++) r.h[i] = hh[8 + i];
            return BBB_OK;
        }
    }
    for (;;) {
        // verify, and reduce at once in the hope that the chain is already consistent: one round trip
        (void)hipMemsetAsync(tail, 0, 5 * sizeof(u64), st);
        if ((rc = det_reduce_launch(a, p.rgrid, tail, list, nlist, nullptr, st))) return rc;
        hipError_t e = hipMemcpyAsync(r.h, tail, sizeof r.h, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        BBB_HIP(e);
        const unsigned nbad = (unsigned)(r.h[4] & 0xffffffffull);
        if (!nbad) return BBB_OK;
        passes++;
        if (passes > 32) {
            // the speculation does not settle on this stream: continue serially from the first bad chunk
            std::vector<unsigned> hb(nbad);
            e = hipMemcpy(hb.data(), list, nbad * sizeof(unsigned), hipMemcpyDeviceToHost);
            BBB_HIP(e);
            unsigned c0 = hb[0];
            for (unsigned x : hb) c0 = x < c0 ? x : c0;
            if ((rc = det_serial_launch(k, a, c0, st))) return rc;
            r.serial = true;
            passes = 0;                     // the serial kernel stops where the chain is consistent again: verify anew
            r.rerun += 1;
            continue;
        }
        r.rerun += nbad;
        if ((rc = det_rerun_launch(k, a, (nbad + 255) / 256, list, nbad, nullptr, st))) return rc;
    }
}

}  // namespace

int prbs_detector_stream_launch(int k, const uint64_t *src, uint64_t nbits, uint64_t *err, uint64_t *reload,
                                bbb_detector_stats *stats, uint64_t chunk_bits, uint64_t warm_bits, hipStream_t st) {
    if (!det_k_ok(k)) return fail(BBB_EINVAL, "k=" + std::to_string(k) + " invalid for PRBS");
    int dev = 0, ncu = 256;
    if (chunk_bits == 0 && nbits / 262144 > 32768)      // (the calls whose plan looks at the CU count: the default rule's `want` above 32768)
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1) ncu = 256;
    DetPlan p;
    int rc = det_plan(k, src, nbits, chunk_bits, warm_bits, ncu, &p);
    if (rc) return rc;
    if (nbits == 0) {
        if (stats) *stats = bbb_detector_stats{};
        return BBB_OK;
    }
    DetResult r;
    {
        DetLease lease;                           // (handed back, the stream synchronised, before the call's error is asked for)
        rc = det_run(k, p, src, nbits, err, reload, st, lease, r);
    }
    if (rc) return rc;
    BBB_HIP(hipGetLastError());
    if (stats) {
        stats->bits = nbits;
        stats->errors = r.h[0];
        stats->errors_raw = r.h[1];
        stats->reload_clocks = r.h[2];
        stats->resyncs = r.h[3];
        stats->chunks = p.nchunks;
        stats->chunks_rerun = r.rerun;
        stats->serial_fallback = r.serial ? 1 : 0;
    }
    return BBB_OK;
}

}  // namespace bbb
