// capture.hpp -- what the host files of the capture side share, the calls that take samples or packed bits the caller already
// holds: the device and stream of an object that owns both (bbb_errstat, bbb_nco, bbb_sinc_eye), the stream-ordered slab
// that one call owns, and the front end of the FIR-shaped calls (bbb_fir_*, bbb_ddc_run).  Host only: no kernel file includes
// it, and everything here is compiled unchanged against a model of HIP (tests/sched_model/capture_driver.cpp).
#pragma once
#include "bbb_common.hpp"
#include "dev_buf.hpp"

namespace bbb {

// Declared LAST in its object, as TxChunks is: destroyed first, it selects the device for the frees of the DevBufs declared
// before it (which go in reverse order of declaration).
struct StreamObj {
    int device = -1;
    hipStream_t st = nullptr;
    ~StreamObj() { if (device >= 0) (void)hipSetDevice(device); }

    // what is queued on the new stream from here on comes behind everything the object queued on the old one
    int rebind(hipStream_t s) {
        if (s == st) return BBB_OK;
        BBB_HIP(hipSetDevice(device));
        hipEvent_t ev;
        BBB_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        hipError_t e = hipEventRecord(ev, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, ev, 0);
        (void)hipEventDestroy(ev);
        if (e != hipSuccess) return fail(BBB_EHIP, std::string("ordering the new stream: ") + hipGetErrorString(e));
        st = s;
        return BBB_OK;
    }
    // before the object goes: its buffers may still be in use by queued launches
    void drain() const {
        if (device >= 0) (void)hipSetDevice(device);
        (void)hipStreamSynchronize(st);
    }
};

// A stream-ordered allocation of `count` T that one call owns: from `pool`, or from the device's default pool, on the
// call's stream, and released on that stream when the call returns -- behind the kernels the call queued.
template <typename T>
struct CallScratch {
    T *p = nullptr;
    hipStream_t st = nullptr;
    CallScratch() = default;
    CallScratch(const CallScratch &) = delete;
    CallScratch &operator=(const CallScratch &) = delete;
    ~CallScratch() { if (p) (void)hipFreeAsync(p, st); }
    operator T *() const { return p; }
    int alloc(size_t count, hipStream_t stream, hipMemPool_t pool = nullptr) {
        st = stream;
        if (pool) BBB_HIP(hipMallocFromPoolAsync((void **)&p, count * sizeof(T), pool, st));
        else BBB_HIP(hipMallocAsync((void **)&p, count * sizeof(T), st));
        return BBB_OK;
    }
};

inline int device_cus(int device, int *cus) {
    BBB_HIP(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device));
    return BBB_OK;
}

// ---- the FIR-shaped calls: nin inputs behind up to ntaps - 1 samples of history, one output per decim inputs ------------
constexpr uint64_t kFirSampleLimit = 1ull << 58;

// two byte ranges share a byte (an empty range shares none)
inline bool overlap(const void *a, uint64_t abytes, const void *b, uint64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return abytes && bbytes && a0 < b0 + bbytes && b0 < a0 + abytes;
}

inline uint64_t fir_nout(const bbb_fir_cfg *cfg, uint64_t nin) { return cfg->phase < nin ? (nin - cfg->phase + cfg->decim - 1) / cfg->decim : 0; }

// *before: the history the launch reads, nbefore clamped to what the taps reach.  Refuses an output (`out_name`, out_bytes of
// it: 0 when there is none) that overlaps the samples and that history.
inline int fir_history(const int16_t *in, uint64_t nin, uint32_t nbefore, uint32_t ntaps, const void *out, uint64_t out_bytes,
                       const char *out_name, uint32_t *before) {
    *before = std::min<uint32_t>(nbefore, ntaps - 1);
    if (out_bytes && overlap(in - *before, (nin + *before) * 2, out, out_bytes))
        return fail(BBB_EINVAL, std::string(out_name) + " overlaps the samples");
    return BBB_OK;
}

}  // namespace bbb
