// dev_buf.hpp -- the owning device buffer of the host files (bbb_api.hip's scheduler, the transmitter-driven analysers of
// tx_chunks.hpp, and through capture.hpp the capture side's objects: bbb_errstat, bbb_nco, bbb_sinc_eye).  Host only: no
// kernel file includes it.
#pragma once
#include "bbb_common.hpp"

#include <utility>

namespace bbb {

// A device buffer of T (Pinned: page-locked host memory) that grows to exactly the size asked for: the old buffer is freed
// first, nothing is allocated ahead.  hipFree waits for the device, so a grow is a host synchronisation.  Move-only; the
// destructor frees it.
template <typename T, bool Pinned = false>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }   // (o frees the old one)
    ~DevBuf() { if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p)); }
    operator T *() const { return p; }
    int grow(size_t need) {
        if (cap >= need) return BBB_OK;
        if (p) BBB_HIP(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
        BBB_HIP(Pinned ? hipHostMalloc((void **)&p, need * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, need * sizeof(T)));
        cap = need;
        return BBB_OK;
    }
};

}  // namespace bbb
