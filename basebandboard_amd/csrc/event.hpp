// event.hpp -- the owning event of the host files (bbb_api.hip's scheduler, detector_api.hip's workspaces).  Host only.
#pragma once
#include "bbb_common.hpp"

#include <utility>

namespace bbb {

// An owned event; the destructor destroys it.  An ordering event (hipEventDisableTiming) is created by its first record, so
// a host-only handle creates none -- or ahead of it by create(), where the moment of creation matters; an event that
// bbb_lutopt_profile reads times between is created by create_timed().
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); return *this; }      // (o destroys the old one)
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    int create() { BBB_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); return BBB_OK; }
    int create_timed() { BBB_HIP(hipEventCreate(&e)); return BBB_OK; }
    int record(hipStream_t s) {
        if (!e) BBB_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        BBB_HIP(hipEventRecord(e, s));
        return BBB_OK;
    }
};

}  // namespace bbb
