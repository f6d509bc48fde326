// tests/sched_model/model.hpp -- see model.cpp
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

namespace model {

typedef std::vector<uint32_t> VC;                 // one component per stream
struct Access { VC vc; int stream = 0; std::string what; uint64_t seq = 0; };
struct Buffer {
    char *base = nullptr; size_t size = 0, maplen = 0; int id = 0; std::string tag = "?";
    bool freed = false, has_write = false;
    Access last_write;
    std::vector<Access> reads;                    // since the last write, the latest per stream
};

// an operation of the caller or of a kernel stub on stream s: it reads / writes the allocations these pointers lie in
void op(hipStream_t s, const std::string &what, std::initializer_list<const void *> reads, std::initializer_list<const void *> writes);
void host_note(const std::string &what);          // a line in the trace
void reset_trace();
void tag(const void *p, const std::string &t);    // a name for an allocation, for the reports
const std::vector<std::string> &errors();
void clear_errors();
uint64_t ops_checked();
uint64_t transcript();                            // the running hash over everything logged so far (model.cpp)
void fail_nth_launch(int nth);                    // the nth kernel-launch stub from now on returns BBB_EHIP, once (0: none does)
bool launch_failure_pending();                    // ... and has not done so yet
bool refused();                                   // a launch stub asks first: true means queue nothing and return BBB_EHIP
// what the next device-to-host copies deliver instead of zeros: one entry per copy, in order (a shorter entry: zeros behind it)
void deliver_next_d2h(const void *bytes, size_t n);
size_t deliveries_pending();
void clear_deliveries();                          // (a call that returned early left some unread)

// " (a, b, ...)": a launch stub's scalar arguments, appended to its operation text so that the transcript covers them
template <typename... T>
std::string args(T... v) {
    std::string s;
    ((s += (s.empty() ? " (" : ", ") + std::to_string(v)), ...);
    return s + ")";
}

}  // namespace model
