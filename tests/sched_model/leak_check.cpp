// What the scheduler holds when a call returns EARLY.  With profiling on (bbb_lutopt_profile) a timed fill creates three timing
// events in front of its start states and every mover two around its kernel; until they are queued for bbb_lutopt_profile_read
// they belong to the call, and a call that fails in between -- the seeding, the sample kernel, the data bits or the mover refused
// by the runtime -- has to give them back.  The model's launches never fail, so the random sequences of driver.cpp cannot see
// this; here model::fail_nth_launch makes each launch of three calls fail in turn:
//   a staged fill, an unstaged fill of the specialised kernel, a staged transmitter fill,
// each on a fresh handle, which is destroyed afterwards.  The program is built with AddressSanitizer: an event (a MockEvent of
// model.cpp) that nobody destroyed is reported by its leak check when the process ends.  Test infrastructure only.
//   leak_check <taps file>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/bbb.h"
#include "model.hpp"

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: leak_check <taps>\n"); return 2; }
    std::vector<uint16_t> taps;
    std::vector<uint32_t> off;
    {
        std::ifstream f(argv[1]);
        std::string line;
        while (std::getline(f, line)) {
            if (line.empty()) continue;
            off.push_back((uint32_t)taps.size());
            std::istringstream is(line);
            int v;
            while (is >> v) taps.push_back((uint16_t)v);
        }
        off.push_back((uint32_t)taps.size());
    }
    const int k = (int)off.size() - 1;
    if (k != 256) { std::fprintf(stderr, "expected the n256 tap list\n"); return 2; }

    hipStream_t user;
    hipStreamCreateWithFlags(&user, 0);
    void *dst8 = nullptr, *dst16 = nullptr;
    const uint64_t n = 1ull << 24;                  // (the smallest request that takes the staged form)
    hipMalloc(&dst8, n);
    hipMalloc(&dst16, 2 * n);
    bbb_tx_cfg tx{};
    for (int i = 0; i < 64; i++) tx.coeffs[i] = (int16_t)(i - 32);
    tx.source = 0; tx.prbs_k = 31; tx.prbs_state = 1; tx.bit_en = 1; tx.noise_en = 1; tx.noise_var = 8; tx.warmup = 16;
    const uint64_t init[8] = {1, 0, 0, 0, 0, 0, 0, 0};

    // {name, staging level, launches the call makes: two of seeding, (the data bits,) the sample kernel, (the mover)}
    struct Case { const char *name; int staged; int launches; } cases[3] = {
        {"staged fill", 1, 4}, {"unstaged specialised fill", 0, 3}, {"staged transmitter fill", 1, 5}};
    for (int ci = 0; ci < 3; ci++) {
        const Case &c = cases[ci];
        for (int nth = 1; nth <= c.launches + 1; nth++) {
            bbb_lutopt *h = nullptr;
            if (bbb_lutopt_create(&h, k, taps.data(), off.data(), init, 0) != BBB_OK || bbb_lutopt_set_stream(h, (void *)user) != BBB_OK ||
                bbb_lutopt_set_staged(h, c.staged) != BBB_OK || bbb_lutopt_profile(h, 1) != BBB_OK) {
                std::printf("FAIL: %s: no handle (%s)\n", c.name, bbb_last_error_detail());
                return 1;
            }
            model::fail_nth_launch(nth);
            const int rc = ci == 2 ? bbb_tx_fill_i16(h, &tx, (int16_t *)dst16, n, 4096) : bbb_awgn_fill_i8(h, (int8_t *)dst8, n, 4096);
            const bool failed = !model::launch_failure_pending();
            model::fail_nth_launch(0);
            // launch 1 .. launches fails and the call says so; one past the last finds nothing to fail: the count is right
            if (failed != (nth <= c.launches) || rc != (failed ? BBB_EHIP : BBB_OK)) {
                std::printf("FAIL: %s, launch %d of %d: returned %d, the launch %s\n", c.name, nth, c.launches, rc, failed ? "failed" : "did not fail");
                return 1;
            }
            if (bbb_lutopt_destroy(h) != BBB_OK) { std::printf("FAIL: %s: destroy\n", c.name); return 1; }
        }
    }
    hipFree(dst8);
    hipFree(dst16);
    if (!model::errors().empty()) { std::printf("FAIL: the model reported: %s\n", model::errors()[0].c_str()); return 1; }
    std::printf("ok no event outlives its call\n");
    return 0;
}
