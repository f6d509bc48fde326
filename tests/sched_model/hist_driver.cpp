// Random call sequences that mix bbb_awgn_hist with fills, announcements, staging levels, the noise stream object and a re-bound
// caller stream, over the stream / event model of model.cpp.
//   hist_driver <taps file> <number of sequences> <seed> [max_bad]
// Compiled with the REAL bbb_api.hip and the REAL hist_api.hip: what is modelled is the path bbb_awgn_hist takes through the
// scheduler -- lutopt_stage_visit (the staged sample kernel of a chunk with the histogram mover as the reader of its slot), the
// level it sets for the call and gives back, its announcements, its chunk buffer and partials with their stream-ordered
// release.  The histogram kernels are stubs that record what the real ones read and write (hist_kernels.hip is not compiled).
// The driver plays the caller as driver.cpp does: it writes the counters on its stream before a call and reads them after.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "bbb_common.hpp"
#include "model.hpp"

namespace bbb {
int hist_grid_blocks() { return 256; }
int hist_planes_launch(const void *stage, uint64_t nsamples, unsigned L, unsigned nlanes, uint32_t *scratch, int blocks, unsigned *used, hipStream_t st) {
    model::op(st, "hist_planes_kernel" + model::args(nsamples, L, nlanes, blocks), {stage}, {scratch});
    *used = 1;
    return BBB_OK;
}
int hist_samples_launch(const void *samples, int elem, uint64_t nsamples, unsigned nbins, uint32_t *scratch, int blocks, unsigned *used, hipStream_t st) {
    model::op(st, "hist_samples_kernel" + model::args(elem, nsamples, nbins, blocks), {samples}, {scratch});
    *used = 1;
    return BBB_OK;
}
int hist_reduce_launch(const uint32_t *scratch, unsigned used, unsigned nbins, uint64_t *hist, hipStream_t st) {
    model::op(st, "hist_reduce_kernel" + model::args(used, nbins), {scratch, hist}, {hist});
    return BBB_OK;
}
}  // namespace bbb

#define CK(call)                                                                                                       \
    do {                                                                                                               \
        const int rc_ = (call);                                                                                        \
        if (rc_ != BBB_OK) { std::fprintf(stderr, "%s failed: %s (%s)\n", #call, bbb_strerror(rc_), bbb_last_error_detail()); std::exit(2); } \
    } while (0)

struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t s) : g(s) {}
    uint64_t below(uint64_t n) { return n ? g() % n : 0; }
    bool chance(int pct) { return (int)below(100) < pct; }
};

int main(int argc, char **argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: hist_driver <taps> <nseq> <seed> [max_bad]\n"); return 2; }
    const long max_bad = argc > 4 ? std::atol(argv[4]) : 1000000;
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
    const long nseq = std::atol(argv[2]);
    Rng rng((uint64_t)std::atoll(argv[3]));

    hipStream_t user[2];
    hipStreamCreateWithFlags(&user[0], 0);
    hipStreamCreateWithFlags(&user[1], 0);
    hipEvent_t uev;
    hipEventCreate(&uev);
    const uint64_t kMax = 3ull << 24;
    void *sets[2][2] = {};                       // per caller stream (driver.cpp): int8 samples, histogram counters
    for (int i = 0; i < 2; i++) {
        const std::string sfx = i ? " (stream 1)" : " (stream 0)";
        hipMalloc(&sets[i][0], kMax + 64); model::tag(sets[i][0], "caller: int8 samples" + sfx);
        hipMalloc(&sets[i][1], 256 * 8); model::tag(sets[i][1], "caller: histogram counters" + sfx);
    }
    void *dst8 = sets[0][0], *hist = sets[0][1];
    auto use_set = [&](int i) { dst8 = sets[i][0]; hist = sets[i][1]; };

    const uint64_t sizes[4] = {1ull << 24, (1ull << 24) + 4096, 1ull << 25, 3ull << 24};
    // histogram ranges: through memory only; one staged chunk; a staged chunk and a rest through memory; two staged chunks of
    // 2^30 and of 2^24 + ..., the second announced, and a rest
    const uint64_t hsizes[6] = {4099, 1ull << 24, (1ull << 24) + 4099, 3ull << 24, (1ull << 30) + (1ull << 24), (1ull << 30) + (1ull << 25) + 77};

    uint64_t init[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    bbb_lutopt *h = nullptr;
    int cur = 0;
    auto fresh_handle = [&]() {
        if (h) CK(bbb_lutopt_destroy(h));
        CK(bbb_lutopt_create(&h, k, taps.data(), off.data(), init, 0));
        cur = 0;
        use_set(0);
        CK(bbb_lutopt_set_stream(h, (void *)user[0]));
    };
    fresh_handle();

    long bad_sequences = 0;
    uint64_t calls = 0, hists = 0;
    for (long seq = 0; seq < nseq; seq++) {
        if (seq % 400 == 399) fresh_handle();
        hipDeviceSynchronize();
        model::reset_trace();
        model::host_note("sequence " + std::to_string(seq));
        bbb_awgn_stream *ns = nullptr;
        uint64_t pos = 16 + rng.below(1000) * 16;
        uint64_t n = sizes[rng.below(4)];
        const int ncalls = 8 + (int)rng.below(25);
        for (int c = 0; c < ncalls; c++, calls++) {
            hipStream_t us = user[cur];
            const int what = (int)rng.below(10);
            switch (what) {
            case 0: case 1: case 2: {  // a histogram: at the reader's position or elsewhere
                const uint64_t nn = hsizes[rng.below(6)];
                const uint64_t first = rng.chance(60) ? pos : 16 + rng.below(1u << 30) * 16;
                model::op(us, "CALLER writes the counters (zeroes them, or a previous consumer)", {}, {hist});
                model::host_note("bbb_awgn_hist n " + std::to_string(nn) + " first " + std::to_string(first));
                CK(bbb_awgn_hist(h, (uint64_t *)hist, nn, first));
                model::op(us, "CALLER reads the counters", {hist}, {});
                pos = first + nn;
                hists++;
                break;
            }
            case 3: case 4: {          // a fill: through the open stream object, or plain
                model::op(us, "CALLER writes dst (previous consumer)", {}, {dst8});
                if (ns) {
                    model::host_note("bbb_awgn_stream_next");
                    CK(bbb_awgn_stream_next(ns, dst8));
                } else {
                    const uint64_t first = rng.chance(75) ? pos : 16 + rng.below(1u << 30) * 16;
                    const uint64_t nn = rng.chance(80) ? n : 16 * (1 + rng.below(1000));
                    model::host_note("bbb_awgn_fill_i8 n " + std::to_string(nn) + " first " + std::to_string(first));
                    CK(bbb_awgn_fill_i8(h, (int8_t *)dst8, nn, first));
                    pos = first + nn;
                }
                model::op(us, "CALLER reads dst", {dst8}, {});
                break;
            }
            case 5: {                  // an announcement, for a fill that may never come (a histogram may come instead)
                if (ns) break;
                const uint64_t first = rng.chance(65) ? pos : 16 + rng.below(1u << 30) * 16;
                model::host_note("bbb_awgn_prefetch n " + std::to_string(n) + " first " + std::to_string(first));
                CK(bbb_awgn_prefetch(h, n, first));
                break;
            }
            case 6: {                  // staging level
                if (ns) break;
                const int lv[5] = {0, 1, 2, 2, 4};
                const int l = lv[rng.below(5)];
                model::host_note("bbb_lutopt_set_staged " + std::to_string(l));
                CK(bbb_lutopt_set_staged(h, l));
                break;
            }
            case 7: {                  // noise stream object: open / close (histograms between its reads are allowed)
                if (!ns) { n = sizes[rng.below(4)]; model::host_note("bbb_awgn_stream_open"); CK(bbb_awgn_stream_open(h, n, pos, 1, &ns)); }
                else { uint64_t t = 0; CK(bbb_awgn_stream_tell(ns, &t)); pos = t; model::host_note("bbb_awgn_stream_close"); CK(bbb_awgn_stream_close(ns)); ns = nullptr; }
                break;
            }
            case 8: {                  // the caller re-binds the handle to its other stream, ordering its streams or not
                if (ns) break;
                const bool ordered = rng.chance(50);
                if (ordered) hipEventRecord(uev, user[cur]);
                cur ^= 1;
                if (ordered) hipStreamWaitEvent(user[cur], uev, 0);
                use_set(cur);
                model::host_note(std::string("bbb_lutopt_set_stream -> user stream ") + std::to_string(cur) + (ordered ? " (ordered)" : " (NOT ordered)"));
                CK(bbb_lutopt_set_stream(h, (void *)user[cur]));
                break;
            }
            case 9: hipStreamSynchronize(us); break;
            default: break;
            }
            if (!model::errors().empty()) break;
        }
        if (ns) CK(bbb_awgn_stream_close(ns));
        if (!model::errors().empty()) {
            bad_sequences++;
            if (bad_sequences <= 3)
                for (const std::string &e : model::errors()) std::fprintf(stderr, "sequence %ld: UNORDERED ACCESS\n  %s\n", seq, e.c_str());
            model::clear_errors();
            if (bad_sequences >= max_bad) break;
            fresh_handle();
        }
    }
    if (h) CK(bbb_lutopt_destroy(h));
    hipEventDestroy(uev);
    for (auto &st : sets) for (void *p : st) hipFree(p);
    std::printf("{\"sequences\": %ld, \"calls\": %llu, \"histograms\": %llu, \"operations_checked\": %llu, \"sequences_with_unordered_access\": %ld, "
                "\"transcript\": \"%016llx\"}\n",
                nseq, (unsigned long long)calls, (unsigned long long)hists, (unsigned long long)model::ops_checked(), bad_sequences,
                (unsigned long long)model::transcript());
    return bad_sequences ? 1 : 0;
}
