// Random sequences of bbb_prbs_detector_stream calls over the stream / event model of model.cpp, on two caller streams.
//   detector_driver <number of sequences> <seed> [max_bad]
//   detector_driver plan < lines of "k nbits chunk_bits warm_bits alignment ncu"
// Compiled with the REAL detector_api.hip: what is modelled is everything the call queues -- the pooled workspace and its
// reuse by a call with another layout on another stream, the zeroing a call leaves queued behind its read-back and the event
// the next call waits for, the first pass in its four forms, the verify pass, the repairs queued blind and after a look, the
// general repair loop and the serial continuation.  The launchers of detector_launch.hpp are stubs that record what the real
// kernels read and write and every scalar they are given (detector_kernels.hip is not compiled), pointers as offsets, so the
// transcript says what was queued, in which order, with which arguments, on which stream: a refactor of detector_api.hip must
// leave it as it was.  Refused calls and calls that fail at a launch are part of it.
// The model has no values, so the driver SCRIPTS what every read-back delivers (model::deliver_next_d2h) -- consistent at
// once, repaired by the first re-run, more bad chunks than the blind re-run takes, a second verify that still finds some,
// and more than 32 passes -- and holds the statistics that come back to what the script implies.
// `plan` prints what det_plan makes of a call's arguments, for tests/detector_geometry.py to be held against.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "detector_launch.hpp"
#include "model.hpp"

static std::vector<std::pair<const char *, size_t>> g_caller;
static std::string at(const void *p) {            // a pointer into a caller's buffer, by its offset
    if (!p) return "-";
    for (const auto &b : g_caller)
        if ((const char *)p >= b.first && (const char *)p < b.first + b.second) return std::to_string((const char *)p - b.first);
    return "?";
}
static uint64_t g_forms[4] = {0, 0, 0, 0};

namespace bbb {

std::string &last_error() {
    static thread_local std::string s;
    return s;
}

bool det_k_ok(int k) { return k == 7 || k == 9 || k == 11 || k == 15 || k == 20 || k == 23 || k == 31; }
bool det_sparse_ok(int k) { return k != 20; }

// the workspace's pointers as offsets from its first byte (spec: o_spec == 0)
static std::string ws_at(const DetLaunch &a, const void *p) { return p ? std::to_string((const char *)p - (const char *)a.spec) : "-"; }
static std::string call_args(const DetLaunch &a) {
    return model::args(a.nbits, a.nwords, a.chunk_words, a.warm_words, a.nchunks, a.tiles_ok) + " src " + at(a.src) + " err " + at(a.err) + " reload " +
           at(a.reload) + " endst " + ws_at(a, a.endst) + " counts " + ws_at(a, a.counts);
}

int det_first_pass_launch(int k, DetForm form, const DetLaunch &a, unsigned grid, unsigned cgrid, hipStream_t st) {
    if (model::refused()) return BBB_EHIP;
    g_forms[form]++;
    const std::string what = model::args(k, grid) + call_args(a);
    switch (form) {
    case kDetFused: model::op(st, "det_fused_kernel" + what, {a.src}, {a.spec, a.endst, a.counts, a.err, a.reload}); break;
    case kDetTwoKernels:
        model::op(st, "det_classify_kernel" + model::args(k, cgrid, a.nbits, a.nwords) + " flags " + ws_at(a, a.flags), {a.src}, {a.flags});
        model::op(st, "det_sparse_kernel" + what, {a.src, a.flags}, {a.spec, a.endst, a.counts, a.err, a.reload});
        break;
    case kDetDenseOut: model::op(st, "det_chunk_kernel<OUT> mode 0" + what, {a.src}, {a.spec, a.endst, a.counts, a.err, a.reload}); break;
    case kDetDenseTotals: model::op(st, "det_chunk_kernel<totals> mode 0" + what, {a.src}, {a.spec, a.endst, a.counts, a.err, a.reload}); break;
    }
    return BBB_OK;
}
int det_reduce_launch(const DetLaunch &a, unsigned rgrid, uint64_t *totals, unsigned *list, unsigned *nlist, const unsigned *skip_if_zero,
                      hipStream_t st) {
    if (model::refused()) return BBB_EHIP;
    model::op(st, "det_reduce_kernel" + model::args(rgrid, a.nchunks) + " totals " + ws_at(a, totals) + " list " + ws_at(a, list) + " nlist " +
                      ws_at(a, nlist) + " gate " + ws_at(a, skip_if_zero),
              {a.counts, a.spec, a.endst, skip_if_zero}, {totals, list, nlist});
    return BBB_OK;
}
int det_rerun_launch(int k, const DetLaunch &a, unsigned grid, const unsigned *list, unsigned nlist, const unsigned *nlist_dev, hipStream_t st) {
    if (model::refused()) return BBB_EHIP;
    model::op(st, "det_chunk_kernel<OUT> mode 1" + model::args(k, grid, nlist) + call_args(a) + " list " + ws_at(a, list) + " count " + ws_at(a, nlist_dev),
              {list, nlist_dev, a.src, a.spec, a.endst, a.counts}, {a.spec, a.endst, a.counts, a.err, a.reload});
    return BBB_OK;
}
int det_serial_launch(int k, const DetLaunch &a, uint64_t c0, hipStream_t st) {
    if (model::refused()) return BBB_EHIP;
    model::op(st, "det_serial_kernel" + model::args(k, c0) + call_args(a), {a.src, a.spec, a.endst}, {a.spec, a.endst, a.counts, a.err, a.reload});
    return BBB_OK;
}

}  // namespace bbb

using namespace bbb;

static const char *form_name(const DetPlan &p) { return p.sparse ? (p.fused ? "fused" : "two-kernel") : (p.tiles_ok ? "dense-tiled" : "dense-lane"); }

static int plan_mode() {
    long long k, nbits, cb, wb, al, ncu;
    while (std::cin >> k >> nbits >> cb >> wb >> al >> ncu) {
        DetPlan p;
        const int rc = det_plan((int)k, (const void *)(uintptr_t)(4096 + al), (uint64_t)nbits, (uint64_t)cb, (uint64_t)wb, (int)ncu, &p);
        if (rc) std::printf("{\"k\": %lld, \"nbits\": %lld, \"chunk_bits\": %lld, \"warm_bits\": %lld, \"alignment\": %lld, \"ncu\": %lld, \"refused\": \"%s\"}\n",
                            k, nbits, cb, wb, al, ncu, last_error().c_str());
        else std::printf("{\"k\": %lld, \"nbits\": %lld, \"chunk_bits\": %lld, \"warm_bits\": %lld, \"alignment\": %lld, \"ncu\": %lld, \"form\": \"%s\", "
                         "\"chunk_words\": %llu}\n", k, nbits, cb, wb, al, ncu, form_name(p), (unsigned long long)p.chunk_words);
    }
    return 0;
}

struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t s) : g(s) {}
    uint64_t below(uint64_t n) { return n ? g() % n : 0; }
    bool chance(int pct) { return (int)below(100) < pct; }
};

enum Outcome { kConsistentSparse, kConsistentDense, kRepairedSparse, kRepairedDense, kManyBad, kSecondVerifyBad, kSerial, kOutcomes };
static const char *const kOutcomeNames[kOutcomes] = {"consistent_sparse", "consistent_dense", "repaired_sparse", "repaired_dense", "many_bad",
                                                     "second_verify_bad", "serial"};

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "plan") return plan_mode();
    if (argc < 3) { std::fprintf(stderr, "usage: detector_driver <nseq> <seed> [max_bad] | plan\n"); return 2; }
    const long nseq = std::atol(argv[1]);
    Rng rng((uint64_t)std::atoll(argv[2]));
    const long max_bad = argc > 3 ? std::atol(argv[3]) : 1000000;

    hipStream_t user[2];
    hipStreamCreateWithFlags(&user[0], 0);
    hipStreamCreateWithFlags(&user[1], 0);
    std::vector<void *> all;
    auto alloc = [&](size_t bytes, const std::string &tag) {
        void *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { std::fprintf(stderr, "no address space for %s\n", tag.c_str()); std::exit(2); }
        model::tag(p, tag);
        g_caller.emplace_back((const char *)p, bytes);
        all.push_back(p);
        return (uint64_t *)p;
    };
    // each caller stream owns its input and its outputs: 1e10 bits and a word of slack
    const size_t kBytes = (size_t)10000000000ull / 8 + 4096;
    uint64_t *src[2], *err[2], *reload[2];
    for (int i = 0; i < 2; i++) {
        const std::string sfx = i ? " (stream 1)" : " (stream 0)";
        src[i] = alloc(kBytes, "caller: packed stream" + sfx);
        err[i] = alloc(kBytes, "caller: err" + sfx);
        reload[i] = alloc(kBytes, "caller: reload" + sfx);
    }

    const int ks[7] = {7, 9, 11, 15, 20, 23, 31};
    // (chunk words, warm bits): fused, two kernels (chunk no multiple of 128, too long, warm-up too long), no tiles
    const uint64_t geo[][2] = {{128, 1024}, {256, 1024}, {640, 1024}, {1024, 64}, {128, 8192}, {64, 1024}, {192, 1024}, {2048, 1024},
                               {512, 16384}, {64, 64}, {24, 1024}, {1, 64}, {16, 1000}};
    const int ngeo = (int)(sizeof geo / sizeof geo[0]);

    long bad_sequences = 0;
    uint64_t calls = 0, refused = 0, failed = 0, other_layout = 0, outcomes[kOutcomes] = {};
    for (long seq = 0; seq < nseq; seq++) {
        hipDeviceSynchronize();
        model::reset_trace();
        model::host_note("sequence " + std::to_string(seq));
        const int ncalls = 3 + (int)rng.below(8);
        uint64_t last_tail = ~0ull;
        int last_stream = -1;
        for (int c = 0; c < ncalls; c++, calls++) {
            const int sx = (int)rng.below(2);
            hipStream_t ux = user[sx];
            const int k = ks[rng.below(7)];
            uint64_t chunk_bits = 0, warm_bits = 0, nbits;
            if (rng.chance(70)) {
                const int g = (int)rng.below((uint64_t)ngeo);
                chunk_bits = geo[g][0] * 64; warm_bits = rng.chance(20) ? 0 : geo[g][1];
                switch (rng.below(4)) {             // one word ... several thousand chunks
                case 0: nbits = 1 + rng.below(64 * 3); break;
                case 1: nbits = 1 + rng.below(chunk_bits * 70); break;
                case 2: nbits = chunk_bits * (300 + rng.below(400)) + rng.below(64); break;
                default: nbits = chunk_bits * (4200 + rng.below(5000)) - rng.below(64); break;
                }
                if (geo[g][0] == 1 && rng.chance(30)) nbits = 64 * (4000000 + rng.below(100000));     // a workspace above 256 MiB: not kept
            } else {                                // the default geometry: 64 words, 128 words (fused), the CU rule (fused)
                const uint64_t lens[6] = {300001, 2000000, 1000000000ull, 2120000000ull, 8590000000ull, 10000000000ull};
                nbits = lens[rng.below(6)] - rng.below(1000);
            }
            if (rng.chance(3)) nbits = 0;
            const uint64_t shift = rng.chance(15) ? 1 : 0;                  // an input 8 bytes off a 16-byte boundary: the dense pass
            const bool want_err = rng.chance(60), want_reload = rng.chance(60), want_stats = rng.chance(85);
            const uint64_t *s = src[sx] + shift;
            uint64_t *e = want_err ? err[sx] + rng.below(2) : nullptr, *r = want_reload ? reload[sx] + rng.below(2) : nullptr;
            bbb_detector_stats stats{};
            model::op(ux, "CALLER writes the stream; the previous reader of the outputs", {}, {src[sx], err[sx], reload[sx]});
            model::host_note("call k " + std::to_string(k) + " nbits " + std::to_string(nbits) + " chunk " + std::to_string(chunk_bits) + " warm " +
                             std::to_string(warm_bits) + " stream " + std::to_string(sx));

            if (rng.chance(6)) {                    // refused for its geometry: nothing is queued, no slot is taken
                const bool many = rng.chance(50);
                const int rc = many ? prbs_detector_stream_launch(k, s, ((0x7fffffffull + 1 + rng.below(1000)) * 64), e, r, &stats, 64, 0, ux)
                                    : prbs_detector_stream_launch(k, s, nbits, e, r, &stats, 64 * (1 + rng.below(100)) + 1 + rng.below(63), warm_bits, ux);
                if (rc == BBB_OK) { std::fprintf(stderr, "a call with a bad geometry was not refused\n"); return 2; }
                model::host_note("refused -> " + std::to_string(rc) + " " + last_error());
                refused++;
                continue;
            }

            DetPlan p;
            if (det_plan(k, s, nbits, chunk_bits, warm_bits, 256, &p)) { std::fprintf(stderr, "det_plan refused: %s\n", last_error().c_str()); return 2; }
            // ---- the script: what the read-backs deliver, and the statistics that implies
            uint64_t tot[4], exp_rerun = 0, exp_serial = 0;
            for (uint64_t &t : tot) t = rng.below(1ull << 40);
            auto garbage16 = [&](uint64_t (&w)[16]) { for (uint64_t &x : w) x = rng.below(1ull << 40); };
            Outcome oc = p.sparse ? kConsistentSparse : kConsistentDense;
            if (nbits) {
                const uint64_t maxbad = p.nchunks - 1;           // chunk 0 is never inconsistent
                int want = (int)rng.below(10);                   // 0-4 consistent, 5-6 repaired, 7 many, 8 second verify, 9 serial
                if (want == 7 && maxbad < 4097) want = 5;
                if (want >= 5 && maxbad < 1) want = 0;
                uint64_t first[16], second[16];
                garbage16(first); garbage16(second);
                uint64_t passes = 0;
                bool loop = false;
                if (want < 5) {
                    for (int i = 0; i < 4; i++) first[i] = tot[i];
                    first[4] = 0;
                    model::deliver_next_d2h(first, sizeof first);
                } else {
                    const uint64_t nb1 = want == 7 ? 4097 + rng.below(maxbad - 4096) : 1 + rng.below(std::min<uint64_t>(4096, maxbad));
                    const bool again = want >= 8 || (want == 7 && rng.chance(50));       // the verify behind the re-run still finds some
                    uint64_t (&look)[16] = p.sparse ? second : first;                    // where the second verify's result is read
                    first[4] = nb1 | (rng.below(1000) << 32);                            // (the high half is not the count)
                    for (int i = 0; i < 4; i++) look[8 + i] = tot[i];
                    look[12] = again ? 1 + rng.below(nb1) : 0;
                    model::deliver_next_d2h(first, sizeof first);
                    if (p.sparse) model::deliver_next_d2h(second, sizeof second);
                    exp_rerun = std::min<uint64_t>(nb1, 4096);
                    passes = 1;
                    loop = nb1 > 4096 || again;
                    oc = want == 7 ? kManyBad : want == 8 ? kSecondVerifyBad : want == 9 ? kSerial : p.sparse ? kRepairedSparse : kRepairedDense;
                }
                if (loop) {
                    // the general loop: verify, look, re-run; more than 32 passes in a row: the serial continuation, then anew
                    uint64_t more = want == 9 ? 33 + rng.below(3) : rng.below(4);
                    for (;;) {
                        uint64_t h[5];
                        for (uint64_t &x : h) x = rng.below(1ull << 40);
                        const uint64_t nbad = more ? 1 + rng.below(std::min<uint64_t>(maxbad, 300)) : 0;
                        h[4] = nbad | (rng.below(1000) << 32);
                        if (!nbad) for (int i = 0; i < 4; i++) h[i] = tot[i];
                        model::deliver_next_d2h(h, sizeof h);
                        if (!nbad) break;
                        more--;
                        if (++passes > 32) {
                            std::vector<unsigned> bad(nbad);
                            for (unsigned &x : bad) x = 1 + (unsigned)rng.below(maxbad);
                            model::deliver_next_d2h(bad.data(), bad.size() * sizeof(unsigned));
                            exp_serial = 1; passes = 0; exp_rerun += 1;
                            continue;
                        }
                        exp_rerun += nbad;
                    }
                }
            }
            const int nth = rng.chance(20) ? 1 + (int)rng.below(5) : 0;       // a launch that fails: the call returns early
            model::fail_nth_launch(nth);
            const int rc = prbs_detector_stream_launch(k, s, nbits, e, r, want_stats ? &stats : nullptr, chunk_bits, warm_bits, ux);
            const bool launch_failed = nth && !model::launch_failure_pending();
            model::fail_nth_launch(0);
            if (launch_failed) {
                if (rc != BBB_EHIP) { std::fprintf(stderr, "a failing launch gave %d\n", rc); return 2; }
                model::clear_deliveries();
                model::host_note("failed at launch " + std::to_string(nth) + " -> " + std::to_string(rc));
                failed++;
            } else {
                if (rc != BBB_OK) { std::fprintf(stderr, "call failed: %d %s\n", rc, last_error().c_str()); return 2; }
                if (model::deliveries_pending()) { std::fprintf(stderr, "%zu scripted read-backs were not read (%s)\n", model::deliveries_pending(), kOutcomeNames[oc]); return 2; }
                if (nbits) {
                    outcomes[oc]++;
                    if (last_tail != ~0ull && last_tail != p.o_tail && last_stream != sx) other_layout++;
                    last_tail = p.o_tail; last_stream = sx;
                }
                if (want_stats) {
                    const bbb_detector_stats &t = stats;
                    const bool ok = nbits ? t.bits == nbits && t.errors == tot[0] && t.errors_raw == tot[1] && t.reload_clocks == tot[2] && t.resyncs == tot[3] &&
                                                t.chunks == p.nchunks && t.chunks_rerun == exp_rerun && t.serial_fallback == exp_serial
                                          : t.bits == 0 && t.chunks == 0 && t.chunks_rerun == 0;
                    if (!ok) {
                        std::fprintf(stderr, "sequence %ld call %d (%s): the statistics are not what the read-backs imply: chunks %llu (%llu) rerun %llu (%llu) "
                                             "serial %llu (%llu) errors %llu (%llu)\n", seq, c, kOutcomeNames[oc], (unsigned long long)t.chunks,
                                     (unsigned long long)p.nchunks, (unsigned long long)t.chunks_rerun, (unsigned long long)exp_rerun,
                                     (unsigned long long)t.serial_fallback, (unsigned long long)exp_serial, (unsigned long long)t.errors, (unsigned long long)tot[0]);
                        return 2;
                    }
                }
            }
            model::op(ux, "CALLER reads the outputs", {err[sx], reload[sx]}, {});
            if (!model::errors().empty()) break;
        }
        if (!model::errors().empty()) {
            bad_sequences++;
            if (bad_sequences <= 3)
                for (const std::string &e : model::errors()) std::fprintf(stderr, "sequence %ld: UNORDERED ACCESS\n  %s\n", seq, e.c_str());
            model::clear_errors();
            if (bad_sequences >= max_bad) break;
        }
    }
    hipDeviceSynchronize();
    for (void *p : all) hipFree(p);
    std::printf("{\"sequences\": %ld, \"calls\": %llu, \"refused\": %llu, \"failed_launches\": %llu, \"other_layout_other_stream\": %llu, "
                "\"forms\": {\"fused\": %llu, \"two-kernel\": %llu, \"dense-out\": %llu, \"dense-totals\": %llu}, \"outcomes\": {",
                nseq, (unsigned long long)calls, (unsigned long long)refused, (unsigned long long)failed, (unsigned long long)other_layout,
                (unsigned long long)g_forms[kDetFused], (unsigned long long)g_forms[kDetTwoKernels], (unsigned long long)g_forms[kDetDenseOut],
                (unsigned long long)g_forms[kDetDenseTotals]);
    for (int i = 0; i < kOutcomes; i++) std::printf("%s\"%s\": %llu", i ? ", " : "", kOutcomeNames[i], (unsigned long long)outcomes[i]);
    std::printf("}, \"operations_checked\": %llu, \"sequences_with_unordered_access\": %ld, \"transcript\": \"%016llx\"}\n",
                (unsigned long long)model::ops_checked(), bad_sequences, (unsigned long long)model::transcript());
    return bad_sequences ? 1 : 0;
}
