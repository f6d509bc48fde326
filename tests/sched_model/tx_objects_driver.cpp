// Random call sequences over the five objects that walk the transmitter's waveform chunk by chunk -- bbb_tx_eye,
// bbb_tx_ber_sweep, bbb_tx_acf, bbb_link_sweep, bbb_tx_xcorr -- mixed with plain fills, over the stream / event model of model.cpp.
//   tx_objects_driver <taps file> <number of sequences> <seed> [max_bad]
// Compiled with the REAL bbb_api.hip and the REAL eye_api.hip, txsweep_api.hip, acf_api.hip, link_api.hip, xcorr_api.hip (and
// fir_api.hip, for the link's filter checks): what is modelled is everything these objects queue -- their buffers, the fills
// and announcements of every chunk, the chunk's data bits, the launches.  The objects' kernels are stubs that record what the
// real ones read and write and every scalar they are given (the *_kernels.hip files are not compiled), so the transcript says
// what was queued, in which order, with which arguments, on which stream: a refactor of the host files must leave it as it was.
// The driver uses include/bbb.h and the launch signatures of bbb_common.hpp only.  It plays the caller as driver.cpp does: it
// writes the counters on its stream before a call and reads them after.
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

static std::string taps_hash(const uint32_t *w, size_t n) {       // (a launch's tap words, folded into one argument)
    uint64_t x = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) x = (x ^ w[i]) * 1099511628211ull;
    return " taps " + std::to_string(x);
}

int eye_grid_blocks(uint64_t nsamples) { return (int)std::min<uint64_t>(256, (nsamples + 2047) / 2048); }
int eye_accumulate_launch(const EyeLaunch &a, const int16_t *samples, uint64_t nsamples, uint64_t first_sample, uint32_t *scratch, int blocks,
                          uint64_t *hist, uint64_t *bathtub, hipStream_t st) {
    const std::string what = "eye_kernel" + model::args(a.ncols, a.shift, a.col_origin, a.threshold, a.strict, a.bits != nullptr, a.bit0, a.nbits,
                                                        a.pulser, a.want_hist, a.want_tub, nsamples, first_sample, blocks);
    model::op(st, what, {samples, a.nbits ? a.bits : nullptr}, {scratch});
    model::op(st, "eye_reduce", {scratch, hist, bathtub}, {hist, bathtub});
    return BBB_OK;
}

AcfPlan acf_plan(uint32_t nlags, uint64_t max_nfirst) {
    AcfPlan p{};
    p.gx = (int)std::min<uint64_t>(64, (max_nfirst + 4095) / 4096);
    p.gy = (int)((nlags + 63) / 64);
    p.smem = 1024;
    p.partial_words = (uint64_t)p.gx * p.gy * 65;
    p.scratch_words = p.partial_words + 64;
    return p;
}
int acf_launch(const AcfPlan &p, const int16_t *samples, uint64_t nfirst, uint64_t navail, uint32_t nlags, uint64_t *scratch, uint64_t *acf,
               hipStream_t st) {
    model::op(st, "acf_kernel" + model::args(p.gx, p.gy, p.smem, p.scratch_words, nfirst, navail, nlags), {samples, scratch, acf}, {scratch, acf});
    return BBB_OK;
}

XcorrPlan xcorr_plan(uint32_t spb, uint32_t nlags, uint64_t max_nsamples) {
    XcorrPlan p{};
    p.gx = (int)std::min<uint64_t>(64, (max_nsamples + 4095) / 4096);
    p.xt = 8;
    p.lw = p.xt * spb;
    p.gy = (int)((nlags + p.lw - 1) / p.lw);
    p.scratch_words = (uint64_t)p.gx * p.gy * p.lw;
    return p;
}
int xcorr_launch(const XcorrPlan &p, const XcorrLaunch &l, uint64_t *scratch, int64_t *xc, hipStream_t st) {
    const std::string what = "xcorr_kernel" + model::args(p.gx, p.gy, p.xt, p.lw, p.scratch_words, l.nsamples, l.first_sample, l.bit0, l.nbits, l.spb,
                                                          l.nlags, l.origin);
    model::op(st, what, {l.samples, l.bits, scratch, xc}, {scratch, xc});
    return BBB_OK;
}
int xcorr_pulser_bits_launch(uint64_t *dst, uint64_t first_bit, uint64_t nwords, hipStream_t st) {
    model::op(st, "xcorr_pulser_bits_kernel" + model::args(first_bit, nwords), {}, {dst});
    return BBB_OK;
}

int sweep_grid_blocks(uint64_t n) { return (int)std::min<uint64_t>(256, (n + 2047) / 2048); }
int sweep_tables_launch(const int16_t *coeffs_dev, int ntab, uint16_t *tables, hipStream_t st) {
    model::op(st, "sweep_tables_kernel" + model::args(ntab), {coeffs_dev}, {tables});
    return BBB_OK;
}
int sweep_launch(const SweepGroup &g, const uint16_t *tables, const SweepChunk &c, uint32_t *scratch, int blocks, uint64_t *counters, hipStream_t st) {
    std::string what = "sweep_kernel" + model::args(g.table, g.pairs, g.thr, c.noise != nullptr, c.bits != nullptr, c.m0, c.navail, c.source, c.first,
                                                    c.n, blocks);
    for (int k = 0; k < kSweepMaxPairs; k++) what += model::args(g.nv2[k], g.t0[k], g.t1[k], g.idx[2 * k], g.idx[2 * k + 1]);
    model::op(st, what, {tables, c.noise, c.navail ? c.bits : nullptr}, {scratch});
    model::op(st, "sweep_reduce", {scratch, counters}, {counters});
    return BBB_OK;
}

int link_grid_blocks(bool hist) { return hist ? 128 : 256; }
int link_launch(const LinkLaunch &a, bool hist, uint64_t first, uint64_t n, uint32_t *scratch, int blocks, uint64_t *hist_out, uint64_t *counters,
                hipStream_t st) {
    const std::string what = "link_kernel" + model::args(a.noise != nullptr, a.norg, a.nnoise, a.bits != nullptr, a.m0, a.nwords, a.source, a.nv, a.tb,
                                                         a.out_lo, a.out_hi, a.delay, a.ngroups, a.shift, a.threshold, a.strict, a.ncols,
                                                         a.eye_shift, a.col_origin, hist, first, n, blocks) + taps_hash(a.taps, BBB_FIR_MAX_TAPS / 2);
    model::op(st, what, {a.noise, a.bits, a.table}, {scratch});
    model::op(st, "link_reduce", {scratch, hist_out, counters}, {hist_out, counters});
    return BBB_OK;
}

int fir_launch(const FirLaunch &, int, int, hipStream_t) { return BBB_OK; }       // (fir_api.hip's own entry points are not driven)

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
    if (argc < 4) { std::fprintf(stderr, "usage: tx_objects_driver <taps> <nseq> <seed> [max_bad]\n"); return 2; }
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

    hipStream_t user;
    hipStreamCreateWithFlags(&user, 0);
    const uint64_t kMax = 3ull << 24;
    const int kMaxSet = 40;
    void *dst8, *dst16, *hist, *tub, *acf, *xc, *counters, *lhist;
    hipMalloc(&dst8, kMax + 64); model::tag(dst8, "caller: int8 samples");
    hipMalloc(&dst16, 2 * (kMax + 64)); model::tag(dst16, "caller: int16 samples");
    hipMalloc(&hist, 256 * 64 * 8); model::tag(hist, "caller: eye histogram");
    hipMalloc(&tub, 16 * 8); model::tag(tub, "caller: bathtub");
    hipMalloc(&acf, (BBB_ACF_MAX_LAGS + 1) * 8); model::tag(acf, "caller: acf counters");
    hipMalloc(&xc, 512 * 8); model::tag(xc, "caller: xcorr counters");
    hipMalloc(&counters, kMaxSet * 16 * 8); model::tag(counters, "caller: sweep counters");
    hipMalloc(&lhist, (size_t)kMaxSet * 256 * 64 * 8); model::tag(lhist, "caller: link histograms");
    void *const all[] = {dst8, dst16, hist, tub, acf, xc, counters, lhist};

    // small chunks, where a range of a few chunks stays cheap to log, and one at which the fills take the staged path
    const uint64_t chunks[4] = {4096 + 8, 5000, 65536, (1ull << 24) + 4096};

    uint64_t init[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    bbb_lutopt *h = nullptr;
    auto fresh_handle = [&]() {
        if (h) CK(bbb_lutopt_destroy(h));
        CK(bbb_lutopt_create(&h, k, taps.data(), off.data(), init, 0));
        CK(bbb_lutopt_set_stream(h, (void *)user));
    };
    fresh_handle();

    long bad_sequences = 0;
    uint64_t calls = 0, runs = 0;
    for (long seq = 0; seq < nseq; seq++) {
        if (seq % 100 == 99) fresh_handle();
        hipDeviceSynchronize();
        model::reset_trace();
        model::host_note("sequence " + std::to_string(seq));

        // the sequence's transmitter: noise on or off, PRBS or Pulser
        bbb_tx_cfg tx{};
        for (int i = 0; i < 64; i++) tx.coeffs[i] = (int16_t)((int)rng.below(511) - 255);
        tx.source = (int)rng.below(2); tx.prbs_k = 31; tx.prbs_state = 1 + rng.below(1000); tx.bit_en = rng.chance(90);
        tx.noise_en = rng.chance(60); tx.noise_var = (int)rng.below(16); tx.warmup = 16 * rng.below(4);
        const uint64_t chunk = chunks[rng.below(4)];
        // the sweeps' settings: a few coefficient sets shared among them, bits and noise on or off, thresholds zero and not
        const int nset = 1 + (int)rng.below(rng.chance(20) ? kMaxSet : 6);
        std::vector<bbb_tx_setting> sets(nset);
        const int ncoef = 1 + (int)rng.below(3);
        for (int i = 0; i < nset; i++) {
            bbb_tx_setting &s = sets[i];
            const int which = (int)rng.below(ncoef);
            for (int j = 0; j < 64; j++) s.coeffs[j] = (int16_t)((j * (which + 1)) % 200 - 100);
            s.bit_en = rng.chance(85); s.noise_en = tx.noise_en && rng.chance(80); s.noise_var = (int)rng.below(16);
            s.threshold = rng.chance(50) ? 0 : (int)rng.below(200) - 100; s.strict = (int)rng.below(2); s.reserved = 0;
        }
        bbb_fir_cfg fir{};
        fir.ntaps = 1 + (uint32_t)rng.below(40);
        for (uint32_t i = 0; i < fir.ntaps; i++) fir.taps[i] = (int16_t)((int)rng.below(21) - 10);
        fir.shift = (uint32_t)rng.below(8); fir.decim = 1; fir.phase = 0; fir.out_bytes = 2;
        const uint32_t delay = (uint32_t)rng.below(rng.chance(50) ? 20 : 256);
        bbb_eye_cfg eye{};
        const uint32_t cols[4] = {8, 16, 32, 64};
        eye.ncols = cols[rng.below(4)]; eye.shift = (uint32_t)rng.below(16); eye.col_origin = BBB_TX_BIT_SAMPLE0; eye.threshold = 0; eye.strict = 0;
        const bool link_eye = rng.chance(50);
        const uint32_t acf_lags = 1 + (uint32_t)rng.below(BBB_ACF_MAX_LAGS), xc_lags = 1 + (uint32_t)rng.below(512);

        bbb_tx_eye *oe = nullptr; bbb_tx_ber_sweep *os = nullptr; bbb_tx_acf *oa = nullptr; bbb_link_sweep *ol = nullptr; bbb_tx_xcorr *ox = nullptr;
        model::host_note("open: chunk " + std::to_string(chunk) + " nset " + std::to_string(nset));
        CK(bbb_tx_eye_open(h, &tx, &eye, chunk, &oe));
        CK(bbb_tx_ber_sweep_open(h, &tx, sets.data(), nset, chunk, &os));
        CK(bbb_tx_acf_open(h, &tx, acf_lags, chunk, &oa));
        CK(bbb_link_sweep_open(h, &tx, sets.data(), nset, &fir, delay, link_eye ? &eye : nullptr, chunk, &ol));
        CK(bbb_tx_xcorr_open(h, &tx, xc_lags, chunk, &ox));

        uint64_t pos = 0;                                // where a "sequential reader" is: the first run starts at sample 0
        const int ncalls = 6 + (int)rng.below(10);
        for (int c = 0; c < ncalls; c++, calls++) {
            // a range of 1, 2 or at least 3 chunks, the last one ragged, at the reader's position or elsewhere
            const uint64_t nch = 1 + rng.below(4);
            const uint64_t n = nch == 1 ? 1 + rng.below(chunk) : (nch - 1) * chunk + 1 + rng.below(chunk - 1);
            const uint64_t first = rng.chance(60) ? pos : rng.below(1u << 20) + (rng.chance(30) ? (1ull << 40) : 0);
            const std::string range = " first " + std::to_string(first) + " n " + std::to_string(n);
            const int what = (int)rng.below(8);
            switch (what) {
            case 0: {
                const bool wh = rng.chance(70), wt = !wh || rng.chance(70);
                model::op(user, "CALLER writes the eye's outputs", {}, {hist, tub});
                model::host_note("bbb_tx_eye_run" + range);
                CK(bbb_tx_eye_run(oe, first, n, wh ? (uint64_t *)hist : nullptr, wt ? (uint64_t *)tub : nullptr));
                model::op(user, "CALLER reads the eye's outputs", {hist, tub}, {});
                break;
            }
            case 1:
                model::op(user, "CALLER writes the sweep counters", {}, {counters});
                model::host_note("bbb_tx_ber_sweep_run" + range);
                CK(bbb_tx_ber_sweep_run(os, first, n, (uint64_t *)counters));
                model::op(user, "CALLER reads the sweep counters", {counters}, {});
                break;
            case 2:
                model::op(user, "CALLER writes the acf counters", {}, {acf});
                model::host_note("bbb_tx_acf_run" + range);
                CK(bbb_tx_acf_run(oa, first, n, (int64_t *)acf));
                model::op(user, "CALLER reads the acf counters", {acf}, {});
                break;
            case 3: {
                const bool wc = !link_eye || rng.chance(70);
                model::op(user, "CALLER writes the link's outputs", {}, {counters, lhist});
                model::host_note("bbb_link_sweep_run" + range);
                CK(bbb_link_sweep_run(ol, first, n, wc ? (uint64_t *)counters : nullptr, (uint64_t *)lhist));
                model::op(user, "CALLER reads the link's outputs", {counters, lhist}, {});
                break;
            }
            case 4:
                model::op(user, "CALLER writes the xcorr counters", {}, {xc});
                model::host_note("bbb_tx_xcorr_run" + range);
                CK(bbb_tx_xcorr_run(ox, first, n, (int64_t *)xc));
                model::op(user, "CALLER reads the xcorr counters", {xc}, {});
                break;
            case 5: {                  // a plain waveform fill between the objects' runs
                const uint64_t nn = rng.chance(50) ? 1ull << 24 : 8 * (1 + rng.below(1u << 16));
                model::op(user, "CALLER writes dst16 (previous consumer)", {}, {dst16});
                model::host_note("bbb_tx_fill_i16 n " + std::to_string(nn) + " first " + std::to_string(first));
                CK(bbb_tx_fill_i16(h, &tx, (int16_t *)dst16, nn, first));
                model::op(user, "CALLER reads dst16", {dst16}, {});
                break;
            }
            case 6: {                  // a plain noise fill, and now and then an announcement nobody takes
                const uint64_t nn = rng.chance(50) ? 1ull << 24 : 16 * (1 + rng.below(1u << 15));
                const uint64_t f16 = 16 + (first & ~15ull);
                model::op(user, "CALLER writes dst (previous consumer)", {}, {dst8});
                model::host_note("bbb_awgn_fill_i8 n " + std::to_string(nn) + " first " + std::to_string(f16));
                CK(bbb_awgn_fill_i8(h, (int8_t *)dst8, nn, f16));
                model::op(user, "CALLER reads dst", {dst8}, {});
                if (rng.chance(30)) { model::host_note("bbb_awgn_prefetch"); CK(bbb_awgn_prefetch(h, nn, f16 + nn)); }
                break;
            }
            case 7: {                  // staging level, or a host synchronisation
                if (rng.chance(50)) { const int lv[4] = {0, 1, 2, 4}; const int l = lv[rng.below(4)]; model::host_note("bbb_lutopt_set_staged " + std::to_string(l)); CK(bbb_lutopt_set_staged(h, l)); }
                else hipStreamSynchronize(user);
                break;
            }
            default: break;
            }
            if (what <= 4) { pos = first + n; runs++; }
            if (!model::errors().empty()) break;
        }
        model::host_note("close");
        CK(bbb_tx_eye_close(oe));
        CK(bbb_tx_ber_sweep_close(os));
        CK(bbb_tx_acf_close(oa));
        CK(bbb_link_sweep_close(ol));
        CK(bbb_tx_xcorr_close(ox));
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
    for (void *p : all) hipFree(p);
    std::printf("{\"sequences\": %ld, \"calls\": %llu, \"runs\": %llu, \"operations_checked\": %llu, \"sequences_with_unordered_access\": %ld, "
                "\"transcript\": \"%016llx\"}\n",
                nseq, (unsigned long long)calls, (unsigned long long)runs, (unsigned long long)model::ops_checked(), bad_sequences,
                (unsigned long long)model::transcript());
    return bad_sequences ? 1 : 0;
}
