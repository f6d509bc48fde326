// Random call sequences over the capture side -- the three objects that own a device and a stream (bbb_errstat, bbb_nco,
// bbb_sinc_eye) and the stateless calls that take samples or packed bits the caller already holds -- over the stream / event
// model of model.cpp, on two caller streams.
//   capture_driver <taps file> <number of sequences> <seed> [max_bad]
// Compiled with the REAL bbb_api.hip, errstat_api.hip, nco_api.hip, sinc_api.hip, eye_api.hip, acf_api.hip, xcorr_api.hip,
// fir_api.hip, ddc_api.hip and hist_api.hip: what is modelled is everything these calls queue -- the objects' buffers, the
// launches of every chunk, a re-bound stream's event, the stream-ordered slab a call owns and its release, the zeroing of a
// decimating slicer's words.  The kernels are stubs that record what the real ones read and write and every scalar they are
// given (the *_kernels.hip files are not compiled), pointers as offsets into the caller's buffers, so the transcript says what
// was queued, in which order, with which arguments, on which stream: a refactor of the host files must leave it as it was.
// Refused calls are part of it, with their return code and bbb_last_error_detail() text.
// The driver uses include/bbb.h and the launch signatures of bbb_common.hpp only.  It plays the caller as driver.cpp does: it
// writes a call's inputs on the call's stream before it and reads the outputs after; each caller stream has buffers of its own.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "bbb_common.hpp"
#include "model.hpp"

// the caller's allocations: a stub names a pointer into one of them by its offset (a chunk loop's progress), any other
// pointer by its offset in its page (the model's allocations start on a page: an object's slot of a small buffer)
static std::vector<std::pair<const char *, size_t>> g_caller;
static std::string at(const void *p) {
    if (!p) return "-";
    for (const auto &b : g_caller)
        if ((const char *)p >= b.first && (const char *)p < b.first + b.second) return std::to_string((const char *)p - b.first);
    return "." + std::to_string((uintptr_t)p & 4095);
}
template <class T> static std::string words_hash(const T *w, size_t n) {     // (a launch's table, folded into one argument)
    uint64_t x = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) x = (x ^ (uint64_t)(int64_t)w[i]) * 1099511628211ull;
    return " table " + std::to_string(x);
}

namespace bbb {

int eye_grid_blocks(uint64_t nsamples) { return (int)std::min<uint64_t>(256, (nsamples + 2047) / 2048); }
int eye_accumulate_launch(const EyeLaunch &a, const int16_t *samples, uint64_t nsamples, uint64_t first_sample, uint32_t *scratch, int blocks,
                          uint64_t *hist, uint64_t *bathtub, hipStream_t st) {
    const std::string what = "eye_kernel" + model::args(a.ncols, a.shift, a.col_origin, a.threshold, a.strict, a.bits != nullptr, a.bit0, a.nbits,
                                                        a.pulser, a.want_hist, a.want_tub, nsamples, first_sample, blocks) + " at " + at(samples);
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
    model::op(st, "acf_kernel" + model::args(p.gx, p.gy, p.smem, p.scratch_words, nfirst, navail, nlags) + " at " + at(samples),
              {samples, scratch, acf}, {scratch, acf});
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
                                                          l.nlags, l.origin) + " at " + at(l.samples) + " " + at(l.bits);
    model::op(st, what, {l.samples, l.bits, scratch, xc}, {scratch, xc});
    return BBB_OK;
}
int xcorr_pulser_bits_launch(uint64_t *dst, uint64_t first_bit, uint64_t nwords, hipStream_t st) {
    model::op(st, "xcorr_pulser_bits_kernel" + model::args(first_bit, nwords), {}, {dst});
    return BBB_OK;
}

int fir_launch(const FirLaunch &a, int mode, int grid, hipStream_t st) {
    const std::string what = "fir_kernel" + model::args(mode, grid, a.nin, a.nout, a.nbefore, a.ngroups, a.shift, a.decim, a.phase, a.threshold,
                                                        a.strict, a.in_vec, a.out_vec) + words_hash(a.taps, BBB_FIR_MAX_TAPS / 2) + " at " + at(a.in) +
                             " " + at(a.out);
    if (mode == 2 && a.decim > 1) model::op(st, what, {a.in, a.out}, {a.out});      // (ORs into the zeroed words)
    else model::op(st, what, {a.in}, {a.out});
    return BBB_OK;
}
int ddc_launch(const DdcLaunch &a, int mode, int cus, hipStream_t st) {
    const std::string what = "ddc_kernel" + model::args(mode, cus, a.nin, a.nout, a.nbefore, a.ngroups, a.shift, a.decim, a.phase, a.first, a.fcw,
                                                        a.pa0, a.in_vec, a.out_vec) + words_hash(a.taps, BBB_FIR_MAX_TAPS / 2) +
                             words_hash(a.rom, 1024) + " at " + at(a.in) + " " + at(a.out);
    model::op(st, what, {a.in}, {a.out});
    return BBB_OK;
}
int sinc_launch(const SincLaunch &a, bool in16, bool out16, int grid, hipStream_t st) {
    model::op(st, "sinc_kernel" + model::args(in16, out16, grid, a.n, a.nbefore, a.shift, a.vec) + words_hash(a.words, 32) + " at " + at(a.in) + " " +
                      at(a.out), {a.in}, {a.out});
    return BBB_OK;
}

uint64_t nco_tiles(uint64_t n) { return (n + 16383) / 16384; }
int nco_launch(const NcoLaunch &a, int grid, hipStream_t st) {
    const std::string what = "nco_kernel" + model::args(grid, a.n, a.fcw, a.am_c, a.fm_c, a.pm_c, a.vec) + " at " + at(a.fm) + " " + at(a.am) + " " +
                             at(a.pm) + " " + at(a.x) + " state " + at(a.in) + " -> " + at(a.out);
    if (a.fm) model::op(st, "nco_scan", {a.fm}, {a.tiles});
    model::op(st, what, {a.fm, a.am, a.pm, a.rom, a.in, a.fm ? a.tiles : nullptr}, {a.x, a.out});
    return BBB_OK;
}
int nco_put_state(const bbb_nco_state &s, bbb_nco_state *dst, hipStream_t st) {
    model::op(st, "nco_put_state" + model::args(s.pa, s.q, s.w, s.y) + " state " + at(dst), {}, {dst});
    return BBB_OK;
}

size_t errstat_scratch_bytes() { return 65536 * 64; }
int errstat_launch(const ErrLaunch &a, bbb_errstat_result *res, void *scratch, hipStream_t st) {
    const std::string what = model::args(a.nbits, a.guard, a.nblock, a.block[0], a.block[1], a.block[2], a.block[3], a.vec) + " at " + at(a.err) + " " +
                             at(a.mask);
    model::op(st, "errstat_tile_kernel" + what, {a.err, a.mask}, {scratch});
    model::op(st, "errstat_stitch", {scratch, res}, {res});
    return BBB_OK;
}
int errstat_skip_launch(bbb_errstat_result *res, uint64_t nbits, hipStream_t st) {
    model::op(st, "errstat_skip" + model::args(nbits), {res}, {res});
    return BBB_OK;
}

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

static uint64_t g_refused = 0;
// a call that must succeed, and one that must be refused: its code and text go into the transcript
#define CK(call)                                                                                                       \
    do {                                                                                                               \
        const int rc_ = (call);                                                                                        \
        if (rc_ != BBB_OK) { std::fprintf(stderr, "%s failed: %s (%s)\n", #call, bbb_strerror(rc_), bbb_last_error_detail()); std::exit(2); } \
    } while (0)
#define REFUSED(call)                                                                                                  \
    do {                                                                                                               \
        const int rc_ = (call);                                                                                        \
        if (rc_ == BBB_OK) { std::fprintf(stderr, "%s was not refused\n", #call); std::exit(2); }                       \
        model::host_note(std::string("refused: " #call " -> ") + std::to_string(rc_) + " " + bbb_last_error_detail());  \
        g_refused++;                                                                                                   \
    } while (0)

struct Rng {
    std::mt19937_64 g;
    explicit Rng(uint64_t s) : g(s) {}
    uint64_t below(uint64_t n) { return n ? g() % n : 0; }
    bool chance(int pct) { return (int)below(100) < pct; }
};

// one caller stream's buffers
struct Set {
    char *big;                       // samples of any width, the oscillator's output: 2^31 + 2^27 bytes
    char *err, *mask;                // packed error streams: 2^31 + 2^20 bytes each
    int32_t *fm;                     // the oscillator's per-sample inputs: 2^24 + 2^17 values each
    uint16_t *am;
    int16_t *pm;
    char *out;                       // what a filter, converter or interpolator writes: 64 MiB
    uint64_t *bits, *hist, *nhist;   // packed data bits (1 MiB); eye histogram; noise histogram
    int64_t *acf, *xc;
};

int main(int argc, char **argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: capture_driver <taps> <nseq> <seed> [max_bad]\n"); return 2; }
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
    if ((int)off.size() - 1 != 256) { std::fprintf(stderr, "expected the n256 tap list\n"); return 2; }
    // a generator without the planes form: 128 rows of two taps
    std::vector<uint16_t> taps_b;
    std::vector<uint32_t> off_b;
    for (int r = 0; r < 128; r++) { off_b.push_back((uint32_t)taps_b.size()); taps_b.push_back((uint16_t)r); taps_b.push_back((uint16_t)((r + 1 + r % 3) % 128)); }
    off_b.push_back((uint32_t)taps_b.size());
    const long nseq = std::atol(argv[2]);
    Rng rng((uint64_t)std::atoll(argv[3]));

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
        return p;
    };
    const uint64_t kFmMax = (1ull << 24) + (1ull << 17);
    Set sets[2];
    for (int i = 0; i < 2; i++) {
        const std::string sfx = i ? " (stream 1)" : " (stream 0)";
        Set &s = sets[i];
        s.big = (char *)alloc((1ull << 31) + (1ull << 27), "caller: samples" + sfx);
        s.err = (char *)alloc((1ull << 31) + (1ull << 20), "caller: packed errors" + sfx);
        s.mask = (char *)alloc((1ull << 31) + (1ull << 20), "caller: packed mask" + sfx);
        s.fm = (int32_t *)alloc(kFmMax * 4, "caller: fm" + sfx);
        s.am = (uint16_t *)alloc(kFmMax * 2, "caller: am" + sfx);
        s.pm = (int16_t *)alloc(kFmMax * 2, "caller: pm" + sfx);
        s.out = (char *)alloc(64ull << 20, "caller: filtered output" + sfx);
        s.bits = (uint64_t *)alloc(1ull << 20, "caller: packed data bits" + sfx);
        s.hist = (uint64_t *)alloc(256 * 64 * 8, "caller: eye histogram" + sfx);
        s.nhist = (uint64_t *)alloc(512 * 8, "caller: noise histogram" + sfx);
        s.acf = (int64_t *)alloc((BBB_ACF_MAX_LAGS + 1) * 8, "caller: acf counters" + sfx);
        s.xc = (int64_t *)alloc(BBB_XCORR_MAX_LAGS * 8, "caller: xcorr counters" + sfx);
    }

    uint64_t init[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    bbb_lutopt *ha = nullptr, *hb = nullptr;             // with the planes form (re-bound call by call); without it (stream 0)
    CK(bbb_lutopt_create(&ha, 256, taps.data(), off.data(), init, 0));
    CK(bbb_lutopt_create(&hb, 128, taps_b.data(), off_b.data(), init, 0));
    CK(bbb_lutopt_set_stream(hb, (void *)user[0]));

    const uint32_t cols[4] = {8, 16, 32, 64};
    auto eye_cfg = [&] {
        bbb_eye_cfg e{};
        e.ncols = cols[rng.below(4)]; e.shift = (uint32_t)rng.below(16); e.col_origin = rng.below(64); e.threshold = (int32_t)rng.below(200) - 100;
        e.strict = (int)rng.below(2);
        return e;
    };
    auto fir_cfg = [&](bool decimate) {
        bbb_fir_cfg f{};
        f.ntaps = 1 + (uint32_t)rng.below(rng.chance(80) ? 40 : 256);
        for (uint32_t i = 0; i < f.ntaps; i++) f.taps[i] = (int16_t)((int)rng.below(21) - 10);
        f.shift = (uint32_t)rng.below(8); f.decim = decimate ? 2 + (uint32_t)rng.below(7) : 1; f.phase = (uint32_t)rng.below(f.decim);
        f.out_bytes = rng.chance(50) ? 2 : 4;
        return f;
    };

    long bad_sequences = 0;
    uint64_t calls = 0, chunked = 0;
    for (long seq = 0; seq < nseq; seq++) {
        hipDeviceSynchronize();
        model::reset_trace();
        model::host_note("sequence " + std::to_string(seq));

        // the three objects, each on one of the caller's streams
        int se = (int)rng.below(2), sn = (int)rng.below(2);
        const int ss = (int)rng.below(2);
        bbb_errstat_cfg ec{};
        ec.guard = (uint32_t)rng.below(rng.chance(50) ? 4 : 100000); ec.nblock = (uint32_t)rng.below(5);
        for (uint32_t j = 0; j < ec.nblock; j++) ec.block_bits[j] = rng.chance(15) ? 0 : 1 + rng.below(1ull << (1 + rng.below(39)));
        bbb_nco_cfg nc{(uint32_t)rng.below(1u << 24), (uint32_t)rng.below(1u << 16), (int32_t)rng.below(1u << 24) - (1 << 23), (int32_t)rng.below(1024) - 512};
        bbb_sinc_cfg sc{1 + (uint32_t)rng.below(2), 1 + (uint32_t)rng.below(2), 0};
        if (sc.in_bytes == 2) sc.shift = (uint32_t)rng.below(16);
        const bbb_eye_cfg seye = eye_cfg();
        const uint64_t schunks[4] = {1000, 4096, 65536, 0};
        const uint64_t schunk = schunks[rng.below(rng.chance(90) ? 3 : 4)];
        bbb_errstat *oe = nullptr; bbb_nco *on = nullptr; bbb_sinc_eye *os = nullptr;
        model::host_note("open: streams " + std::to_string(se) + std::to_string(sn) + std::to_string(ss) + " sinc chunk " + std::to_string(schunk));
        CK(bbb_errstat_open(&ec, 0, (void *)user[se], &oe));
        CK(bbb_nco_open(&nc, 0, (void *)user[sn], &on));
        CK(bbb_sinc_eye_open(&sc, &seye, schunk, 0, (void *)user[ss], &os));
        bool ended = false;

        const int ncalls = 8 + (int)rng.below(20);
        for (int c = 0; c < ncalls; c++, calls++) {
            const int what = (int)rng.below(24);
            const int sx = (int)rng.below(2);            // the stream of a stateless call
            Set &x = sets[sx];
            hipStream_t ux = user[sx];
            switch (what) {
            case 0: case 1: {          // errors: a few words, now and then more than a launch takes, or a ragged end
                Set &b = sets[se];
                uint64_t nbits = 64 * (1 + rng.below(1u << 14));
                if (rng.chance(8)) { nbits = (1ull << 34) + 64 * rng.below(1000); chunked++; }
                if (rng.chance(6)) nbits -= 1 + rng.below(63);
                const uint64_t *e = (const uint64_t *)b.err + rng.below(4), *m = rng.chance(50) ? (const uint64_t *)b.mask + rng.below(4) : nullptr;
                model::op(user[se], "CALLER writes the packed errors", {}, {b.err, b.mask});
                model::host_note("bbb_errstat_accumulate nbits " + std::to_string(nbits));
                if (ended) REFUSED(bbb_errstat_accumulate(oe, e, m, nbits));
                else { CK(bbb_errstat_accumulate(oe, e, m, nbits)); ended = (nbits & 63) != 0; }
                break;
            }
            case 2: {
                const uint64_t nbits = rng.chance(90) ? 64 * rng.below(1u << 20) : rng.below(1ull << 40);
                model::host_note("bbb_errstat_skip " + std::to_string(nbits));
                if (ended) REFUSED(bbb_errstat_skip(oe, nbits));
                else { CK(bbb_errstat_skip(oe, nbits)); ended = (nbits & 63) != 0; }
                break;
            }
            case 3: {
                if (rng.chance(60)) { bbb_errstat_result r; model::host_note("bbb_errstat_read"); CK(bbb_errstat_read(oe, &r)); }
                else { model::host_note("bbb_errstat_reset"); CK(bbb_errstat_reset(oe)); ended = false; }
                break;
            }
            case 4: {                  // the statistics move to a stream: the other one, or the one they are on
                se = (int)rng.below(2);
                model::host_note("bbb_errstat_set_stream -> " + std::to_string(se));
                CK(bbb_errstat_set_stream(oe, (void *)user[se]));
                break;
            }
            case 5: case 6: {          // the oscillator: constants or buffers, now and then more than a launch takes
                Set &b = sets[sn];
                const bool fm = rng.chance(40), am = rng.chance(30), pm = rng.chance(30);
                uint64_t n = 1 + rng.below(1u << 17);
                if (rng.chance(8)) { n = fm || am || pm ? (1ull << 24) + 1 + rng.below(1u << 16) : (1ull << 30) + 1 + rng.below(1u << 16); chunked++; }
                const uint64_t o = rng.below(9);
                model::op(user[sn], "CALLER writes fm, am, pm; the previous reader of x", {}, {b.fm, b.am, b.pm, b.big});
                model::host_note("bbb_nco_run n " + std::to_string(n));
                CK(bbb_nco_run(on, fm ? b.fm + o : nullptr, am ? b.am + o : nullptr, pm ? b.pm + o : nullptr, n, (int16_t *)b.big + rng.below(9)));
                model::op(user[sn], "CALLER reads x", {b.big}, {});
                break;
            }
            case 7: {
                const int k = (int)rng.below(4);
                if (k == 0) { bbb_nco_state s; model::host_note("bbb_nco_get_state"); CK(bbb_nco_get_state(on, &s)); }
                else if (k == 1) {
                    const bbb_nco_state s{(uint32_t)rng.below(1u << 24), (int32_t)rng.below(65536) - 32768, (int32_t)rng.below(65536) - 32768, (int32_t)rng.below(1u << 31)};
                    model::host_note("bbb_nco_set_state");
                    CK(bbb_nco_set_state(on, &s));
                } else if (k == 2) {
                    nc.fcw = (uint32_t)rng.below(1u << 24); nc.pm = (int32_t)rng.below(1024) - 512;
                    model::host_note("bbb_nco_set_cfg");
                    CK(bbb_nco_set_cfg(on, &nc));
                } else {
                    sn = (int)rng.below(2);
                    model::host_note("bbb_nco_set_stream -> " + std::to_string(sn));
                    CK(bbb_nco_set_stream(on, (void *)user[sn]));
                }
                break;
            }
            case 8: case 9: {          // the interpolated eye: 1, 2 or more chunks with a ragged last one
                Set &b = sets[ss];
                const uint64_t ch = schunk ? schunk : 1ull << 24, nch = 1 + rng.below(3);
                const uint64_t nin = rng.chance(5) ? 0 : (nch - 1) * ch + 1 + rng.below(ch);
                const uint32_t before = (uint32_t)rng.below(12);
                const uint64_t first = rng.chance(70) ? rng.below(1u << 20) : (1ull << 57) + rng.below(1u << 20);
                if (nin > ch) chunked++;
                model::op(user[ss], "CALLER writes the samples and the histogram", {}, {b.big, b.hist});
                model::host_note("bbb_sinc_eye_run nin " + std::to_string(nin) + " before " + std::to_string(before) + " first " + std::to_string(first));
                CK(bbb_sinc_eye_run(os, b.big + 32 * sc.in_bytes + rng.below(3) * sc.in_bytes, nin, before, first, b.hist));
                model::op(user[ss], "CALLER reads the histogram", {b.hist}, {});
                break;
            }
            case 10: {
                const bbb_eye_cfg e = eye_cfg();
                const uint64_t n = rng.chance(5) ? 0 : 1 + rng.below(1u << 20), first = rng.below(1ull << 40);
                model::op(ux, "CALLER writes the samples and the histogram", {}, {x.big, x.hist});
                model::host_note("bbb_eye_accumulate_i16 n " + std::to_string(n) + " first " + std::to_string(first));
                CK(bbb_eye_accumulate_i16((const int16_t *)x.big + rng.below(9), n, first, &e, x.hist, 0, (void *)ux));
                model::op(ux, "CALLER reads the histogram", {x.hist}, {});
                break;
            }
            case 11: {
                const uint32_t nlags = 1 + (uint32_t)rng.below(BBB_ACF_MAX_LAGS);
                const uint64_t n = rng.chance(5) ? 0 : 1 + rng.below(1u << 20), avail = n + rng.below(nlags);
                model::op(ux, "CALLER writes the samples and the acf counters", {}, {x.big, x.acf});
                model::host_note("bbb_acf_accumulate_i16 n " + std::to_string(n) + " avail " + std::to_string(avail) + " nlags " + std::to_string(nlags));
                CK(bbb_acf_accumulate_i16((const int16_t *)x.big + rng.below(9), n, avail, nlags, x.acf, 0, (void *)ux));
                model::op(ux, "CALLER reads the acf counters", {x.acf}, {});
                break;
            }
            case 12: {
                bbb_xcorr_cfg xcfg{1u << rng.below(6), 0, 0};
                xcfg.nlags = 1 + (uint32_t)rng.below(std::min<uint32_t>(64 * xcfg.spb, BBB_XCORR_MAX_LAGS));
                const uint64_t n = rng.chance(5) ? 0 : 1 + rng.below(1u << 18), first = rng.below(1u << 20);
                const uint64_t nbits = (first + n) / xcfg.spb + 2;
                model::op(ux, "CALLER writes the samples, the bits and the xcorr counters", {}, {x.big, x.bits, x.xc});
                model::host_note("bbb_xcorr_accumulate_i16 n " + std::to_string(n) + " first " + std::to_string(first));
                CK(bbb_xcorr_accumulate_i16((const int16_t *)x.big + rng.below(9), n, first, x.bits, 0, nbits, &xcfg, x.xc, 0, (void *)ux));
                model::op(ux, "CALLER reads the xcorr counters", {x.xc}, {});
                break;
            }
            case 13: case 14: case 15: {   // the filter and the slicer, with and without decimation
                const bool slice = what == 15 || rng.chance(30);
                const bbb_fir_cfg f = fir_cfg(rng.chance(50));
                const uint64_t nin = rng.chance(5) ? rng.below(3) : 1 + rng.below(1u << 18);
                const uint32_t before = (uint32_t)rng.below(300);
                const int16_t *in = (const int16_t *)x.big + 256 + rng.below(9);
                uint64_t got = 0;
                model::op(ux, "CALLER writes the samples; the previous reader of the output", {}, {x.big, x.out});
                model::host_note(std::string(slice ? "bbb_fir_slice" : "bbb_fir_filter") + " nin " + std::to_string(nin) + " before " + std::to_string(before));
                if (slice) CK(bbb_fir_slice(in, nin, before, &f, (int32_t)rng.below(2000) - 1000, (int)rng.below(2), (uint64_t *)x.out + rng.below(3), &got, 0, (void *)ux));
                else CK(bbb_fir_filter(in, nin, before, &f, x.out + 4 * rng.below(5), &got, 0, (void *)ux));
                model::host_note("nout " + std::to_string(got));
                model::op(ux, "CALLER reads the output", {x.out}, {});
                break;
            }
            case 16: case 17: {
                const bbb_fir_cfg f = fir_cfg(rng.chance(60));
                const bbb_ddc_cfg d{(uint32_t)rng.below(1u << 24), (uint32_t)rng.below(1u << 24), (uint32_t)rng.below(3)};
                const uint64_t nin = rng.chance(5) ? rng.below(3) : 1 + rng.below(1u << 18), first = rng.chance(70) ? rng.below(1u << 30) : (1ull << 57) + rng.below(1u << 30);
                const uint32_t before = (uint32_t)rng.below(300);
                uint64_t got = 0;
                model::op(ux, "CALLER writes the samples; the previous reader of the output", {}, {x.big, x.out});
                model::host_note("bbb_ddc_run nin " + std::to_string(nin) + " before " + std::to_string(before) + " first " + std::to_string(first));
                CK(bbb_ddc_run((const int16_t *)x.big + 256 + rng.below(9), nin, before, first, &d, &f, x.out + 8 * rng.below(3), &got, 0, (void *)ux));
                model::host_note("nout " + std::to_string(got));
                model::op(ux, "CALLER reads the output", {x.out}, {});
                break;
            }
            case 18: {
                bbb_sinc_cfg s{1 + (uint32_t)rng.below(2), 1 + (uint32_t)rng.below(2), 0};
                if (s.in_bytes == 2) s.shift = (uint32_t)rng.below(16);
                const uint64_t nin = rng.chance(5) ? 0 : 1 + rng.below(1u << 20);
                model::op(ux, "CALLER writes the samples; the previous reader of the output", {}, {x.big, x.out});
                model::host_note("bbb_sinc_interpolate nin " + std::to_string(nin));
                CK(bbb_sinc_interpolate(x.big + s.in_bytes * (16 + rng.below(3)), nin, (uint32_t)rng.below(12), &s, x.out + s.out_bytes * rng.below(9), 0, (void *)ux));
                model::op(ux, "CALLER reads the output", {x.out}, {});
                break;
            }
            case 19: {
                const uint64_t nbits = rng.chance(5) ? 0 : 1 + rng.below(1u << 22);
                uint64_t nerr = 0;
                model::op(ux, "CALLER writes the packed bits", {}, {x.bits});
                model::host_note("bbb_prbs_check nbits " + std::to_string(nbits));
                CK(bbb_prbs_check(31, 1 + rng.below(1000), rng.below(1ull << 40), nbits, x.bits, &nerr, 0, (void *)ux));
                break;
            }
            case 20: {
                bbb_tx_cfg tx{};
                for (int i = 0; i < 64; i++) tx.coeffs[i] = (int16_t)((int)rng.below(511) - 255);
                tx.source = (int)rng.below(2); tx.prbs_k = 31; tx.prbs_state = 1 + rng.below(1000); tx.bit_en = 1;
                const uint64_t n = rng.chance(5) ? 0 : 1 + rng.below(1u << 20), first = rng.chance(50) ? rng.below(64) : rng.below(1ull << 40);
                model::op(ux, "CALLER: the previous reader of the waveform", {}, {x.big});
                model::host_note("bbb_shaper_fill_i16 n " + std::to_string(n) + " first " + std::to_string(first));
                CK(bbb_shaper_fill_i16(&tx, (int16_t *)x.big + 8 * rng.below(3), n, first, 0, (void *)ux));
                model::op(ux, "CALLER reads the waveform", {x.big}, {});
                break;
            }
            case 21: case 22: {        // the noise histogram: with the planes form (through memory, staged, both) and without
                const bool planes = rng.chance(50);
                const uint64_t sizes[4] = {4099, 1ull << 24, (1ull << 24) + 4099, (1ull << 30) + (1ull << 24) + 77};
                const uint64_t n = planes ? sizes[rng.below(4)] : rng.chance(10) ? (1ull << 26) + 16 * rng.below(1000) : 1 + rng.below(1u << 20);
                const uint64_t first = 16 + rng.below(1u << 30) * 16;
                const int s = planes ? sx : 0;
                if (planes) CK(bbb_lutopt_set_stream(ha, (void *)ux));
                model::op(user[s], "CALLER writes the noise histogram", {}, {sets[s].nhist});
                model::host_note(std::string("bbb_awgn_hist ") + (planes ? "planes" : "generic") + " n " + std::to_string(n) + " first " + std::to_string(first));
                CK(bbb_awgn_hist(planes ? ha : hb, sets[s].nhist, n, first));
                model::op(user[s], "CALLER reads the noise histogram", {sets[s].nhist}, {});
                break;
            }
            case 23: {                 // refused calls: null and misaligned pointers, an output over the samples, rules of a cfg
                const bbb_eye_cfg e = eye_cfg();
                bbb_eye_cfg bad = e;
                const bbb_fir_cfg f = fir_cfg(false);
                const bbb_ddc_cfg d{1, 2, 0};
                bbb_sinc_cfg s{2, 2, 3};
                bbb_sinc_eye *none = nullptr;
                uint64_t got = 0;
                const int16_t *in = (const int16_t *)x.big + 512;
                switch ((int)rng.below(14)) {
                case 0: REFUSED(bbb_eye_accumulate_i16(in, 100, 0, &e, nullptr, 0, (void *)ux)); break;
                case 1: REFUSED(bbb_eye_accumulate_i16((const int16_t *)(x.big + 1), 100, 0, &e, x.hist, 0, (void *)ux)); break;
                case 2: REFUSED(bbb_acf_accumulate_i16(nullptr, 100, 100, 16, x.acf, 0, (void *)ux)); break;
                case 3: REFUSED(bbb_xcorr_accumulate_i16(in, 100, 0, x.bits, 50, 10, nullptr, x.xc, 0, (void *)ux)); break;
                case 4: REFUSED(bbb_fir_filter(in, 1000, 300, &f, (void *)(in + 10), &got, 0, (void *)ux)); break;
                case 5: REFUSED(bbb_fir_filter(in, 1000, 300, &f, (void *)(in - std::min<uint32_t>(300, f.ntaps - 1) - 1), &got, 0, (void *)ux)); break;
                case 6: REFUSED(bbb_fir_slice(in, 1000, 0, &f, 0, 0, (uint64_t *)(x.out + 4), &got, 0, (void *)ux)); break;
                case 7: REFUSED(bbb_ddc_run(in, 1000, 5, 0, &d, &f, (void *)(in + 998), &got, 0, (void *)ux)); break;
                case 8: REFUSED(bbb_ddc_run(in, 1000, 5, 1ull << 58, &d, &f, x.out, &got, 0, (void *)ux)); break;
                case 9: REFUSED(bbb_sinc_interpolate(x.big + 64, 100, 3, &s, x.out + 1, 0, (void *)ux)); break;
                case 10: bad.ncols = 7 + 2 * (uint32_t)rng.below(20); REFUSED(bbb_sinc_eye_open(&s, &bad, 0, 0, (void *)ux, &none)); break;
                case 11: bad.shift = 16 + (uint32_t)rng.below(20); REFUSED(bbb_sinc_eye_open(&s, &bad, 0, 0, (void *)ux, &none)); break;
                case 12: if (rng.chance(50)) REFUSED(bbb_sinc_eye_open(&s, nullptr, 0, 0, (void *)ux, &none)); else REFUSED(bbb_sinc_eye_open(&s, &e, (1ull << 27) + 1, 0, (void *)ux, &none)); break;
                default: REFUSED(bbb_nco_run(on, (const int32_t *)(x.big + 2), nullptr, nullptr, 10, (int16_t *)x.big)); break;
                }
                break;
            }
            default: break;
            }
            if (!model::errors().empty()) break;
        }
        model::host_note("close");              // (with whatever the last calls queued still on the streams)
        CK(bbb_errstat_close(oe));
        CK(bbb_nco_close(on));
        CK(bbb_sinc_eye_close(os));
        if (!model::errors().empty()) {
            bad_sequences++;
            if (bad_sequences <= 3)
                for (const std::string &e : model::errors()) std::fprintf(stderr, "sequence %ld: UNORDERED ACCESS\n  %s\n", seq, e.c_str());
            model::clear_errors();
            if (bad_sequences >= max_bad) break;
        }
    }
    CK(bbb_lutopt_destroy(ha));
    CK(bbb_lutopt_destroy(hb));
    for (void *p : all) hipFree(p);
    std::printf("{\"sequences\": %ld, \"calls\": %llu, \"chunked\": %llu, \"refused\": %llu, \"operations_checked\": %llu, "
                "\"sequences_with_unordered_access\": %ld, \"transcript\": \"%016llx\"}\n",
                nseq, (unsigned long long)calls, (unsigned long long)chunked, (unsigned long long)g_refused,
                (unsigned long long)model::ops_checked(), bad_sequences, (unsigned long long)model::transcript());
    return bad_sequences ? 1 : 0;
}
