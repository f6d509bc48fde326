// bbb_mc -- a plain C++ caller of the C ABI (include/bbb.h): the Monte-Carlo loops of BASELINE.json configs[1..4].
// No torch, no Python: the library, hipMalloc'd buffers, std::thread and printf.
// Build: make -C examples   (hipcc, links ../basebandboard_amd/libbbb_hip.so)
//
//   bbb_mc [--matrix FILE] [--init HEX] [--gpus N] [--json 1]
//          BER sweep:   [--prbs 31] [--bits 1e9] [--nv 8] [--ebn0 A:B:STEP] [--seeds N] [--shard bits|seeds|trials|groups]
//          AWGN fill:   --nsamples 1e9 [--steps 5] [--staged 0|1|m]   the sample stream drained through bbb_awgn_stream_next;
//                       --staged picks the level of bbb_lutopt_set_staged for it (default: the stream's own choice, two reads
//                       per sample kernel; 0 = plain bbb_awgn_fill_i8 calls in the one-kernel form)
//          loopback:    --loopback BITS
//          eye:         --eye FILE [--eye-samples 1e6] [--prbs 31] [--nv 8] [--shape 16] [--shift 4]   eye diagram and bathtub of the
//                       transmitter (bbb_tx_eye_*; raised-cosine set `shape` of tx.py:54, noise_var nv): the DSO's persistence
//                       image (gateware/bbb/dso.py, 256 rows x 64 columns) written to FILE as a PGM, one line per bathtub phase
//          tx sweep:    --tx-sweep 1 [--eye-samples 1e6] [--prbs 31] [--shape 16] [--nv-range 0:15]   BER of the shaped link for
//                       every noise_var A..B of raised-cosine set `shape` in one pass (bbb_tx_ber_sweep_*): one JSON line per
//                       setting and phase (bits decided, errors) after a header line
//          nco:         --nco FILE [--fcw 1048576] [--am 16384] [--nco-samples 1e6]   the NCO's tone (bbb_nco_*), written as
//                       little-endian int16 samples (software/memdump's `<h` format)
//          ddc:         --ddc 1 [--fcw 1048576] [--am 16384] [--pm 100] [--nco-samples 1e6]   the receive half of the NCO
//                       (bbb_ddc_run): the tone made with the constant phase offset `pm` (in 1/1024 turn) is taken back to
//                       baseband by a converter at the same fcw with pa0 = -3 fcw, a 64-tap boxcar at decim 64, polar outputs:
//                       one JSON line with the range of the magnitude (about am / 4) and of the phase (1/65536 turn: about 64 pm - 16384,
//                       the tone being a sine and the converter's reference a cosine)
//          carrier:     --carrier OFF [--fcw 1048576] [--am 16384] [--nco-samples 1e6]   carrier recovery (bbb_carrier_run): the NCO's
//                       tone phase-modulated by half a turn per bit 1, 64 samples a bit, through a down-converter whose fcw lies
//                       OFF (nonzero, |OFF| <= 4096) below the transmitter's.  Prints the errors the sign of Q leaves, those
//                       left behind the recovery (L 32, init_phase 16384) and the estimated offset in turns per pair.
//          sinc:        --sinc FILE [--eye-samples 1e6] [--prbs 31] [--nv 8] [--shape 16] [--shift 4]   the scope's 16x sinc
//                       interpolator (bbb_sinc_*; gateware/bbb/sinc.py): one JSON line with the module's 1024 outputs for the
//                       7-cycle sine of the reference's test, then the eye of a capture at 4 samples per bit (every second
//                       sample of the transmitter's waveform) after interpolation, 64 columns per bit, to FILE as a PGM
//          fir:         --fir 1 [--eye-samples 1e6] [--prbs 31] [--nv 8]   the moving-average receiver of gateware/bbb/rx.py:24-26
//                       (bbb_fir_slice with the taps of bbb_fir_moving_average) beside the plain sign slicer (bbb_rx_slice) over a
//                       noisy transmission of the 4-sample rectangular pulse (the last set of PRBSShaper.from_rcf), each at 8
//                       samples per bit into the exact detector: one JSON line with both error counts
//          dfe:         --dfe 1 [--eye-samples 1e6] [--prbs 31] [--nv 8]   the same receiver behind an echo of 0.7 one bit late
//                       (bbb_fir_filter as the channel), without and with one feedback tap (bbb_dfe_run): errors of both
//          mlse:        --mlse MEM [--eye-samples 1e6] [--prbs 31] [--nv 8]   the same record through the moving average, the DFE
//                       and the Viterbi sequence detector with a target of MEM (1..4) symbols of memory (bbb_mlse_run)
//          timing:      --timing OFFSET [--eye-samples 1e6] [--prbs 31] [--nv 8]   the record of --fir resampled on the host with a
//                       clock offset of OFFSET / 65536 (20: 305 ppm), then the moving-average slicer at its one fixed phase beside
//                       the timing recovery (bbb_timing_run) behind the same filter: errors of both, wraps and bits emitted
//                       from the exact detector, and the call's region counters
//          fec:         --fec P [--eye-samples 1e6] [--prbs 31] [--nv 8]   forward error correction (bbb_conv_*): eye-samples PRBS bits
//                       through the K = 7 code (0171, 0133), P = 1: rate 1/2, P = 2, 3, 5, 7: punctured to 2/3, 3/4, 5/6, 7/8,
//                       sent as +-64 plus Gaussian noise of sigma 5 nv made on the host, sliced (bbb_rx_slice) and decoded
//                       from the hard decisions and from the soft values: one JSON line with the channel's errors and both
//                       decoders' (sigma 40 of the default nv is past what hard decisions survive at rate 3/4; --nv 5 is not)
//          rs:          --rs I [--eye-samples 1e6] [--prbs 31] [--sigma 42]   the concatenated code (bbb_rs_* around bbb_conv_*): the whole
//                       CCSDS (255, 223) frames of depth I (1..8) that eye-samples PRBS bits fill, RS-encoded, their bits through
//                       the K = 7 code (0171, 0133) at rate 1/2, sent as +-64 plus Gaussian noise of sigma made on the host, sliced,
//                       Viterbi-decoded from the hard decisions and RS-decoded: one JSON line with the bit errors of the channel,
//                       behind the Viterbi decoder and behind the RS decoder, and the RS decoder's statistics
//                       --sync J with --rs: a CCSDS marker attached to every coded frame and the payload randomised
//                       (bbb_frame_attach), J >= 0 random bits put in front, the whole channel inverted; behind the Viterbi decoder
//                       the frames are found and cut out (bbb_framesync_run, bbb_frame_extract; tol_search 2, tol_lock 6, verify 1,
//                       flywheel 2) and handed to the RS decoder; the line gains the synchroniser's counters
//          ldpc:        --ldpc P [--eye-samples 1e6] [--prbs 31] [--sigma 32]   the LDPC codec (bbb_ldpc_*): the whole codewords of the
//                       array code array(P, 4, 16) (P an odd prime >= 17; 127: n = 2032, rate 3/4) that eye-samples PRBS bits fill,
//                       encoded, sent as +-64 plus Gaussian noise of sigma made on the host, decoded from the soft values (max_iter 20,
//                       norm 12): one JSON line with the channel's errors, the data errors behind the decoder and its statistics
//          link:        --link 1 [--eye-samples 1e6] [--prbs 31] [--nv 8] [--shape 16] [--delay 2]   the bathtub of one transmitter
//                       setting decided on the raw sample (bbb_tx_ber_sweep_*) and behind the moving average of rx.py:24-26
//                       (bbb_link_sweep_* with the taps of bbb_fir_moving_average, the filtered stream re-timed by `delay`), the
//                       waveform never materialised: one JSON line per phase with the bits decided and both error counts
//          errstat:     --errstat 1 [--bits 1e8] [--prbs 31] [--guard 64]   how errors are distributed (bbb_errstat_*): a PRBS stream
//                       with a bit flipped every 99991 positions and one burst of 3 k flipped bits, through the exact detector
//                       (bbb_prbs_detector_stream) into the error statistics with `reload` as the mask: one JSON line with the
//                       totals, the gaps, the bursts (the open one closed on the host) and the errored blocks of 1e3 .. 1e6 bits
//          xcorr:       --xcorr 1 [--lags 64] [--eye-samples 1e6] [--prbs 31] [--shape 16]   the transmitter's pulse response with
//                       the noise off (bbb_tx_xcorr_*): the waveform correlated with its own data bits, divided by the number of
//                       terms of each lag, printed beside the coefficient set it was shaped with: one JSON line
//          spectrum:    --spectrum FILE [--lags 256] [--eye-samples 1e6] [--prbs 31] [--nv 8] [--shape 16]   autocorrelation
//                       counters of the transmitter's waveform (bbb_tx_acf_*) and the power spectrum from them (Bartlett lag
//                       window, mean removed, one-sided, fs = 1): FILE gets a CSV k,freq,psd,psd_db (psd_db is nan in a bin
//                       where the finite-record estimate dips below zero); one JSON line with the counters
//          grng eval:   --grng-eval N [--first-step S]   the evaluation of software/clt-grng/clt-grng-evaluate.py:18-31 over N
//                       samples of the generator's stream from clock S (bbb_awgn_hist in chunks; the samples never leave the
//                       chip): the reference's two lines (theoretical and sample mean and variance, from the counters, in
//                       double), then one JSON line with the counters' total, the lowest and highest occupied bin and the
//                       elapsed milliseconds
//          search:      --search K [--seed S] [--count N] --out FILE    the reference's rnghunt (software/rnghunt/src/bin/
//                       rnghunt.rs:13-66) on the GPU: candidates of `seed` are examined in windows of N (default 65536)
//                       until one has period 2^K - 1; it is written to FILE in the reference's `out` format (K lines of K
//                       characters 0/1), read back and re-checked (bbb_lutopt_is_full_period)
//
// --matrix   the reference's 0/1 text format (software/rnghunt/matrices/256); default: the shipped n256 matrix
//            (gateware/bbb/rng_recurrences.py:172-259, used by tx.py:70).
// --init     the generator's reset state (hex, default 1: gateware/bbb/rng.py:21).
// --ebn0     A:B:STEP in dB (also --from/--to/--step); amplitude per point for sigma = 8 noise_var, one sample per bit.
// --gpus N   BER sweep: bbb_ber_sweep_multi over devices 0..N-1 -- one host thread per device and ONE RCCL
//            all-reduce of the uint64 counters.  --shard bits (default): every device runs every point over its
//            slice of the bit range, the counters equal the 1-GPU counters exactly; seeds: device d runs every
//            point on its own seed (below), counters summed (points x seeds, BASELINE configs[4]); trials: point i
//            on device i % N; groups (with --seeds S): the sweep once per seed as ONE call of S x points trials, a seed's
//            sweep on one device (group q on device q % N: configs[4] as eight sweeps on one device, one each on eight).  AWGN fill: device d reads stream positions [16 + 2^48 d + s n, +n) in step s -- its own
//            contiguous stretch of the one sequential stream, no collective.
// --multi 1  take the bbb_ber_sweep_multi route (RCCL) even with --gpus 1.
// --seeds N  (1 GPU) repeat the sweep on N seeds and sum the counters.  Seed d = the reset state `init` advanced 2^48 d
//            clocks (GF(2) jump-ahead, bbb_lutopt_state_at): disjoint stretches of the generator's one cycle.  (Reset
//            states that differ by small integers are XOR-dependent streams, and nothing would keep them from overlapping.)
// --json 1   one JSON object per line (points, then a summary with rates and the roofline fraction) instead of
//            the table.
#include "../include/bbb.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#define CHECK(call)                                                                                     \
    do {                                                                                                \
        int rc_ = (call);                                                                               \
        if (rc_ != BBB_OK) {                                                                            \
            std::fprintf(stderr, "%s: %s (%s)\n", #call, bbb_strerror(rc_), bbb_last_error_detail());   \
            return 1;                                                                                   \
        }                                                                                               \
    } while (0)

static const double kHbmPeakGBs = 8000.0;     // MI355X HBM3E, nominal

// The raised-cosine tap set of PRBSShaper.from_rcf (bitshaper.py:97-107; basebandboard_amd.bitshaper.rcf_coefficients): T = 8
// samples per bit, peak 254, the two singular taps replaced by their limit, truncated towards zero.
static double sinc(double x) { return x == 0.0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x); }
static void rcf_taps(double beta, int16_t *c) {
    const double T = 8;
    for (int i = 0; i < 64; i++) {
        const double t = i - 32;
        double v;
        if (beta != 0.0 && std::fabs(t) == T / (2 * beta)) v = M_PI / (4 * T) * sinc(1 / (2 * beta));
        else v = 1 / T * sinc(t / T) * std::cos(M_PI * beta * t / T) / (1 - (2 * beta * t / T) * (2 * beta * t / T));
        c[i] = (int16_t)(long long)(v * T * 254);
    }
}

static bool load_taps_file(const std::string &path, int *k, std::vector<uint16_t> *taps, std::vector<uint32_t> *off) {
    // packed tap lists: one row per line, space separated column indices (basebandboard_amd/data/*.taps)
    FILE *f = std::fopen(path.c_str(), "r");
    if (!f) return false;
    char line[8192];
    off->assign(1, 0);
    while (std::fgets(line, sizeof line, f)) {
        char *p = line, *e = nullptr;
        bool any = false;
        for (;;) {
            const long v = std::strtol(p, &e, 10);
            if (e == p) break;
            taps->push_back((uint16_t)v);
            p = e;
            any = true;
        }
        if (any) off->push_back((uint32_t)taps->size());
    }
    std::fclose(f);
    *k = (int)off->size() - 1;
    return *k > 0;
}

static double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Matrix {
    int n = 0;
    std::vector<uint16_t> taps;
    std::vector<uint32_t> off;
};

// AWGN fill on one device: `steps` consecutive fills of n samples; device d reads its own stretch of the stream, 2^48 d steps in
struct FillResult { int rc = 0; std::string err; double kernel_ms = 0, seed_ms = 0, wall_s = 0; uint64_t launches = 0; std::vector<int8_t> head; };
static void fill_worker(const Matrix &m, unsigned long long init0, int dev, int ndev, uint64_t n, int steps, int staged, FillResult *res) {
    auto body = [&]() -> int {
        if (hipSetDevice(dev) != hipSuccess) { res->err = "hipSetDevice failed"; return 1; }
        const uint64_t init[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        bbb_lutopt *h = nullptr;
        int rc = bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, dev);
        if (rc) { res->err = bbb_last_error_detail(); return rc; }
        int8_t *buf = nullptr;
        if (hipMalloc((void **)&buf, (n + 15) / 16 * 16) != hipSuccess) { res->err = "hipMalloc failed"; return 1; }
        (void)ndev;
        const uint64_t first0 = (uint64_t)16 + ((uint64_t)dev << 48);
        auto first = [&](int s) { return first0 + (uint64_t)s * n; };
        // the sample stream as an object: the library owns staging, the two-kernel form and the announcement of every next read
        bbb_awgn_stream *st = nullptr;
        if (staged > 0) (void)bbb_lutopt_set_staged(h, staged);             // an explicit level; otherwise the stream picks its own
        if (staged != 0) {
            if ((rc = bbb_awgn_stream_open(h, n, first0, 1, &st))) { res->err = bbb_last_error_detail(); return rc; }
            if ((rc = bbb_awgn_stream_next(st, buf))) { res->err = bbb_last_error_detail(); return rc; }       // builds the jump plan
        } else if ((rc = bbb_awgn_fill_i8(h, buf, n, first(0)))) { res->err = bbb_last_error_detail(); return rc; }
        res->head.resize(n < 64 ? n : 64);
        (void)hipMemcpy(res->head.data(), buf, res->head.size(), hipMemcpyDeviceToHost);
        if (st) (void)bbb_awgn_stream_seek(st, first(1));      // (drops what a sample kernel produced ahead: the timed steps start on a launch)
        (void)bbb_lutopt_profile(h, 1);
        (void)hipDeviceSynchronize();
        const double t0 = now_s();
        for (int s = 1; s <= steps; s++) {
            if (st) rc = bbb_awgn_stream_next(st, buf);
            else {
                rc = bbb_awgn_fill_i8(h, buf, n, first(s));
                if (!rc) (void)bbb_awgn_prefetch(h, n, first(s + 1));       // the next step's seeding runs beside this step's kernel
            }
            if (rc) { res->err = bbb_last_error_detail(); return rc; }
        }
        (void)hipDeviceSynchronize();
        res->wall_s = now_s() - t0;
        uint64_t calls = 0;
        (void)bbb_lutopt_profile_read(h, &res->seed_ms, &res->kernel_ms, &calls, 1);
        if (calls) { res->kernel_ms /= (double)calls; res->seed_ms /= (double)calls; }
        res->launches = calls;
        if (st) (void)bbb_awgn_stream_close(st);
        (void)hipFree(buf);
        (void)bbb_lutopt_destroy(h);
        return 0;
    };
    res->rc = body();
}

int main(int argc, char **argv) {
    std::string matrix, shard = "bits";
    int k = 31, nv = 8, seeds = 1, gpus = 1, json = 0, steps = 5, multi = 0, staged = -1, search_k = 0;
    unsigned long long search_seed = 1, search_count = 65536;
    std::string outfile;
    std::string eyefile, specfile, ncofile, sincfile;
    unsigned long nco_fcw = 1ul << 20, nco_am = 1ul << 14;      // NCOTest's resets (gateware/top.py:54-55)
    double nco_samples = 1e6;
    int lags = 256;
    bool lags_set = false;
    int shape = 16, eye_shift = 4;
    double eye_samples = 1e6;
    int tx_sweep = 0, nv_lo = 0, nv_hi = 15, fir = 0, dfe = 0, mlse = 0, timing = 0, fec = 0, rs = 0, rs_sigma = 42, ldpc = 0, ldpc_sigma = -1, sync_junk = -1, link = 0, link_delay = 2, errstat = 0, xcorr = 0, ddc = 0, nco_pm = 100, carrier = 0;
    unsigned long errstat_guard = 64;
    unsigned long long init0 = 1;
    double bits = 1e9, from = 0, to = 10, step = 1, loopback = 0, nsamples = 0, grng_eval = 0;
    unsigned long long first_step = 0;
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string a = argv[i];
        const char *v = argv[i + 1];
        if (a == "--matrix") matrix = v;
        else if (a == "--k" || a == "--prbs") k = std::atoi(v);
        else if (a == "--init") init0 = std::strtoull(v, nullptr, 16);
        else if (a == "--seeds") seeds = std::atoi(v);
        else if (a == "--nv") nv = std::atoi(v);
        else if (a == "--bits") bits = std::atof(v);
        else if (a == "--from") from = std::atof(v);
        else if (a == "--to") to = std::atof(v);
        else if (a == "--step") step = std::atof(v);
        else if (a == "--ebn0") {
            if (std::sscanf(v, "%lf:%lf:%lf", &from, &to, &step) != 3) { std::fprintf(stderr, "--ebn0 A:B:STEP\n"); return 2; }
        }
        else if (a == "--loopback") loopback = std::atof(v);
        else if (a == "--nsamples") nsamples = std::atof(v);
        else if (a == "--grng-eval") grng_eval = std::atof(v);
        else if (a == "--first-step") first_step = std::strtoull(v, nullptr, 0);
        else if (a == "--steps") steps = std::atoi(v);
        else if (a == "--gpus") gpus = std::atoi(v);
        else if (a == "--shard") shard = v;
        else if (a == "--json") json = std::atoi(v);
        else if (a == "--multi") multi = std::atoi(v);
        else if (a == "--staged") staged = std::atoi(v);
        else if (a == "--search") search_k = std::atoi(v);
        else if (a == "--seed") search_seed = std::strtoull(v, nullptr, 0);
        else if (a == "--count") search_count = std::strtoull(v, nullptr, 0);
        else if (a == "--out") outfile = v;
        else if (a == "--eye") eyefile = v;
        else if (a == "--spectrum") specfile = v;
        else if (a == "--nco") ncofile = v;
        else if (a == "--sinc") sincfile = v;
        else if (a == "--fcw") nco_fcw = std::strtoul(v, nullptr, 0);
        else if (a == "--am") nco_am = std::strtoul(v, nullptr, 0);
        else if (a == "--nco-samples") nco_samples = std::atof(v);
        else if (a == "--lags") lags = std::atoi(v), lags_set = true;
        else if (a == "--eye-samples") eye_samples = std::atof(v);
        else if (a == "--shape") shape = std::atoi(v);
        else if (a == "--shift") eye_shift = std::atoi(v);
        else if (a == "--tx-sweep") tx_sweep = std::atoi(v);
        else if (a == "--fir") fir = std::atoi(v);
        else if (a == "--dfe") dfe = std::atoi(v);
        else if (a == "--mlse") mlse = std::atoi(v);
        else if (a == "--timing") timing = std::atoi(v);
        else if (a == "--fec") fec = std::atoi(v);
        else if (a == "--rs") rs = std::atoi(v);
        else if (a == "--ldpc") ldpc = std::atoi(v);
        else if (a == "--sigma") rs_sigma = ldpc_sigma = std::atoi(v);
        else if (a == "--sync") sync_junk = std::atoi(v);
        else if (a == "--link") link = std::atoi(v);
        else if (a == "--delay") link_delay = std::atoi(v);
        else if (a == "--errstat") errstat = std::atoi(v);
        else if (a == "--xcorr") xcorr = std::atoi(v);
        else if (a == "--ddc") ddc = std::atoi(v);
        else if (a == "--carrier") carrier = std::atoi(v);
        else if (a == "--pm") nco_pm = std::atoi(v);
        else if (a == "--guard") errstat_guard = std::strtoul(v, nullptr, 0);
        else if (a == "--nv-range") {
            if (std::sscanf(v, "%d:%d", &nv_lo, &nv_hi) != 2) { std::fprintf(stderr, "--nv-range A:B\n"); return 2; }
        }
        else if (a == "--gen") { if (std::string(v) != "lutopt") { std::fprintf(stderr, "--gen lutopt is the only generator the reference has\n"); return 2; } }
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
    }
    if (argc % 2 == 0) { std::fprintf(stderr, "every option takes a value\n"); return 2; }
    if (bbb_abi_version() != BBB_ABI_VERSION) { std::fprintf(stderr, "ABI mismatch\n"); return 1; }
    int mode = BBB_SHARD_BITS;
    if (shard == "seeds") mode = BBB_SHARD_SEEDS;
    else if (shard == "trials") mode = BBB_SHARD_TRIALS;
    else if (shard == "groups") mode = BBB_SHARD_GROUPS;
    else if (shard != "bits") { std::fprintf(stderr, "--shard bits|seeds|trials|groups\n"); return 2; }
    if (seeds < 1 || init0 == 0 || gpus < 1 || step <= 0 || steps < 1) { std::fprintf(stderr, "bad --seeds / --init / --gpus / --step / --steps\n"); return 2; }
    int ndev_seen = 0;
    CHECK(bbb_device_count(&ndev_seen));
    if (gpus > ndev_seen) { std::fprintf(stderr, "--gpus %d but %d device(s) visible\n", gpus, ndev_seen); return 1; }

    // ---- the NCO's tone (gateware/bbb/nco.py; NCOTest, gateware/top.py:38-61, with fm held at 0) ----------------------------
    // Writes little-endian int16, the `<h` samples software/memdump reads.
    if (!ncofile.empty()) {
        if (nco_samples < 1 || nco_fcw >= (1ul << 24) || nco_am >= (1ul << 16)) {
            std::fprintf(stderr, "--nco-samples >= 1, --fcw < 2^24, --am < 2^16\n");
            return 2;
        }
        const uint64_t n = (uint64_t)nco_samples;
        const bbb_nco_cfg cfg = {(uint32_t)nco_fcw, (uint32_t)nco_am, 0, 0};
        bbb_nco *o = nullptr;
        int16_t *x = nullptr;
        CHECK(bbb_nco_open(&cfg, 0, nullptr, &o));
        if (hipMalloc((void **)&x, n * sizeof(int16_t)) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 1; }
        const double t0 = now_s();
        CHECK(bbb_nco_run(o, nullptr, nullptr, nullptr, n, x));
        bbb_nco_state st{};
        CHECK(bbb_nco_get_state(o, &st));
        const double dt = now_s() - t0;
        std::vector<int16_t> h(n);
        if (hipMemcpy(h.data(), x, n * sizeof(int16_t), hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        (void)hipFree(x);
        CHECK(bbb_nco_close(o));
        std::FILE *f = std::fopen(ncofile.c_str(), "wb");
        if (!f) { std::fprintf(stderr, "cannot write %s\n", ncofile.c_str()); return 1; }
        for (uint64_t i = 0; i < n; ++i) {
            const uint16_t u = (uint16_t)h[i];
            const unsigned char b[2] = {(unsigned char)(u & 0xFF), (unsigned char)(u >> 8)};
            std::fwrite(b, 1, 2, f);
        }
        std::fclose(f);
        std::printf("{\"mode\": \"nco\", \"samples\": %llu, \"fcw\": %lu, \"am\": %lu, \"pa\": %u, \"q\": %d, \"w\": %d, \"y\": %d, "
                    "\"seconds\": %.6f}\n", (unsigned long long)n, nco_fcw, nco_am, st.pa, st.q, st.w, st.y, dt);
        return 0;
    }

    // ---- the digital down-converter on the NCO's own tone: amplitude and phase come back ------------------------------------------
    if (ddc) {
        if (nco_samples < 128 || nco_samples > 4e9 || nco_fcw >= (1ul << 24) || nco_am >= (1ul << 16) || nco_pm < -512 || nco_pm >= 512) {
            std::fprintf(stderr, "--nco-samples 128..4e9, --fcw < 2^24, --am < 2^16, --pm in [-512, 512)\n");
            return 2;
        }
        const uint64_t n = (uint64_t)nco_samples;
        const bbb_nco_cfg cfg = {(uint32_t)nco_fcw, (uint32_t)nco_am, 0, nco_pm};
        bbb_nco *o = nullptr;
        int16_t *x = nullptr;
        uint32_t *pol = nullptr;                                           // (mag: uint16, phase: int16) per output
        CHECK(bbb_nco_open(&cfg, 0, nullptr, &o));
        bbb_fir_cfg fc{};
        fc.ntaps = 64;
        for (int i = 0; i < 64; ++i) fc.taps[i] = 1;
        fc.shift = 6, fc.decim = 64, fc.phase = 63;
        const bbb_ddc_cfg dc = {(uint32_t)nco_fcw, (uint32_t)((0x1000000ul - 3 * nco_fcw % 0x1000000ul) & 0xFFFFFFul), BBB_DDC_POLAR};
        const uint64_t nout_max = n / 64 + 1;
        if (hipMalloc((void **)&x, n * sizeof(int16_t)) != hipSuccess || hipMalloc((void **)&pol, nout_max * 4) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        uint64_t nout = 0;
        const double t0 = now_s();
        CHECK(bbb_nco_run(o, nullptr, nullptr, nullptr, n, x));
        CHECK(bbb_ddc_run(x, n, 0, 0, &dc, &fc, pol, &nout, 0, nullptr));
        if (hipDeviceSynchronize() != hipSuccess) { std::fprintf(stderr, "hipDeviceSynchronize failed\n"); return 1; }
        const double dt = now_s() - t0;
        std::vector<uint32_t> h(nout);
        if (hipMemcpy(h.data(), pol, nout * 4, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        (void)hipFree(x);
        (void)hipFree(pol);
        CHECK(bbb_nco_close(o));
        // output 0 still holds the oscillator's three samples of latency; the rest is the steady tone
        unsigned mag_lo = 65535, mag_hi = 0;
        int ph_lo = 32767, ph_hi = -32768;
        for (uint64_t q = 1; q < nout; ++q) {
            const unsigned m = h[q] & 0xFFFFu;
            const int ph = (int16_t)(h[q] >> 16);
            mag_lo = m < mag_lo ? m : mag_lo, mag_hi = m > mag_hi ? m : mag_hi;
            ph_lo = ph < ph_lo ? ph : ph_lo, ph_hi = ph > ph_hi ? ph : ph_hi;
        }
        std::printf("{\"mode\": \"ddc\", \"samples\": %llu, \"outputs\": %llu, \"fcw\": %lu, \"am\": %lu, \"pm\": %d, \"mag_min\": %u, "
                    "\"mag_max\": %u, \"phase_min\": %d, \"phase_max\": %d, \"seconds\": %.6f}\n", (unsigned long long)n,
                    (unsigned long long)nout, nco_fcw, nco_am, nco_pm, mag_lo, mag_hi, ph_lo, ph_hi, dt);
        return 0;
    }

    // ---- carrier recovery: the down-converter's tone with the two oscillators apart ------------------------------------------
    if (carrier) {
        if (nco_samples < 64 * 64 || nco_samples > 4e9 || nco_fcw >= (1ul << 24) || nco_fcw <= 4096 || nco_am >= (1ul << 16) || carrier < -4096 || carrier > 4096) {
            std::fprintf(stderr, "--nco-samples 4096..4e9, 4096 < --fcw < 2^24, --am < 2^16, --carrier in [-4096, 4096]\n");
            return 2;
        }
        const uint64_t nbits = (uint64_t)nco_samples / 64, n = nbits * 64;
        std::vector<uint8_t> data(nbits);
        std::vector<int16_t> pm(n);
        uint64_t lcg = 5;
        for (uint64_t b = 0; b < nbits; ++b) {
            lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
            data[b] = (uint8_t)(lcg >> 63);
            for (int i = 0; i < 64; ++i) pm[b * 64 + i] = data[b] ? -512 : 0;
        }
        const bbb_nco_cfg cfg = {(uint32_t)nco_fcw, (uint32_t)nco_am, 0, 0};
        const uint32_t rx_fcw = (uint32_t)((long)nco_fcw - carrier);
        bbb_fir_cfg fc{};
        fc.ntaps = 64;
        for (int i = 0; i < 64; ++i) fc.taps[i] = 1;
        fc.shift = 6, fc.decim = 64, fc.phase = 63;
        const bbb_ddc_cfg dc = {rx_fcw, (uint32_t)((0x1000000ul - 3ul * rx_fcw % 0x1000000ul) & 0xFFFFFFul), BBB_DDC_IQ16};
        const bbb_carrier_cfg cc = {32, 16384, 0, 0, 0};
        const uint64_t npairs = nbits - 1, nwords = (npairs + 31) / 32 * 32 / 64 + 1;
        bbb_nco *o = nullptr;
        int16_t *x = nullptr, *pmd = nullptr, *iq = nullptr;
        uint64_t *words = nullptr, *state = nullptr;                       // state[2] and stats[4] in one allocation
        CHECK(bbb_nco_open(&cfg, 0, nullptr, &o));
        if (hipMalloc((void **)&x, n * 2) != hipSuccess || hipMalloc((void **)&pmd, n * 2) != hipSuccess || hipMalloc((void **)&iq, npairs * 4) != hipSuccess ||
            hipMalloc((void **)&words, nwords * 8) != hipSuccess || hipMalloc((void **)&state, 48) != hipSuccess ||
            hipMemcpy(pmd, pm.data(), n * 2, hipMemcpyHostToDevice) != hipSuccess || hipMemset(state, 0, 48) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        uint64_t nout = 0;
        const double t0 = now_s();
        CHECK(bbb_nco_run(o, nullptr, nullptr, pmd, n, x));
        // the record is entered 3 samples late, the oscillator's latency, with those 3 as history: pair q is data bit q
        CHECK(bbb_ddc_run(x + 3, n - 3, 3, 3, &dc, &fc, iq, &nout, 0, nullptr));
        if (nout != npairs) { std::fprintf(stderr, "unexpected pair count\n"); return 1; }
        CHECK(bbb_carrier_run(iq, npairs, 1, &cc, state, nullptr, words, nullptr, nullptr, state + 2, 0, nullptr));
        if (hipDeviceSynchronize() != hipSuccess) { std::fprintf(stderr, "hipDeviceSynchronize failed\n"); return 1; }
        const double dt = now_s() - t0;
        std::vector<int16_t> hiq(2 * npairs);
        std::vector<uint64_t> hw(nwords), hs(6);
        if (hipMemcpy(hiq.data(), iq, npairs * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(hw.data(), words, nwords * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hs.data(), state, 48, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        (void)hipFree(x), (void)hipFree(pmd), (void)hipFree(iq), (void)hipFree(words), (void)hipFree(state);
        CHECK(bbb_nco_close(o));
        uint64_t before = 0, after = 0;
        for (uint64_t q = 0; q < npairs; ++q) {
            before += (hiq[2 * q + 1] > 0) != (data[q] != 0);
            after += ((hw[q >> 6] >> (q & 63)) & 1) != data[q];
        }
        const double offset = hs[2] ? (double)(int64_t)hs[5] / ((double)hs[2] * 32.0 * 65536.0) : 0.0;
        std::printf("{\"mode\": \"carrier\", \"samples\": %llu, \"bits\": %llu, \"fcw\": %lu, \"rx_fcw\": %u, \"errors_sign_of_q\": %llu, "
                    "\"errors_recovered\": %llu, \"blocks\": %llu, \"offset_turns_per_pair\": %.9f, \"ideal_offset\": %.9f, \"seconds\": %.6f}\n",
                    (unsigned long long)n, (unsigned long long)npairs, nco_fcw, rx_fcw, (unsigned long long)before, (unsigned long long)after,
                    (unsigned long long)hs[2], offset, carrier * 64.0 / 16777216.0, dt);
        return 0;
    }

    // ---- how the detector's errors are distributed (the reference's own detector test injects isolated errors and a burst,
    // gateware/bbb/prbs.py:129-138) ------------------------------------------------------------------------------------------
    if (errstat) {
        if (bits < 1024 || bits > 1e11 || errstat_guard >= (1ull << 32)) { std::fprintf(stderr, "--bits 1024..1e11, --guard < 2^32\n"); return 2; }
        const uint64_t n = (uint64_t)bits, nw = (n + 63) / 64;
        uint64_t *buf = nullptr, *err = nullptr, *rl = nullptr;
        if (hipMalloc((void **)&buf, nw * 8) != hipSuccess || hipMalloc((void **)&err, nw * 8) != hipSuccess ||
            hipMalloc((void **)&rl, nw * 8) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        CHECK(bbb_prbs_fill(k, 1, 0, n, buf, 0, nullptr));
        // flips: one word at a time through the host (a handful of words; the stream itself stays on the device)
        std::vector<uint64_t> flips;
        for (uint64_t t = 4096; t < n; t += 99991) flips.push_back(t);
        for (uint64_t t = n / 2; t < n / 2 + 3 * (uint64_t)k && t < n; ++t) flips.push_back(t);
        for (uint64_t t : flips) {
            uint64_t w = 0;
            if (hipMemcpy(&w, buf + t / 64, 8, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
            w ^= 1ull << (t % 64);
            if (hipMemcpy(buf + t / 64, &w, 8, hipMemcpyHostToDevice) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        }
        const bbb_errstat_cfg cfg = {(uint32_t)errstat_guard, 4, {1000, 10000, 100000, 1000000}};
        bbb_errstat *e = nullptr;
        CHECK(bbb_errstat_open(&cfg, 0, nullptr, &e));
        bbb_detector_stats ds{};
        const double t0 = now_s();
        CHECK(bbb_prbs_detector_stream(k, buf, n, err, rl, &ds, 0, 0, 0, nullptr));
        const double t1 = now_s();
        CHECK(bbb_errstat_accumulate(e, err, rl, n));
        std::vector<bbb_errstat_result> rv(1);
        bbb_errstat_result &r = rv[0];
        CHECK(bbb_errstat_read(e, &r));
        const double t2 = now_s();
        CHECK(bbb_errstat_close(e));
        (void)hipFree(buf);
        (void)hipFree(err);
        (void)hipFree(rl);
        // the burst still open at the end of the data counts as a burst here
        unsigned long long bursts = r.bursts, len_sum = r.burst_len_sum, max_len = r.max_burst_len, max_w = r.max_burst_weight;
        if (r.open_weight) {
            const unsigned long long len = r.open_last - r.open_first + 1;
            ++bursts;
            len_sum += len;
            if (len > max_len) max_len = len;
            if (r.open_weight > max_w) max_w = r.open_weight;
        }
        unsigned long long isolated = r.burst_weight_hist[1] + (r.open_weight == 1 ? 1 : 0);
        std::printf("{\"mode\": \"errstat\", \"prbs\": %d, \"bits\": %llu, \"flipped\": %llu, \"guard\": %lu, \"errors\": %llu, "
                    "\"errors_raw\": %llu, \"resyncs\": %llu, \"first_error\": %llu, \"last_error\": %llu, \"max_gap\": %llu, "
                    "\"bursts\": %llu, \"isolated\": %llu, \"mean_burst_len\": %.3f, \"max_burst_len\": %llu, \"max_burst_weight\": %llu, "
                    "\"block_bits\": [1000, 10000, 100000, 1000000], \"errored_blocks\": [%llu, %llu, %llu, %llu], "
                    "\"detector_seconds\": %.6f, \"errstat_seconds\": %.6f}\n",
                    k, (unsigned long long)r.bits, (unsigned long long)flips.size(), errstat_guard, (unsigned long long)r.errors,
                    (unsigned long long)ds.errors_raw, (unsigned long long)ds.resyncs, (unsigned long long)r.first_error,
                    (unsigned long long)r.last_error, (unsigned long long)r.max_gap, bursts, isolated,
                    bursts ? (double)len_sum / (double)bursts : 0.0, max_len, max_w, (unsigned long long)r.errored_blocks[0],
                    (unsigned long long)r.errored_blocks[1], (unsigned long long)r.errored_blocks[2],
                    (unsigned long long)r.errored_blocks[3], t1 - t0, t2 - t1);
        if (r.errors != ds.errors) { std::fprintf(stderr, "the statistics count %llu errors, the detector %llu\n", (unsigned long long)r.errors, (unsigned long long)ds.errors); return 1; }
        return 0;
    }

    // ---- matrix search (software/rnghunt/src/bin/rnghunt.rs:13-66) -------------------------------------------------------
    if (search_k > 0) {
        if (outfile.empty()) { std::fprintf(stderr, "--search K needs --out FILE\n"); return 2; }
        std::vector<uint16_t> taps((size_t)search_k * 4);
        std::vector<uint32_t> off((size_t)search_k + 1);
        uint64_t found = ~0ull, first = 0, tested = 0, full = 0;
        double kernel_ms = 0;
        const double t0 = now_s();
        while (found == ~0ull) {                       // the reference's workers loop until one reports a hit (rnghunt.rs:23-57)
            bbb_search_stats st{};
            CHECK(bbb_lutopt_search(search_k, search_seed, first, search_count, &found, taps.data(), off.data(), &st, 0, nullptr));
            tested += st.tested; full += st.full_degree; kernel_ms += (double)st.kernel_ns * 1e-6;
            first += search_count;
            if (first > (1ull << 40)) { std::fprintf(stderr, "no matrix among 2^40 candidates\n"); return 1; }
        }
        CHECK(bbb_lutopt_save_matrix_file(outfile.c_str(), search_k, taps.data(), off.data()));      // rnghunt.rs:51-53
        int k2 = 0, ok = 0;
        uint16_t *t2 = nullptr;
        uint32_t *o2 = nullptr;
        CHECK(bbb_lutopt_load_matrix_file(outfile.c_str(), &k2, &t2, &o2));                              // what --matrix reads
        CHECK(bbb_lutopt_is_full_period(k2, t2, o2, &ok));
        bbb_free(t2);
        bbb_free(o2);
        std::printf("{\"mode\": \"search\", \"k\": %d, \"seed\": %llu, \"candidate\": %llu, \"tested\": %llu, \"full_degree\": %llu, "
                    "\"kernel_ms\": %.3f, \"seconds\": %.3f, \"out\": \"%s\", \"reloaded_k\": %d, \"full_period\": %s}\n",
                    search_k, search_seed, (unsigned long long)found, (unsigned long long)tested, (unsigned long long)full, kernel_ms, now_s() - t0,
                    outfile.c_str(), k2, ok ? "true" : "false");
        return ok && k2 == search_k ? 0 : 1;
    }

    Matrix m;
    if (matrix.empty()) {
        const char *here = std::getenv("BBB_DATA");
        const std::string path = std::string(here ? here : "basebandboard_amd/data") + "/lutopt_256.taps";
        if (!load_taps_file(path, &m.n, &m.taps, &m.off)) { std::fprintf(stderr, "cannot read %s (set BBB_DATA)\n", path.c_str()); return 1; }
    } else {
        uint16_t *t = nullptr;
        uint32_t *o = nullptr;
        CHECK(bbb_lutopt_load_matrix_file(matrix.c_str(), &m.n, &t, &o));
        m.taps.assign(t, t + o[m.n]);
        m.off.assign(o, o + m.n + 1);
        bbb_free(t);
        bbb_free(o);
    }

    // seed d of the run = the reset state advanced 2^48 d clocks (host-side GF(2) jump-ahead on a device -1 handle)
    auto seed_words = [&](int d, uint64_t (&w)[8]) -> int {
        const uint64_t base[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 8; i++) w[i] = base[i];
        if (d == 0) return BBB_OK;
        bbb_lutopt *hh = nullptr;
        int rc = bbb_lutopt_create(&hh, m.n, m.taps.data(), m.off.data(), base, -1);
        if (rc) return rc;
        rc = bbb_lutopt_state_at(hh, (uint64_t)d << 48, w);
        (void)bbb_lutopt_destroy(hh);
        return rc;
    };

    // ---- the generator's evaluation (software/clt-grng/clt-grng-evaluate.py:18-31) over any number of samples ------------------
    if (grng_eval >= 1) {
        const uint64_t n = (uint64_t)grng_eval, chunk = 1ull << 34;
        if (m.n < 2 || m.n > 512 || (m.n & (m.n - 1))) { std::fprintf(stderr, "--grng-eval needs a power-of-two matrix up to 512\n"); return 2; }
        const uint64_t init[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        bbb_lutopt *h = nullptr;
        CHECK(bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, 0));
        const size_t nb = (size_t)m.n;
        uint64_t *d = nullptr;
        if (hipMalloc((void **)&d, nb * sizeof(uint64_t)) != hipSuccess || hipMemset(d, 0, nb * sizeof(uint64_t)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        const double t0 = now_s();
        for (uint64_t off = 0; off < n; off += chunk)               // the calls add into the same counters
            CHECK(bbb_awgn_hist(h, d, n - off < chunk ? n - off : chunk, first_step + off));
        std::vector<uint64_t> c(nb);
        if (hipMemcpy(c.data(), d, nb * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        const double ms = (now_s() - t0) * 1e3;
        CHECK(bbb_lutopt_destroy(h));
        (void)hipFree(d);
        // bin b holds the sample b - n/2; sums in long double, the two lines in double as the reference prints them
        long double total = 0, s1 = 0, s2 = 0;
        int lo = -1, hi = -1;
        for (size_t b = 0; b < nb; b++) {
            if (!c[b]) continue;
            const long double x = (long double)b - (long double)(nb / 2);
            total += (long double)c[b];
            s1 += x * (long double)c[b];
            s2 += x * x * (long double)c[b];
            if (lo < 0) lo = (int)b;
            hi = (int)b;
        }
        const double mean = (double)(s1 / total), var = (double)(s2 / total - (s1 / total) * (s1 / total));
        std::printf("Theoretical mean \u03bc=%.4e, variance \u03c3\u00b2=%.4e.\n", 0.0, (double)m.n / 4);
        std::printf("Sample mean \u03bc=%.4e, variance \u03c3\u00b2=%.4e.\n", mean, var);
        std::printf("{\"mode\": \"grng_eval\", \"n\": %d, \"first_step\": %llu, \"total\": %llu, \"min_bin\": %d, \"max_bin\": %d, "
                    "\"min_sample\": %d, \"max_sample\": %d, \"elapsed_ms\": %.3f}\n", m.n, first_step, (unsigned long long)total, lo, hi,
                    lo - (int)(nb / 2), hi - (int)(nb / 2), ms);
        return 0;
    }

    // ---- eye diagram and bathtub of the transmitter (gateware/bbb/dso.py, drawn by ui.py) -------------------------------
    if (!eyefile.empty()) {
        if (shape < 0 || shape > 31 || eye_samples < 1) { std::fprintf(stderr, "--shape 0..31, --eye-samples >= 1\n"); return 2; }
        bbb_tx_cfg cfg{};
        rcf_taps(shape == 31 ? 1.0 : shape * (1.0 / 31), cfg.coeffs);          // tx.py:54: np.linspace(0, 1, 32)
        cfg.source = 0;
        cfg.prbs_k = k;
        cfg.prbs_state = 1;
        cfg.bit_en = 1;
        cfg.noise_en = 1;
        cfg.noise_var = nv;
        cfg.warmup = 16;
        const bbb_eye_cfg eye{64, (uint32_t)eye_shift, BBB_TX_BIT_SAMPLE0, 0, 0};
        const uint64_t init[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        bbb_lutopt *h = nullptr;
        CHECK(bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, 0));
        bbb_tx_eye *e = nullptr;
        CHECK(bbb_tx_eye_open(h, &cfg, &eye, 0, &e));
        const size_t nh = 256 * 64, nw = nh + 16;
        uint64_t *d = nullptr;
        if (hipMalloc((void **)&d, nw * sizeof(uint64_t)) != hipSuccess || hipMemset(d, 0, nw * sizeof(uint64_t)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        const double t0 = now_s();
        CHECK(bbb_tx_eye_run(e, 0, (uint64_t)eye_samples, d, d + nh));
        std::vector<uint64_t> out(nw);
        if (hipMemcpy(out.data(), d, nw * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        const double secs = now_s() - t0;
        CHECK(bbb_tx_eye_close(e));
        CHECK(bbb_lutopt_destroy(h));
        (void)hipFree(d);
        FILE *f = std::fopen(eyefile.c_str(), "wb");
        if (!f) { std::fprintf(stderr, "cannot write %s\n", eyefile.c_str()); return 1; }
        std::fprintf(f, "P5\n64 256\n255\n");                               // the DSO's memory image: row << 6 | col
        std::vector<unsigned char> img(nh);
        for (size_t i = 0; i < nh; i++) img[i] = out[i] ? 255 : 0;
        const bool ok = std::fwrite(img.data(), 1, nh, f) == nh;
        if (std::fclose(f) != 0 || !ok) { std::fprintf(stderr, "cannot write %s\n", eyefile.c_str()); return 1; }
        std::printf("{\"mode\": \"eye\", \"samples\": %llu, \"prbs\": %d, \"nv\": %d, \"shape\": %d, \"shift\": %d, \"seconds\": %.4f, "
                    "\"pgm\": \"%s\", \"taps\": [", (unsigned long long)eye_samples, k, nv, shape, eye_shift, secs, eyefile.c_str());
        for (int i = 0; i < 64; i++) std::printf("%s%d", i ? ", " : "", cfg.coeffs[i]);
        std::printf("]}\n");
        for (int p = 0; p < 8; p++) {
            const uint64_t nb = out[nh + 2 * p], ne = out[nh + 2 * p + 1];
            std::printf("{\"phase\": %d, \"bits\": %llu, \"errors\": %llu, \"ber\": %.6e}\n", p, (unsigned long long)nb,
                        (unsigned long long)ne, nb ? (double)ne / (double)nb : 0.0);
        }
        return 0;
    }

    // ---- the scope's sinc interpolator (gateware/bbb/sinc.py) ---------------------------------------------------------------
    if (!sincfile.empty()) {
        if (shape < 0 || shape > 31 || eye_samples < 1 || eye_shift < 0 || eye_shift > 15) {
            std::fprintf(stderr, "--shape 0..31, --eye-samples >= 1, --shift 0..15\n");
            return 2;
        }
        // the module's batch: 72 samples of a 7-cycle sine (gateware/bbb/tests/test_sinc.py:22), outputs y[109 .. 1132]
        int8_t x[72];
        for (int i = 0; i < 72; i++) x[i] = (int8_t)(std::sin(2.0 * M_PI * 7.0 * (i == 71 ? 1.0 : i * (1.0 / 71.0))) * 127.0);
        int8_t *xd = nullptr, *yd = nullptr;
        if (hipMalloc((void **)&xd, sizeof x) != hipSuccess || hipMalloc((void **)&yd, 72 * BBB_SINC_UP) != hipSuccess ||
            hipMemcpy(xd, x, sizeof x, hipMemcpyHostToDevice) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        const bbb_sinc_cfg c8{1, 1, 0};
        CHECK(bbb_sinc_interpolate(xd, 72, 0, &c8, yd, 0, nullptr));
        int8_t y[72 * BBB_SINC_UP];
        if (hipMemcpy(y, yd, sizeof y, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        (void)hipFree(xd);
        (void)hipFree(yd);
        std::printf("{\"mode\": \"sinc\", \"batch\": [");
        for (int i = 0; i < 1024; i++) std::printf("%s%d", i ? ", " : "", y[109 + i]);
        std::printf("]}\n");
        // a capture at 4 samples per bit: every second sample of the transmitter's waveform (8 per bit), interpolated 16x
        bbb_tx_cfg cfg{};
        rcf_taps(shape == 31 ? 1.0 : shape * (1.0 / 31), cfg.coeffs);
        cfg.source = 0;
        cfg.prbs_k = k;
        cfg.prbs_state = 1;
        cfg.bit_en = 1;
        cfg.noise_en = 1;
        cfg.noise_var = nv;
        cfg.warmup = 16;
        const uint64_t init[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        bbb_lutopt *h = nullptr;
        CHECK(bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, 0));
        const uint64_t ntx = (uint64_t)eye_samples & ~1ull, ncap = ntx / 2;
        const size_t nh = 256 * 64;
        int16_t *w = nullptr;
        uint64_t *d = nullptr;
        if (hipMalloc((void **)&w, (ntx + 8) * sizeof(int16_t)) != hipSuccess || hipMalloc((void **)&d, nh * sizeof(uint64_t)) != hipSuccess ||
            hipMemset(d, 0, nh * sizeof(uint64_t)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        CHECK(bbb_tx_fill_i16(h, &cfg, w, ntx, 0));
        std::vector<int16_t> tx(ntx), cap(ncap);
        if (hipMemcpy(tx.data(), w, ntx * sizeof(int16_t), hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        for (uint64_t i = 0; i < ncap; i++) cap[i] = tx[2 * i];
        if (hipMemcpy(w, cap.data(), ncap * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        // transmitter sample 2i is captured sample i: bit m peaks at sample 8m + 49, interpolated sample 64m + 392
        const bbb_sinc_cfg c16{2, 2, (uint32_t)eye_shift};
        const bbb_eye_cfg eye{64, 0, 392 - 32, 0, 0};
        bbb_sinc_eye *e = nullptr;
        CHECK(bbb_sinc_eye_open(&c16, &eye, 0, 0, nullptr, &e));
        const double t0 = now_s();
        CHECK(bbb_sinc_eye_run(e, w, ncap, 0, 0, d));
        std::vector<uint64_t> out(nh);
        if (hipMemcpy(out.data(), d, nh * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        const double secs = now_s() - t0;
        CHECK(bbb_sinc_eye_close(e));
        CHECK(bbb_lutopt_destroy(h));
        (void)hipFree(w);
        (void)hipFree(d);
        FILE *f = std::fopen(sincfile.c_str(), "wb");
        if (!f) { std::fprintf(stderr, "cannot write %s\n", sincfile.c_str()); return 1; }
        std::fprintf(f, "P5\n64 256\n255\n");
        std::vector<unsigned char> img(nh);
        uint64_t total = 0;
        for (size_t i = 0; i < nh; i++) { img[i] = out[i] ? 255 : 0; total += out[i]; }
        const bool ok = std::fwrite(img.data(), 1, nh, f) == nh;
        if (std::fclose(f) != 0 || !ok) { std::fprintf(stderr, "cannot write %s\n", sincfile.c_str()); return 1; }
        std::printf("{\"mode\": \"sinc-eye\", \"captured\": %llu, \"interpolated\": %llu, \"prbs\": %d, \"nv\": %d, \"shape\": %d, "
                    "\"shift\": %d, \"seconds\": %.4f, \"pgm\": \"%s\"}\n", (unsigned long long)ncap, (unsigned long long)total, k, nv,
                    shape, eye_shift, secs, sincfile.c_str());
        return 0;
    }

    // ---- the moving-average receiver (gateware/bbb/average.py, rx.py:24-26) beside the plain slicer ---------------------------
    if (fir) {
        if (eye_samples < 1 || nv < 0 || nv > 15) { std::fprintf(stderr, "--eye-samples >= 1, --nv 0..15\n"); return 2; }
        bbb_tx_cfg cfg{};
        for (int i = 30; i < 34; i++) cfg.coeffs[i] = 254;          // the rectangular pulse (bitshaper.py:108)
        cfg.source = 0;
        cfg.prbs_k = k;
        cfg.prbs_state = 1;
        cfg.bit_en = 1;
        cfg.noise_en = 1;
        cfg.noise_var = nv;
        cfg.warmup = 16;
        const uint64_t init[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        bbb_lutopt *h = nullptr;
        CHECK(bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, 0));
        const uint64_t ntx = (uint64_t)eye_samples;
        int16_t *w = nullptr;
        uint64_t *b = nullptr;
        if (hipMalloc((void **)&w, ntx * sizeof(int16_t)) != hipSuccess || hipMalloc((void **)&b, (ntx / 8 / 64 + 2) * sizeof(uint64_t)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        CHECK(bbb_tx_fill_i16(h, &cfg, w, ntx, 0));
        // bit m holds samples 8m + 47 .. 8m + 50: the plain slicer looks at 8m + 48, the running sum of four is complete at 8m + 50
        uint64_t nplain = 0, nfilt = 0;
        bbb_detector_stats plain{}, filt{};
        const double t0 = now_s();
        CHECK(bbb_rx_slice(w, ntx, 8, 0, 0, b, &nplain, 0, nullptr));
        CHECK(bbb_prbs_detector_stream(k, b, nplain, nullptr, nullptr, &plain, 0, 0, 0, nullptr));
        bbb_fir_cfg fc;
        CHECK(bbb_fir_moving_average(&fc, 0));
        fc.decim = 8;
        fc.phase = 2;
        CHECK(bbb_fir_slice(w, ntx, 0, &fc, 0, 0, b, &nfilt, 0, nullptr));
        CHECK(bbb_prbs_detector_stream(k, b, nfilt, nullptr, nullptr, &filt, 0, 0, 0, nullptr));
        const double secs = now_s() - t0;
        CHECK(bbb_lutopt_destroy(h));
        (void)hipFree(w);
        (void)hipFree(b);
        std::printf("{\"mode\": \"fir\", \"samples\": %llu, \"prbs\": %d, \"nv\": %d, \"plain\": {\"phase\": 0, \"bits\": %llu, \"errors\": %llu, "
                    "\"reload_clocks\": %llu}, \"moving_average\": {\"phase\": 2, \"bits\": %llu, \"errors\": %llu, \"reload_clocks\": %llu}, "
                    "\"seconds\": %.4f}\n", (unsigned long long)ntx, k, nv, (unsigned long long)plain.bits, (unsigned long long)plain.errors,
                    (unsigned long long)plain.reload_clocks, (unsigned long long)filt.bits, (unsigned long long)filt.errors,
                    (unsigned long long)filt.reload_clocks, secs);
        return 0;
    }

    // ---- forward error correction: the K = 7 code around a noisy two-level link, hard against soft decisions (bbb_conv_*) --------
    if (fec) {
        static const uint32_t keeps[8][2] = {{0, 0}, {1, 1}, {1, 3}, {5, 3}, {0, 0}, {21, 11}, {0, 0}, {81, 47}};
        if (eye_samples < 1 || nv < 0 || nv > 15 || fec > 7 || fec < 0 || !keeps[fec][0]) {
            std::fprintf(stderr, "--eye-samples >= 1, --nv 0..15, --fec 1, 2, 3, 5 or 7\n");
            return 2;
        }
        bbb_conv_cfg cc{};
        cc.K = 7, cc.n = 2, cc.gen[0] = 0171, cc.gen[1] = 0133;
        cc.period = (uint32_t)fec, cc.keep[0] = keeps[fec][0], cc.keep[1] = keeps[fec][1];
        const uint64_t nbits = (uint64_t)eye_samples;
        uint64_t ntx = 0;
        uint64_t *data = nullptr, *tx = nullptr, *hard = nullptr, *dec = nullptr;
        int16_t *soft = nullptr;
        const uint64_t max_tx = 2 * nbits;
        if (hipMalloc((void **)&data, (nbits / 64 + 1) * 8) != hipSuccess || hipMalloc((void **)&tx, (max_tx / 64 + 1) * 8) != hipSuccess ||
            hipMalloc((void **)&hard, (max_tx / 64 + 1) * 8) != hipSuccess || hipMalloc((void **)&dec, (nbits / 64 + 1) * 8) != hipSuccess ||
            hipMalloc((void **)&soft, max_tx * sizeof(int16_t)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        CHECK(bbb_prbs_fill(k, 1, 0, nbits, data, 0, nullptr));
        const double t0 = now_s();
        CHECK(bbb_conv_encode(data, nbits, 0, &cc, nullptr, tx, &ntx, 0, nullptr));
        std::vector<uint64_t> txh((size_t)(ntx + 63) / 64);
        if (hipMemcpy(txh.data(), tx, txh.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        std::vector<int16_t> x((size_t)ntx);
        std::mt19937_64 gen(26);
        std::normal_distribution<double> noise(0.0, 5.0 * nv);
        for (uint64_t i = 0; i < ntx; ++i) x[(size_t)i] = (int16_t)((txh[(size_t)(i >> 6)] >> (i & 63) & 1 ? 64 : -64) + std::lrint(noise(gen)));
        if (hipMemcpy(soft, x.data(), ntx * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        uint64_t nhard = 0, nd_hard = 0, nd_soft = 0, e_hard = 0, e_soft = 0, e_channel = 0;
        CHECK(bbb_rx_slice(soft, ntx, 1, 0, 0, hard, &nhard, 0, nullptr));
        CHECK(bbb_conv_decode(hard, 0, nhard, 0, 0, 1, BBB_CONV_HARD, &cc, dec, nullptr, &nd_hard, 0, nullptr));
        CHECK(bbb_prbs_check(k, 1, 0, nd_hard, dec, &e_hard, 0, nullptr));
        CHECK(bbb_conv_decode(soft, 0, ntx, 0, 0, 1, BBB_CONV_SOFT16, &cc, dec, nullptr, &nd_soft, 0, nullptr));
        CHECK(bbb_prbs_check(k, 1, 0, nd_soft, dec, &e_soft, 0, nullptr));
        const double secs = now_s() - t0;
        for (uint64_t i = 0; i < ntx; ++i) e_channel += (uint64_t)((x[(size_t)i] >= 0) != (bool)(txh[(size_t)(i >> 6)] >> (i & 63) & 1));
        (void)hipFree(data);
        (void)hipFree(tx);
        (void)hipFree(hard);
        (void)hipFree(dec);
        (void)hipFree(soft);
        std::printf("{\"mode\": \"fec\", \"bits\": %llu, \"prbs\": %d, \"gen\": [\"0171\", \"0133\"], \"period\": %d, \"keep\": [%u, %u], \"sigma\": %d, "
                    "\"coded_bits\": %llu, \"channel_errors\": %llu, \"hard\": {\"bits\": %llu, \"errors\": %llu}, \"soft\": {\"bits\": %llu, \"errors\": %llu}, "
                    "\"seconds\": %.4f}\n", (unsigned long long)nbits, k, fec, cc.keep[0], cc.keep[1], 5 * nv, (unsigned long long)ntx,
                    (unsigned long long)e_channel, (unsigned long long)nd_hard, (unsigned long long)e_hard, (unsigned long long)nd_soft,
                    (unsigned long long)e_soft, secs);
        return 0;
    }

    // ---- the LDPC codec: encode, noise, decode, counts (bbb_ldpc_*) ---------------------------------------------------------------------
    if (ldpc) {
        bool prime = ldpc >= 17 && ldpc <= 512 && (ldpc & 1);
        for (int d = 3; prime && d * d <= ldpc; d += 2) prime = ldpc % d != 0;
        if (ldpc_sigma == -1) ldpc_sigma = 32;
        const uint32_t Z = (uint32_t)ldpc, J = 4, K = 16;
        const uint64_t kbits = (uint64_t)(K - J) * Z, nbitsw = (uint64_t)K * Z, ncw = eye_samples < 1 || !prime ? 0 : (uint64_t)eye_samples / kbits;
        if (!prime || ldpc_sigma < 0 || ldpc_sigma > 200 || ncw < 1) {
            std::fprintf(stderr, "--ldpc P with P an odd prime 17..512, --sigma 0..200, --eye-samples at least one codeword of 12 P bits\n");
            return 2;
        }
        bbb_ldpc_cfg lc{};
        lc.Z = Z, lc.J = J, lc.K = K, lc.max_iter = 20, lc.norm = 12;
        for (uint32_t j = 0; j < J; ++j) {
            for (uint32_t c = 0; c < K - J; ++c) lc.base[j * K + c] = (int16_t)(j * (c + J - j) % Z);
            for (uint32_t i = 0; i < J; ++i) lc.base[j * K + K - J + i] = (int16_t)(i >= j ? j * (i - j) % Z : -1);
        }
        const uint64_t ndata = ncw * kbits, ncoded = ncw * nbitsw;
        uint64_t *data = nullptr, *coded = nullptr, *out = nullptr, *stats = nullptr, e_data = 0, e_channel = 0;
        int16_t *soft = nullptr;
        if (hipMalloc((void **)&data, (ndata / 64 + 1) * 8) != hipSuccess || hipMalloc((void **)&coded, (ncoded / 64 + 1) * 8) != hipSuccess ||
            hipMalloc((void **)&out, (ndata / 64 + 1) * 8) != hipSuccess || hipMalloc((void **)&stats, BBB_LDPC_NSTATS * 8) != hipSuccess ||
            hipMalloc((void **)&soft, ncoded * sizeof(int16_t)) != hipSuccess || hipMemset(stats, 0, BBB_LDPC_NSTATS * 8) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        CHECK(bbb_prbs_fill(k, 1, 0, ndata, data, 0, nullptr));
        const double t0 = now_s();
        CHECK(bbb_ldpc_encode(data, ncw, &lc, coded, 0, nullptr));
        std::vector<uint64_t> txh((size_t)(ncoded + 63) / 64);
        if (hipMemcpy(txh.data(), coded, txh.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        std::vector<int16_t> x((size_t)ncoded);
        std::mt19937_64 gen(44);
        std::normal_distribution<double> noise(0.0, (double)ldpc_sigma);
        for (uint64_t i = 0; i < ncoded; ++i) {
            const bool b = txh[(size_t)(i >> 6)] >> (i & 63) & 1;
            x[(size_t)i] = (int16_t)((b ? 64 : -64) + std::lrint(noise(gen)));
            e_channel += (uint64_t)((x[(size_t)i] > 0) != b);
        }
        if (hipMemcpy(soft, x.data(), ncoded * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        CHECK(bbb_ldpc_decode(soft, 0, ncw, BBB_CONV_SOFT16, &lc, out, nullptr, stats, 0, nullptr));
        CHECK(bbb_prbs_check(k, 1, 0, ndata, out, &e_data, 0, nullptr));
        uint64_t st[BBB_LDPC_NSTATS];
        if (hipMemcpy(st, stats, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        const double secs = now_s() - t0;
        for (void *p : {(void *)data, (void *)coded, (void *)out, (void *)stats, (void *)soft}) (void)hipFree(p);
        std::printf("{\"mode\": \"ldpc\", \"code\": \"array(%d,4,16)\", \"n\": %llu, \"k\": %llu, \"codewords\": %llu, \"data_bits\": %llu, \"prbs\": %d, "
                    "\"sigma\": %d, \"coded_bits\": %llu, \"channel_errors\": %llu, \"data_errors\": %llu, \"clean\": %llu, \"failed\": %llu, "
                    "\"iterations\": %llu, \"bits_corrected\": %llu, \"seconds\": %.4f}\n", ldpc, (unsigned long long)nbitsw, (unsigned long long)kbits,
                    (unsigned long long)st[0], (unsigned long long)ndata, k, ldpc_sigma, (unsigned long long)ncoded, (unsigned long long)e_channel,
                    (unsigned long long)e_data, (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3], (unsigned long long)st[4], secs);
        return 0;
    }

    // ---- the concatenated code: Reed-Solomon around the K = 7 code, the closed loop through the C ABI (bbb_rs_*, bbb_conv_*) -----------
    if (rs) {
        bbb_rs_cfg rc{};
        rc.prim_poly = 0x187, rc.fcr = 112, rc.prim = 11, rc.nroots = 32, rc.n = 255, rc.depth = (uint32_t)rs;
        const uint64_t fdata = 223ull * (uint64_t)(rs > 0 ? rs : 1), fcoded = 255ull * (uint64_t)(rs > 0 ? rs : 1);
        const uint64_t nframes = eye_samples < 1 ? 0 : (uint64_t)eye_samples / (8 * fdata);
        if (rs < 1 || rs > 8 || rs_sigma < 0 || rs_sigma > 200 || nframes < 1 || sync_junk < -1 || sync_junk > (1 << 20)) {
            std::fprintf(stderr, "--rs 1..8, --sigma 0..200, --eye-samples at least one frame of 1784 I bits, --sync 0..2^20\n");
            return 2;
        }
        bbb_conv_cfg cc{};
        cc.K = 7, cc.n = 2, cc.gen[0] = 0171, cc.gen[1] = 0133, cc.period = 1, cc.keep[0] = cc.keep[1] = 1;
        const bool sync = sync_junk >= 0;
        bbb_framesync_cfg fc{};
        fc.marker = 0x1DFCCF1A, fc.marker_bits = 32, fc.frame_bits = 32 + 8 * (uint32_t)fcoded, fc.tol_search = 2, fc.tol_lock = 6, fc.verify = 1;
        fc.flywheel = 2, fc.both_polarities = 1, fc.rand_poly = 0x1A9, fc.rand_seed = 0xFF;
        // ncoded: the bits that go into the convolutional encoder: the coded frames, or the junk and the marked frames
        const uint64_t nbits = nframes * fdata * 8, nplain = nframes * fcoded * 8, ncoded = sync ? (uint64_t)sync_junk + nframes * fc.frame_bits : nplain;
        uint64_t ntx = 0, nhard = 0, nd = 0, e_viterbi = 0, e_data = 0, e_channel = 0;
        uint64_t *data = nullptr, *coded = nullptr, *tx = nullptr, *hard = nullptr, *dec = nullptr, *out = nullptr, *stats = nullptr;
        int16_t *soft = nullptr;
        if (hipMalloc((void **)&data, (nbits / 64 + 1) * 8) != hipSuccess || hipMalloc((void **)&coded, (ncoded / 64 + 1) * 8) != hipSuccess ||
            hipMalloc((void **)&tx, (2 * ncoded / 64 + 1) * 8) != hipSuccess || hipMalloc((void **)&hard, (2 * ncoded / 64 + 1) * 8) != hipSuccess ||
            hipMalloc((void **)&dec, (ncoded / 64 + 1) * 8) != hipSuccess || hipMalloc((void **)&out, (nbits / 64 + 1) * 8) != hipSuccess ||
            hipMalloc((void **)&stats, BBB_RS_NSTATS * 8) != hipSuccess ||
            hipMalloc((void **)&soft, 2 * ncoded * sizeof(int16_t)) != hipSuccess || hipMemset(stats, 0, BBB_RS_NSTATS * 8) != hipSuccess ||
            hipMemset(coded, 0, (ncoded / 64 + 1) * 8) != hipSuccess || hipMemset(out, 0, (nbits / 64 + 1) * 8) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        CHECK(bbb_prbs_fill(k, 1, 0, nbits, data, 0, nullptr));
        const double t0 = now_s();
        std::mt19937_64 gen(43);
        uint64_t *frames = nullptr, *fstate = nullptr, *fpos = nullptr, *fscratch = nullptr;
        uint16_t *fmeta = nullptr;
        bbb_framesync_plan_out plan{};
        if (!sync) {
            CHECK(bbb_rs_encode((const uint8_t *)data, nframes, &rc, (uint8_t *)coded, 0, nullptr));
        } else {
            CHECK(bbb_framesync_plan(ncoded, &fc, &plan));
            if (hipMalloc((void **)&frames, (nplain / 64 + 1) * 8) != hipSuccess || hipMalloc((void **)&fstate, BBB_FRAMESYNC_NSTATE * 8) != hipSuccess ||
                hipMalloc((void **)&fpos, (nframes + 1) * 8) != hipSuccess || hipMalloc((void **)&fmeta, (nframes + 1) * 2) != hipSuccess ||
                hipMalloc((void **)&fscratch, plan.scratch_bytes) != hipSuccess || hipMemset(fstate, 0, BBB_FRAMESYNC_NSTATE * 8) != hipSuccess) {
                std::fprintf(stderr, "hipMalloc failed\n");
                return 1;
            }
            // RS-encode into `frames`, attach into `dec` (free until the decoder runs), then junk in front on the host
            CHECK(bbb_rs_encode((const uint8_t *)data, nframes, &rc, (uint8_t *)frames, 0, nullptr));
            CHECK(bbb_frame_attach((const uint8_t *)frames, nframes, &fc, dec, 0, nullptr));
            const uint64_t nmarked = nframes * fc.frame_bits;
            std::vector<uint64_t> marked((size_t)(nmarked + 63) / 64), line((size_t)(ncoded / 64 + 1), 0);
            if (hipMemcpy(marked.data(), dec, marked.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
            for (uint64_t i = 0; i < ncoded; ++i) {
                const uint64_t b = i < (uint64_t)sync_junk ? gen() & 1 : marked[(size_t)((i - sync_junk) >> 6)] >> ((i - sync_junk) & 63) & 1;
                line[(size_t)(i >> 6)] |= b << (i & 63);
            }
            if (hipMemcpy(coded, line.data(), line.size() * 8, hipMemcpyHostToDevice) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        }
        CHECK(bbb_conv_encode(coded, ncoded, 0, &cc, nullptr, tx, &ntx, 0, nullptr));
        std::vector<uint64_t> txh((size_t)(ntx + 63) / 64), codedh((size_t)(ncoded + 63) / 64), dech((size_t)(ncoded + 63) / 64);
        if (hipMemcpy(txh.data(), tx, txh.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        std::vector<int16_t> x((size_t)ntx);
        std::normal_distribution<double> noise(0.0, (double)rs_sigma);
        const int one = sync ? -64 : 64;              // with --sync the whole channel is inverted
        for (uint64_t i = 0; i < ntx; ++i) x[(size_t)i] = (int16_t)((txh[(size_t)(i >> 6)] >> (i & 63) & 1 ? one : -one) + std::lrint(noise(gen)));
        if (hipMemcpy(soft, x.data(), ntx * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        CHECK(bbb_rx_slice(soft, ntx, 1, 0, 0, hard, &nhard, 0, nullptr));
        CHECK(bbb_conv_decode(hard, 0, nhard, 0, 0, 1, BBB_CONV_HARD, &cc, dec, nullptr, &nd, 0, nullptr));
        uint64_t nfound = nd / (8 * fcoded), fs[BBB_FRAMESYNC_NSTATE] = {0};
        if (sync) {
            CHECK(bbb_framesync_run(dec, nd, 0, 1, &fc, fstate, fpos, fmeta, nframes, fscratch, 0, nullptr));
            CHECK(bbb_frame_extract(dec, nd, 0, fpos, fmeta, fstate, nframes, &fc, (uint8_t *)frames, 0, nullptr));
            if (hipMemcpy(fs, fstate, sizeof fs, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
            nfound = std::min<uint64_t>(fs[0] >> 32, nframes);
        }
        CHECK(bbb_rs_decode(sync ? (const uint8_t *)frames : (const uint8_t *)dec, nfound, &rc, (uint8_t *)out, nullptr, stats, 0, nullptr));
        CHECK(bbb_prbs_check(k, 1, 0, nfound * fdata * 8, out, &e_data, 0, nullptr));
        e_data += (nframes - nfound) * fdata * 8;     // a frame that was not found is all wrong
        uint64_t st[BBB_RS_NSTATS];
        if (hipMemcpy(st, stats, sizeof st, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(codedh.data(), coded, codedh.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(dech.data(), dec, dech.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        const double secs = now_s() - t0;
        for (uint64_t i = 0; i < ntx; ++i) e_channel += (uint64_t)((x[(size_t)i] >= 0) != ((bool)(txh[(size_t)(i >> 6)] >> (i & 63) & 1) != sync));
        for (uint64_t i = 0; i < nd && i < ncoded; ++i) e_viterbi += ((codedh[(size_t)(i >> 6)] ^ dech[(size_t)(i >> 6)]) >> (i & 63) & 1) ^ (uint64_t)sync;
        for (void *p : {(void *)data, (void *)coded, (void *)tx, (void *)hard, (void *)dec, (void *)out, (void *)stats, (void *)soft, (void *)frames,
                        (void *)fstate, (void *)fpos, (void *)fmeta, (void *)fscratch})
            if (p) (void)hipFree(p);
        if (sync)
            std::printf("{\"mode\": \"sync\", \"junk_bits\": %d, \"inverted\": %llu, \"frames_found\": %llu, \"flywheeled\": %llu, \"acquisitions\": %llu, "
                        "\"losses\": %llu, \"rejected\": %llu, \"marker_bit_errors\": %llu}\n", sync_junk, (unsigned long long)(fs[0] >> 8 & 1),
                        (unsigned long long)fs[2], (unsigned long long)fs[3], (unsigned long long)fs[4], (unsigned long long)fs[5], (unsigned long long)fs[6],
                        (unsigned long long)fs[7]);
        std::printf("{\"mode\": \"rs\", \"code\": \"ccsds(255,223)\", \"depth\": %d, \"frames\": %llu, \"data_bits\": %llu, \"prbs\": %d, \"sigma\": %d, "
                    "\"coded_bits\": %llu, \"channel_errors\": %llu, \"viterbi_errors\": %llu, \"data_errors\": %llu, \"codewords\": %llu, \"clean\": %llu, "
                    "\"failed\": %llu, \"symbols_corrected\": %llu, \"bits_corrected\": %llu, \"seconds\": %.4f}\n", rs, (unsigned long long)nframes,
                    (unsigned long long)nbits, k, rs_sigma, (unsigned long long)ntx, (unsigned long long)e_channel, (unsigned long long)e_viterbi,
                    (unsigned long long)e_data, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3],
                    (unsigned long long)st[4], secs);
        return 0;
    }

    // ---- a capture from an ADC with its own clock: one fixed phase beside the timing recovery (bbb_timing_run) -----------------
    if (timing) {
        if (eye_samples < 4096 || nv < 0 || nv > 15 || timing < -1000 || timing > 1000) {
            std::fprintf(stderr, "--eye-samples >= 4096, --nv 0..15, --timing -1000..1000 (not 0)\n");
            return 2;
        }
        bbb_tx_cfg cfg{};
        for (int i = 30; i < 34; i++) cfg.coeffs[i] = 254;          // the rectangular pulse (bitshaper.py:108)
        cfg.source = 0;
        cfg.prbs_k = k;
        cfg.prbs_state = 1;
        cfg.bit_en = 1;
        cfg.noise_en = 1;
        cfg.noise_var = nv;
        cfg.warmup = 16;
        const uint64_t init[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        bbb_lutopt *h = nullptr;
        CHECK(bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, 0));
        const uint64_t ntx = (uint64_t)eye_samples;
        // y[n] = (x[i] (65536 - f) + x[i + 1] f) >> 16 at pos = n * (65536 + OFFSET), i = pos >> 16, f = pos & 65535
        const uint64_t step = (uint64_t)(65536 + timing);
        const uint64_t nrx = std::min<uint64_t>(ntx, ((ntx - 2) << 16) / step);
        bbb_timing_cfg tc{};
        CHECK(bbb_fir_moving_average(&tc.ff, 0));
        tc.spb = 8;
        tc.init_phase = BBB_TIMING_ACQUIRE;
        uint64_t nblocks = 0, nconsumed = 0, max_bits = 0;
        CHECK(bbb_timing_plan(&tc, nrx, 1, &nblocks, &nconsumed, &max_bits, nullptr));
        int16_t *w = nullptr;
        uint64_t *b = nullptr, *words = nullptr;                    // words: state[2], stats[4], nbits
        if (hipMalloc((void **)&w, ntx * sizeof(int16_t)) != hipSuccess || hipMalloc((void **)&b, (max_bits / 64 + 2) * sizeof(uint64_t)) != hipSuccess ||
            hipMalloc((void **)&words, 7 * sizeof(uint64_t)) != hipSuccess || hipMemset(words, 0, 7 * sizeof(uint64_t)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        CHECK(bbb_tx_fill_i16(h, &cfg, w, ntx, 0));
        std::vector<int16_t> x(ntx), y(nrx);
        if (hipMemcpy(x.data(), w, ntx * sizeof(int16_t), hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        for (uint64_t n = 0; n < nrx; ++n) {
            const uint64_t pos = n * step, i = pos >> 16;
            const int64_t f = (int64_t)(pos & 65535);
            y[n] = (int16_t)(((int64_t)x[i] * (65536 - f) + (int64_t)x[i + 1] * f) >> 16);
        }
        if (hipMemcpy(w, y.data(), nrx * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        uint64_t nfix = 0;
        bbb_detector_stats fix{}, trk{};
        const double t0 = now_s();
        bbb_fir_cfg fc = tc.ff;
        fc.decim = 8;
        fc.phase = 2;                                               // where the running sum of four is complete without an offset
        CHECK(bbb_fir_slice(w, nrx, 0, &fc, 0, 0, b, &nfix, 0, nullptr));
        CHECK(bbb_prbs_detector_stream(k, b, nfix, nullptr, nullptr, &fix, 0, 0, 0, nullptr));
        CHECK(bbb_timing_run(w, nrx, 0, 1, &tc, words, b, nullptr, nullptr, words + 2, words + 6, 0, nullptr));
        uint64_t out[7];
        if (hipMemcpy(out, words, sizeof out, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        CHECK(bbb_prbs_detector_stream(k, b, out[6], nullptr, nullptr, &trk, 0, 0, 0, nullptr));
        const double secs = now_s() - t0;
        CHECK(bbb_lutopt_destroy(h));
        (void)hipFree(w);
        (void)hipFree(b);
        (void)hipFree(words);
        std::printf("{\"mode\": \"timing\", \"samples\": %llu, \"prbs\": %d, \"nv\": %d, \"offset_ppm\": %.1f, \"fixed_phase\": {\"phase\": 2, \"bits\": %llu, "
                    "\"errors\": %llu, \"reload_clocks\": %llu}, \"timing\": {\"bits\": %llu, \"errors\": %llu, \"reload_clocks\": %llu, \"blocks\": %llu, "
                    "\"moves\": %llu, \"wraps_up\": %llu, \"wraps_down\": %llu, \"last_phase\": %llu}, \"seconds\": %.4f}\n",
                    (unsigned long long)nrx, k, nv, timing / 65536.0 * 1e6, (unsigned long long)fix.bits, (unsigned long long)fix.errors,
                    (unsigned long long)fix.reload_clocks, (unsigned long long)trk.bits, (unsigned long long)trk.errors,
                    (unsigned long long)trk.reload_clocks, (unsigned long long)out[2], (unsigned long long)out[3], (unsigned long long)out[4],
                    (unsigned long long)out[5], (unsigned long long)(out[0] & 0xFFFFFFFFull), secs);
        return 0;
    }

    // ---- an echo one bit late: the moving-average receiver beside the same filter with one feedback tap (bbb_dfe_run) ---------
    if (dfe || mlse) {
        if (eye_samples < 1 || nv < 0 || nv > 15 || mlse < 0 || mlse > 4) { std::fprintf(stderr, "--eye-samples >= 1, --nv 0..15, --mlse 1..4\n"); return 2; }
        bbb_tx_cfg cfg{};
        for (int i = 30; i < 34; i++) cfg.coeffs[i] = 254;          // the rectangular pulse (bitshaper.py:108)
        cfg.source = 0;
        cfg.prbs_k = k;
        cfg.prbs_state = 1;
        cfg.bit_en = 1;
        cfg.noise_en = 1;
        cfg.noise_var = nv;
        cfg.warmup = 16;
        const uint64_t init[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        bbb_lutopt *h = nullptr;
        CHECK(bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, 0));
        const uint64_t ntx = (uint64_t)eye_samples;
        int16_t *w = nullptr, *y = nullptr;
        uint64_t *b = nullptr, *stats = nullptr;
        uint32_t *state = nullptr;
        if (hipMalloc((void **)&w, ntx * sizeof(int16_t)) != hipSuccess || hipMalloc((void **)&y, ntx * sizeof(int16_t)) != hipSuccess ||
            hipMalloc((void **)&b, (ntx / 8 / 64 + 2) * sizeof(uint64_t)) != hipSuccess || hipMalloc((void **)&stats, 4 * sizeof(uint64_t)) != hipSuccess ||
            hipMalloc((void **)&state, sizeof(uint32_t)) != hipSuccess || hipMemset(stats, 0, 4 * sizeof(uint64_t)) != hipSuccess ||
            hipMemset(state, 0, sizeof(uint32_t)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        CHECK(bbb_tx_fill_i16(h, &cfg, w, ntx, 0));
        // the channel: y(n) = (10 x(n) + 7 x(n - 8)) >> 4, an echo of 0.7 one bit late
        bbb_fir_cfg ch{};
        ch.ntaps = 9, ch.taps[0] = 10, ch.taps[8] = 7, ch.shift = 4, ch.decim = 1, ch.out_bytes = 2;
        CHECK(bbb_fir_filter(w, ntx, 0, &ch, y, nullptr, 0, nullptr));
        // bit m holds samples 8m + 47 .. 8m + 50 at 254 * 10 >> 4 = 158 and its echo at 254 * 7 >> 4 = 111: the running sum of
        // four is complete at 8m + 50 and carries 4 * 111 of the bit before
        uint64_t nlin = 0, ndfe = 0;
        bbb_detector_stats lin{}, eq{};
        const double t0 = now_s();
        bbb_dfe_cfg dc{};
        CHECK(bbb_fir_moving_average(&dc.ff, 0));
        dc.ff.decim = 8;
        dc.ff.phase = 2;
        CHECK(bbb_fir_slice(y, ntx, 0, &dc.ff, 0, 0, b, &nlin, 0, nullptr));
        CHECK(bbb_prbs_detector_stream(k, b, nlin, nullptr, nullptr, &lin, 0, 0, 0, nullptr));
        dc.nfb = 1;
        dc.fb[0] = 4 * 111;
        CHECK(bbb_dfe_run(y, ntx, 0, &dc, state, b, nullptr, stats, &ndfe, 0, nullptr));
        CHECK(bbb_prbs_detector_stream(k, b, ndfe, nullptr, nullptr, &eq, 0, 0, 0, nullptr));
        // the sequence detector on the same filter: the bit and its echo are the target, 4 * 158 and 4 * 111 in units of y
        uint64_t nml = 0;
        bbb_detector_stats ml{};
        if (mlse) {
            bbb_mlse_cfg mc{};
            mc.ff = dc.ff;
            mc.mem = (uint32_t)mlse;
            mc.g[0] = 4 * 158;
            mc.g[1] = 4 * 111;
            CHECK(bbb_mlse_run(y, ntx, 0, 0, 1, &mc, b, nullptr, &nml, 0, nullptr));
            CHECK(bbb_prbs_detector_stream(k, b, nml, nullptr, nullptr, &ml, 0, 0, 0, nullptr));
        }
        const double secs = now_s() - t0;
        uint64_t st[4] = {0, 0, 0, 0};
        if (hipMemcpy(st, stats, sizeof st, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "copy failed\n"); return 1; }
        CHECK(bbb_lutopt_destroy(h));
        (void)hipFree(w);
        (void)hipFree(y);
        (void)hipFree(b);
        (void)hipFree(stats);
        (void)hipFree(state);
        if (mlse) {
            std::printf("{\"mode\": \"mlse\", \"samples\": %llu, \"prbs\": %d, \"nv\": %d, \"echo\": 0.7, \"moving_average\": {\"bits\": %llu, \"errors\": %llu}, "
                        "\"dfe\": {\"fb\": %d, \"bits\": %llu, \"errors\": %llu}, \"mlse\": {\"mem\": %d, \"g\": [%d, %d], \"bits\": %llu, \"errors\": %llu}, "
                        "\"seconds\": %.4f}\n", (unsigned long long)ntx, k, nv, (unsigned long long)lin.bits, (unsigned long long)lin.errors, dc.fb[0],
                        (unsigned long long)eq.bits, (unsigned long long)eq.errors, mlse, 4 * 158, 4 * 111, (unsigned long long)ml.bits,
                        (unsigned long long)ml.errors, secs);
            return 0;
        }
        std::printf("{\"mode\": \"dfe\", \"samples\": %llu, \"prbs\": %d, \"nv\": %d, \"echo\": 0.7, \"moving_average\": {\"bits\": %llu, \"errors\": %llu}, "
                    "\"dfe\": {\"fb\": %d, \"bits\": %llu, \"errors\": %llu, \"regions\": %llu, \"not_proven\": %llu, \"repaired\": %llu}, "
                    "\"seconds\": %.4f}\n", (unsigned long long)ntx, k, nv, (unsigned long long)lin.bits, (unsigned long long)lin.errors, dc.fb[0],
                    (unsigned long long)eq.bits, (unsigned long long)eq.errors, (unsigned long long)st[0], (unsigned long long)st[1],
                    (unsigned long long)st[2], secs);
        return 0;
    }

    // ---- the transmitter's pulse response, measured against its own data bits with the noise off ----------------------------
    if (xcorr) {
        if (!lags_set) lags = 64;                                   // the coefficient set has 64 entries
        if (shape < 0 || shape > 31 || eye_samples < 1 || lags < 1 || lags > 512) {
            std::fprintf(stderr, "--shape 0..31, --eye-samples >= 1, --lags 1..512\n");
            return 2;
        }
        bbb_tx_cfg cfg{};
        rcf_taps(shape == 31 ? 1.0 : shape * (1.0 / 31), cfg.coeffs);          // tx.py:54: np.linspace(0, 1, 32)
        cfg.source = 0;
        cfg.prbs_k = k;
        cfg.prbs_state = 1;
        cfg.bit_en = 1;
        cfg.noise_en = 0;
        cfg.noise_var = 0;
        cfg.warmup = 16;
        const uint64_t init[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        bbb_lutopt *h = nullptr;
        CHECK(bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, 0));
        bbb_tx_xcorr *x = nullptr;
        CHECK(bbb_tx_xcorr_open(h, &cfg, (uint32_t)lags, 0, &x));
        int64_t *d = nullptr;
        if (hipMalloc((void **)&d, (size_t)lags * sizeof(int64_t)) != hipSuccess || hipMemset(d, 0, (size_t)lags * sizeof(int64_t)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        const uint64_t count = (uint64_t)eye_samples;
        const double t0 = now_s();
        CHECK(bbb_tx_xcorr_run(x, 0, count, d));
        std::vector<int64_t> xc((size_t)lags);
        if (hipMemcpy(xc.data(), d, xc.size() * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        const double secs = now_s() - t0;
        CHECK(bbb_tx_xcorr_close(x));
        CHECK(bbb_lutopt_destroy(h));
        (void)hipFree(d);
        std::printf("{\"mode\": \"xcorr\", \"samples\": %llu, \"prbs\": %d, \"shape\": %d, \"lags\": %d, \"seconds\": %.4f, \"pulse_response\": [",
                    (unsigned long long)count, k, shape, lags, secs);
        for (int l = 0; l < lags; l++) {
            // the terms of lag l: samples n < count with n >= 17 + l and n = 17 + l modulo 8
            const uint64_t first = (uint64_t)BBB_TX_BIT_ORIGIN + (uint64_t)l;
            const uint64_t terms = count > first ? (count - first + 7) / 8 : 0;
            std::printf("%s%.4f", l ? ", " : "", terms ? (double)xc[(size_t)l] / (double)terms : 0.0);
        }
        std::printf("], \"coeffs\": [");
        for (int l = 0; l < lags && l < 64; l++) std::printf("%s%d", l ? ", " : "", (int)cfg.coeffs[l]);
        std::printf("]}\n");
        return 0;
    }

    // ---- autocorrelation and power spectrum of the transmitter (software/memdump/fftplot.py) -----------------------------
    if (!specfile.empty()) {
        if (shape < 0 || shape > 31 || eye_samples < 1 || lags < 1 || lags > BBB_ACF_MAX_LAGS) {
            std::fprintf(stderr, "--shape 0..31, --eye-samples >= 1, --lags 1..%d\n", BBB_ACF_MAX_LAGS);
            return 2;
        }
        bbb_tx_cfg cfg{};
        rcf_taps(shape == 31 ? 1.0 : shape * (1.0 / 31), cfg.coeffs);          // tx.py:54: np.linspace(0, 1, 32)
        cfg.source = 0;
        cfg.prbs_k = k;
        cfg.prbs_state = 1;
        cfg.bit_en = 1;
        cfg.noise_en = 1;
        cfg.noise_var = nv;
        cfg.warmup = 16;
        const uint64_t init[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        bbb_lutopt *h = nullptr;
        CHECK(bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, 0));
        bbb_tx_acf *a = nullptr;
        CHECK(bbb_tx_acf_open(h, &cfg, (uint32_t)lags, 0, &a));
        const size_t nw = (size_t)lags + 1;
        int64_t *d = nullptr;
        if (hipMalloc((void **)&d, nw * sizeof(int64_t)) != hipSuccess || hipMemset(d, 0, nw * sizeof(int64_t)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        const uint64_t count = (uint64_t)eye_samples;
        const double t0 = now_s();
        CHECK(bbb_tx_acf_run(a, 0, count, d));
        std::vector<int64_t> acf(nw);
        if (hipMemcpy(acf.data(), d, nw * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        const double secs = now_s() - t0;
        CHECK(bbb_tx_acf_close(a));
        CHECK(bbb_lutopt_destroy(h));
        (void)hipFree(d);
        // Blackman-Tukey: c[l] = acf[l] / count - mu^2, Bartlett window w[l] = 1 - l / L, P[k] = w[0] c[0] + 2 sum_l w[l] c[l]
        // cos(2 pi k l / nfft) over nfft = the smallest power of two >= 2L, bins 1 .. nfft/2 - 1 doubled (one-sided)
        const int L = lags;
        uint64_t nfft = 2;
        while (nfft < 2 * (uint64_t)L) nfft *= 2;
        const double mu = (double)acf[L] / (double)count;
        std::vector<double> y(L), table(nfft);
        for (int l = 0; l < L; l++) y[l] = (1.0 - (double)l / L) * ((double)acf[l] / (double)count - mu * mu);
        for (uint64_t j = 0; j < nfft; j++) table[j] = std::cos(2 * M_PI * (double)j / (double)nfft);
        FILE *f = std::fopen(specfile.c_str(), "w");
        if (!f) { std::fprintf(stderr, "cannot write %s\n", specfile.c_str()); return 1; }
        bool ok = std::fprintf(f, "k,freq,psd,psd_db\n") > 0;
        for (uint64_t kb = 0; kb <= nfft / 2; kb++) {
            double s = 0;
            for (int l = 1; l < L; l++) s += y[l] * table[(kb * (uint64_t)l) % nfft];
            double p = y[0] + 2 * s;
            if (kb > 0 && kb < nfft / 2) p *= 2;
            ok = ok && std::fprintf(f, "%llu,%.17g,%.17g,%.17g\n", (unsigned long long)kb, (double)kb / (double)nfft, p,
                                    10 * std::log10(p)) > 0;
        }
        if (std::fclose(f) != 0 || !ok) { std::fprintf(stderr, "cannot write %s\n", specfile.c_str()); return 1; }
        std::printf("{\"mode\": \"spectrum\", \"samples\": %llu, \"prbs\": %d, \"nv\": %d, \"shape\": %d, \"lags\": %d, \"nfft\": %llu, "
                    "\"seconds\": %.4f, \"csv\": \"%s\", \"acf\": [", (unsigned long long)count, k, nv, shape, L,
                    (unsigned long long)nfft, secs, specfile.c_str());
        for (size_t i = 0; i < nw; i++) std::printf("%s%lld", i ? ", " : "", (long long)acf[i]);
        std::printf("]}\n");
        return 0;
    }

    // ---- the bathtub of one setting, raw and behind the moving average (bbb_link_sweep_*) ------------------------------------
    if (link) {
        if (shape < 0 || shape > 31 || eye_samples < 1 || nv < 0 || nv > 15 || link_delay < 0 || link_delay > 255) {
            std::fprintf(stderr, "--shape 0..31, --eye-samples >= 1, --nv 0..15, --delay 0..255\n");
            return 2;
        }
        bbb_tx_cfg base{};
        base.source = 0;
        base.prbs_k = k;
        base.prbs_state = 1;
        base.warmup = 16;
        bbb_tx_setting st{};
        rcf_taps(shape == 31 ? 1.0 : shape * (1.0 / 31), st.coeffs);            // tx.py:54: np.linspace(0, 1, 32)
        st.bit_en = 1;
        st.noise_en = 1;
        st.noise_var = nv;
        const uint64_t init[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        bbb_lutopt *h = nullptr;
        CHECK(bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, 0));
        bbb_tx_ber_sweep *raw = nullptr;
        CHECK(bbb_tx_ber_sweep_open(h, &base, &st, 1, 0, &raw));
        bbb_fir_cfg fc;
        CHECK(bbb_fir_moving_average(&fc, 0));
        bbb_link_sweep *ma = nullptr;
        CHECK(bbb_link_sweep_open(h, &base, &st, 1, &fc, (uint32_t)link_delay, nullptr, 0, &ma));
        uint64_t *d = nullptr;
        if (hipMalloc((void **)&d, 32 * sizeof(uint64_t)) != hipSuccess || hipMemset(d, 0, 32 * sizeof(uint64_t)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        const double t0 = now_s();
        CHECK(bbb_tx_ber_sweep_run(raw, 0, (uint64_t)eye_samples, d));
        CHECK(bbb_link_sweep_run(ma, 0, (uint64_t)eye_samples, d + 16, nullptr));
        uint64_t out[32];
        if (hipMemcpy(out, d, sizeof out, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        const double secs = now_s() - t0;
        CHECK(bbb_link_sweep_close(ma));
        CHECK(bbb_tx_ber_sweep_close(raw));
        CHECK(bbb_lutopt_destroy(h));
        (void)hipFree(d);
        std::printf("{\"mode\": \"link\", \"samples\": %llu, \"prbs\": %d, \"shape\": %d, \"nv\": %d, \"taps\": [1, 1, 1, 1], \"delay\": %d, "
                    "\"seconds\": %.4f}\n", (unsigned long long)eye_samples, k, shape, nv, link_delay, secs);
        for (int p = 0; p < 8; p++)
            std::printf("{\"phase\": %d, \"bits\": %llu, \"raw_errors\": %llu, \"filtered_bits\": %llu, \"filtered_errors\": %llu}\n", p,
                        (unsigned long long)out[2 * p], (unsigned long long)out[2 * p + 1], (unsigned long long)out[16 + 2 * p],
                        (unsigned long long)out[16 + 2 * p + 1]);
        return 0;
    }

    // ---- BER of the shaped link over noise_var in one pass (bbb_tx_ber_sweep_*) ------------------------------------------
    if (tx_sweep) {
        if (shape < 0 || shape > 31 || eye_samples < 1 || nv_lo < 0 || nv_hi > 15 || nv_lo > nv_hi) {
            std::fprintf(stderr, "--shape 0..31, --eye-samples >= 1, --nv-range A:B with 0 <= A <= B <= 15\n");
            return 2;
        }
        bbb_tx_cfg base{};
        base.source = 0;
        base.prbs_k = k;
        base.prbs_state = 1;
        base.warmup = 16;
        std::vector<bbb_tx_setting> settings;
        for (int v = nv_lo; v <= nv_hi; v++) {
            bbb_tx_setting st{};
            rcf_taps(shape == 31 ? 1.0 : shape * (1.0 / 31), st.coeffs);        // tx.py:54: np.linspace(0, 1, 32)
            st.bit_en = 1;
            st.noise_en = 1;
            st.noise_var = v;
            settings.push_back(st);
        }
        const int nset = (int)settings.size();
        const uint64_t init[8] = {init0, 0, 0, 0, 0, 0, 0, 0};
        bbb_lutopt *h = nullptr;
        CHECK(bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, 0));
        bbb_tx_ber_sweep *s = nullptr;
        CHECK(bbb_tx_ber_sweep_open(h, &base, settings.data(), nset, 0, &s));
        const size_t nw = (size_t)nset * 16;
        uint64_t *d = nullptr;
        if (hipMalloc((void **)&d, nw * sizeof(uint64_t)) != hipSuccess || hipMemset(d, 0, nw * sizeof(uint64_t)) != hipSuccess) {
            std::fprintf(stderr, "hipMalloc failed\n");
            return 1;
        }
        const double t0 = now_s();
        CHECK(bbb_tx_ber_sweep_run(s, 0, (uint64_t)eye_samples, d));
        std::vector<uint64_t> out(nw);
        if (hipMemcpy(out.data(), d, nw * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "hipMemcpy failed\n"); return 1; }
        const double secs = now_s() - t0;
        CHECK(bbb_tx_ber_sweep_close(s));
        CHECK(bbb_lutopt_destroy(h));
        (void)hipFree(d);
        std::printf("{\"mode\": \"tx-sweep\", \"samples\": %llu, \"prbs\": %d, \"shape\": %d, \"settings\": %d, \"seconds\": %.4f}\n",
                    (unsigned long long)eye_samples, k, shape, nset, secs);
        for (int i = 0; i < nset; i++)
            for (int p = 0; p < 8; p++) {
                const uint64_t nb = out[(size_t)i * 16 + 2 * p], ne = out[(size_t)i * 16 + 2 * p + 1];
                std::printf("{\"shape\": %d, \"nv\": %d, \"phase\": %d, \"bits\": %llu, \"errors\": %llu, \"ber\": %.6e}\n", shape,
                            nv_lo + i, p, (unsigned long long)nb, (unsigned long long)ne, nb ? (double)ne / (double)nb : 0.0);
            }
        return 0;
    }

    // ---- AWGN fill mode (BASELINE configs[1]) -----------------------------------------------------------------------
    if (nsamples > 0) {
        const uint64_t n = (uint64_t)nsamples;
        std::vector<FillResult> res((size_t)gpus);
        std::vector<std::thread> th;
        for (int d = 1; d < gpus; d++) th.emplace_back(fill_worker, std::cref(m), init0, d, gpus, n, steps, staged, &res[(size_t)d]);
        fill_worker(m, init0, 0, gpus, n, steps, staged, &res[0]);
        for (auto &t : th) t.join();
        double wall = 0, kms = 0;
        for (int d = 0; d < gpus; d++) {
            if (res[(size_t)d].rc) { std::fprintf(stderr, "device %d: %s\n", d, res[(size_t)d].err.c_str()); return 1; }
            wall = std::fmax(wall, res[(size_t)d].wall_s);
            kms = std::fmax(kms, res[(size_t)d].kernel_ms);
        }
        const double gs = (double)gpus * steps * (double)n / wall / 1e9;
        // what one launch of the sample kernel produces (bbb.h, bbb_lutopt_set_staged: look-ahead applies to fills of at
        // least 2^24 samples, a multiple of 16)
        const uint64_t per_launch = res[0].launches ? (uint64_t)steps * n / res[0].launches : n;
        const double kernel_gbs = kms > 0 ? (double)per_launch / (kms * 1e-3) / 1e9 : 0;        // 1 B per sample
        if (json) {
            std::printf("{\"mode\": \"awgn_fill\", \"n_gpus\": %d, \"samples_per_step_per_gpu\": %llu, \"steps\": %d, \"gsample_s\": %.3f, "
                        "\"kernel_ms_avg\": %.4f, \"samples_per_launch\": %llu, \"seed_ms_avg\": %.4f, \"hbm_write_gb_s_per_gpu\": %.1f, \"hbm_roofline_frac\": %.4f, "
                        "\"collective\": \"none (independent shards of one sequential stream)\", \"head\": [",
                        gpus, (unsigned long long)n, steps, gs, kms, (unsigned long long)per_launch, res[0].seed_ms, kernel_gbs, kernel_gbs / kHbmPeakGBs);
            for (size_t i = 0; i < res[0].head.size(); i++) std::printf("%s%d", i ? ", " : "", (int)res[0].head[i]);
            std::printf("]}\n");
        } else {
            std::printf("# AWGN fill: %d GPU(s) x %d steps x %llu samples: %.3f Gsample/s, sample kernel %.4f ms = %.1f GB/s = %.4f of the HBM peak\n",
                        gpus, steps, (unsigned long long)n, gs, kms, kernel_gbs, kernel_gbs / kHbmPeakGBs);
            std::printf("# head:");
            for (size_t i = 0; i < res[0].head.size(); i++) std::printf(" %d", (int)res[0].head[i]);
            std::printf("\n");
        }
        return 0;
    }

    // ---- BER sweep (BASELINE configs[3], [4]) -----------------------------------------------------------------------
    // amplitude for an Eb/N0: sigma of the scaled CLT sample is 8 * nv (CLTGRNG variance 64), one sample per bit
    std::vector<bbb_trial_cfg> cfg;
    for (double db = from; db <= to + 1e-9; db += step) {
        bbb_trial_cfg c{};
        c.prbs_k = k;
        c.noise_var = nv;
        c.amp = (int)std::lround(8.0 * nv * std::sqrt(2.0 * std::pow(10.0, db / 10.0)));
        c.prbs_state = 1;
        c.warmup = 16;                                                  // 2 * log2(n): rng.py:161-162
        c.first_bit = 0;
        c.nbits = (uint64_t)bits;
        cfg.push_back(c);
    }
    // --shard groups (BASELINE configs[4] as ONE call): the sweep once per seed -- the seeds as stretches of the one cycle 2^48
    // clocks apart, all on the same reset state -- as --seeds groups of consecutive trials; a group stays on one device
    // (bbb_ber_sweep_multi, BBB_SHARD_GROUPS: group q on device q mod N), the rows below are the sums over the seeds
    const size_t npoints = cfg.size();
    if (mode == BBB_SHARD_GROUPS) {
        for (int sd = 1; sd < seeds; sd++)
            for (size_t i = 0; i < npoints; i++) {
                bbb_trial_cfg c = cfg[i];
                c.warmup = 16 + ((uint64_t)sd << 48);
                cfg.push_back(c);
            }
    }
    const int group_seeds = seeds;
    std::vector<bbb_ber> out(cfg.size()), part(cfg.size());
    double ms = 0;
    const char *reduce = "single device";
    bbb_multi_info minfo{};
    int equals_single = -1;              // -1: not compared (single device, or one seed per device)
    if (gpus > 1 || multi) {
        // one handle per device; seeds mode gives device d seed d
        std::vector<bbb_lutopt *> hs((size_t)gpus, nullptr);
        for (int d = 0; d < gpus; d++) {
            uint64_t init[8];
            CHECK(seed_words(mode == BBB_SHARD_SEEDS ? d : 0, init));
            CHECK(bbb_lutopt_create(&hs[(size_t)d], m.n, m.taps.data(), m.off.data(), init, d));
        }
        CHECK(bbb_ber_sweep_multi(hs.data(), gpus, cfg.data(), (int)cfg.size(), mode, out.data()));   // plans + communicators
        const double t0 = now_s();
        CHECK(bbb_ber_sweep_multi(hs.data(), gpus, cfg.data(), (int)cfg.size(), mode, out.data()));
        ms = (now_s() - t0) * 1e3;
        // a multi-device run checks itself: what the communicator says, which RCCL it was, and -- for the sharding modes whose
        // totals do not depend on the device count -- the same trials on device 0 alone
        CHECK(bbb_multi_last_info(&minfo));
        if (mode != BBB_SHARD_SEEDS) {
            std::vector<bbb_ber> single(cfg.size());
            CHECK(bbb_ber_trials(hs[0], cfg.data(), (int)cfg.size(), single.data()));
            equals_single = 1;
            for (size_t i = 0; i < cfg.size(); i++)
                if (single[i].bits != out[i].bits || single[i].errors != out[i].errors) equals_single = 0;
        }
        for (auto *h : hs) CHECK(bbb_lutopt_destroy(h));
        CHECK(bbb_multi_release());
        reduce = "ncclAllReduce(uint64[2 x points], sum) over the devices of this process";
        seeds = mode == BBB_SHARD_SEEDS ? gpus : (mode == BBB_SHARD_GROUPS ? group_seeds : 1);
        if (mode == BBB_SHARD_GROUPS) {                                  // fold the seeds' rows into the points'
            for (int sd = 1; sd < group_seeds; sd++)
                for (size_t i = 0; i < npoints; i++) { out[i].bits += out[(size_t)sd * npoints + i].bits; out[i].errors += out[(size_t)sd * npoints + i].errors; }
            out.resize(npoints);
            cfg.resize(npoints);
        }
    } else if (mode == BBB_SHARD_GROUPS) {
        std::fprintf(stderr, "--shard groups runs through bbb_ber_sweep_multi: add --multi 1 (one device) or --gpus N\n");
        return 2;
    } else {
        bbb_lutopt *h = nullptr;
        for (int sd = 0; sd < seeds; sd++) {
            uint64_t init[8];                                                      // reset value (gateware/bbb/rng.py:21), jumped
            CHECK(seed_words(sd, init));
            if (h) CHECK(bbb_lutopt_destroy(h));
            CHECK(bbb_lutopt_create(&h, m.n, m.taps.data(), m.off.data(), init, 0));
            CHECK(bbb_ber_trials(h, cfg.data(), (int)cfg.size(), part.data()));  // first call builds the jump plans
            const double t0 = now_s();
            CHECK(bbb_ber_trials(h, cfg.data(), (int)cfg.size(), part.data()));
            ms += (now_s() - t0) * 1e3;
            for (size_t i = 0; i < cfg.size(); i++) { out[i].bits += part[i].bits; out[i].errors += part[i].errors; }
        }
        CHECK(bbb_lutopt_destroy(h));
    }
    unsigned long long total_bits = 0;
    for (auto &o : out) total_bits += o.bits;
    if (!json) {
        std::printf("# PRBS-%d, noise_var %d, %.3g bits per point and seed, %d seed(s), %d GPU(s), %zu points in %.3f ms\n", k, nv, bits, seeds,
                    gpus, cfg.size(), ms);
        std::printf("# EbN0_dB  amp  bits  errors  BER  Q(sqrt(2EbN0))\n");
    }
    for (size_t i = 0; i < cfg.size(); i++) {
        const double ebn0 = (double)cfg[i].amp * cfg[i].amp / (2.0 * 64.0 * nv * nv);
        // the slicer threshold falls on the integer lattice of the sigma = 8 sample: an error needs
        // |g| >= ceil(amp / nv), which is what a continuous Gaussian would see at this effective Eb/N0
        const double thr = std::ceil((double)cfg[i].amp / nv) - 0.5;
        const double ebn0_eff = thr * thr / (2.0 * 64.0);
        const double ber = out[i].bits ? (double)out[i].errors / (double)out[i].bits : 0.0;
        if (json)
            std::printf("{\"ebn0_db\": %.3f, \"ebn0_db_effective\": %.3f, \"amp\": %d, \"noise_var\": %d, \"bits\": %llu, \"errors\": %llu, "
                        "\"ber\": %.6e, \"q_theory\": %.6e, \"q_theory_effective\": %.6e}\n",
                        10 * std::log10(ebn0), 10 * std::log10(ebn0_eff), cfg[i].amp, nv, (unsigned long long)out[i].bits,
                        (unsigned long long)out[i].errors, ber, 0.5 * std::erfc(std::sqrt(ebn0)), 0.5 * std::erfc(std::sqrt(ebn0_eff)));
        else
            std::printf("%7.3f %4d %llu %llu %.4e %.4e\n", 10 * std::log10(ebn0), cfg[i].amp, (unsigned long long)out[i].bits,
                        (unsigned long long)out[i].errors, ber, 0.5 * std::erfc(std::sqrt(ebn0)));
    }
    if (json)
        std::printf("{\"mode\": \"ber_sweep\", \"prbs_k\": %d, \"points\": %zu, \"n_gpus\": %d, \"shard\": \"%s\", \"seeds\": %d, \"total_bits\": %llu, "
                    "\"ms\": %.3f, \"gbit_trials_s\": %.2f, \"hbm_bytes_per_bit\": 0, \"hbm_roofline_frac\": null, "
                    "\"bound\": \"integer VALU (no sample stream is written)\", \"reduce\": \"%s\", \"n_ranks_seen\": %d, "
                    "\"rccl_path\": \"%s\", \"rccl_reused\": %s, \"equals_single_device_counters\": %s}\n",
                    k, cfg.size(), gpus, shard.c_str(), seeds, total_bits, ms, ms > 0 ? (double)total_bits / (ms * 1e-3) / 1e9 : 0.0, reduce,
                    minfo.n_ranks_seen, minfo.rccl_path, minfo.rccl_reused ? "true" : "false",
                    equals_single < 0 ? "null" : (equals_single ? "true" : "false"));
    if (loopback > 0) {
        const uint64_t nb = (uint64_t)loopback;
        uint64_t *buf = nullptr;
        (void)hipSetDevice(0);
        if (hipMalloc(&buf, ((nb + 63) / 64) * 8) != hipSuccess) { std::fprintf(stderr, "hipMalloc failed\n"); return 1; }
        CHECK(bbb_prbs_fill(k, 1, 0, nb, buf, 0, nullptr));
        uint64_t nerr = 0;
        CHECK(bbb_prbs_check(k, 1, 0, nb, buf, &nerr, 0, nullptr));         // warm
        hipEvent_t e0, e1, e2;
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); (void)hipEventCreate(&e2);
        (void)hipEventRecord(e0, nullptr);
        CHECK(bbb_prbs_fill(k, 1, 0, nb, buf, 0, nullptr));
        (void)hipEventRecord(e1, nullptr);
        CHECK(bbb_prbs_check(k, 1, 0, nb, buf, &nerr, 0, nullptr));
        (void)hipEventRecord(e2, nullptr);
        (void)hipEventSynchronize(e2);
        float fill_ms = 0, chk_ms = 0;
        (void)hipEventElapsedTime(&fill_ms, e0, e1);
        (void)hipEventElapsedTime(&chk_ms, e1, e2);
        bbb_detector_stats st{};
        CHECK(bbb_prbs_detector_stream(k, buf, nb, nullptr, nullptr, &st, 0, 0, 0, nullptr));
        const double fgb = (double)nb / 8 / (fill_ms * 1e-3) / 1e9, cgb = (double)nb / 8 / (chk_ms * 1e-3) / 1e9;
        if (json)
            std::printf("{\"mode\": \"prbs_loopback\", \"prbs_k\": %d, \"bits\": %llu, \"check_errors\": %llu, \"detector_errors\": %llu, "
                        "\"resyncs\": %llu, \"reload_clocks\": %llu, \"fill_gb_s\": %.1f, \"check_gb_s\": %.1f, "
                        "\"fill_hbm_frac\": %.4f, \"check_hbm_frac\": %.4f}\n",
                        k, (unsigned long long)st.bits, (unsigned long long)nerr, (unsigned long long)st.errors,
                        (unsigned long long)st.resyncs, (unsigned long long)st.reload_clocks, fgb, cgb, fgb / kHbmPeakGBs, cgb / kHbmPeakGBs);
        else
            std::printf("# loopback: %llu bits, %llu errors, %llu resyncs, %llu reload clocks\n", (unsigned long long)st.bits,
                        (unsigned long long)st.errors, (unsigned long long)st.resyncs, (unsigned long long)st.reload_clocks);
        (void)hipFree(buf);
    }
    return 0;
}
