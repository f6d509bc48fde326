// bbb_common.hpp -- shared host-side plumbing for libbbb_hip.so (error codes, HIP checks).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/bbb.h"

#include "custom_abi.hpp"

namespace bbb {

// per-thread text of the last failure (returned by bbb_last_error_detail)
std::string &last_error();

inline int fail(int code, const std::string &what) {
    last_error() = what;
    return code;
}

#define BBB_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return ::bbb::fail(BBB_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// Select `device` after checking that it exists and is a gfx950 part: there is no other
// execution path in this library.
int use_device(int device);

constexpr int kWave = 64;   // CDNA wavefront

// floor(v / d) for signed v and d > 0
inline int64_t floor_div(int64_t v, int64_t d) { return v >= 0 ? v / d : -((-v + d - 1) / d); }
inline int64_t floor8(int64_t v) { return floor_div(v, 8); }

// data bits lo .. hi (inclusive; lo may lie below bit 0, hi < lo: none) that a chunk of samples needs
struct BitRange { int64_t lo, hi; };

// the transmitter's own range, for every call that takes first_sample and nsamples
inline int tx_range_check(uint64_t first, uint64_t n) {
    constexpr uint64_t limit = 1ull << 62;
    if (first > limit || n > limit - first) return fail(BBB_EINVAL, "first_sample + nsamples must be <= 2^62");
    return BBB_OK;
}

// Timing-experiment knobs (kernel variants selected through the environment) exist only in builds made with
// -DBBB_EXPERIMENTS; the shipped library ignores the environment: no variable can change what it computes.
#ifdef BBB_EXPERIMENTS
inline int env_knob(const char *name, int dflt) {
    const char *v = std::getenv(name);
    return v ? std::atoi(v) : dflt;
}
#else
constexpr int env_knob(const char *, int dflt) { return dflt; }
#endif

// ---- PRBS entry points implemented in prbs_kernels.hip -------------------------------------
int prbs_fill_launch(int k, uint64_t init_state, uint64_t first_bit, uint64_t nbits,
                     uint64_t *dst, hipStream_t st, int nt_stores = 0);
int prbs_check_launch(int k, uint64_t init_state, uint64_t first_bit, uint64_t nbits,
                      const uint64_t *src, uint64_t *nerr_dev, hipStream_t st);
int prbs_detector_launch(int k, const uint8_t *bits, uint64_t nstreams, uint64_t n, uint8_t *err,
                         uint8_t *reload, hipStream_t st);

// detector_kernels.hip
int prbs_detector_stream_launch(int k, const uint64_t *src, uint64_t nbits, uint64_t *err, uint64_t *reload,
                                bbb_detector_stats *stats, uint64_t chunk_bits, uint64_t warm_bits, hipStream_t st);

// search_kernels.hip
int lutopt_search_launch(int k, uint64_t seed, uint64_t first, uint64_t count, uint64_t *found, uint16_t *taps_out,
                         uint32_t *row_off_out, bbb_search_stats *stats, hipStream_t st);

// eye_kernels.hip
struct EyeLaunch {
    uint32_t ncols, shift;
    uint64_t col_origin;
    int32_t threshold, strict;
    const unsigned long long *bits;   // data bits bit0 .. bit0 + nbits - 1 (packed LSB first); nullptr: no bathtub
    long long bit0;
    unsigned long long nbits;
    int pulser;                       // 1: the Pulser's bits ((m & 255) == 0), `bits` unused
    int want_hist, want_tub;
};
// blocks the accumulate kernel runs with on the current device for launches of up to nsamples (or a negative BBB_E* code),
// and the u32 words of scratch they need for ncols
int eye_grid_blocks(uint64_t nsamples);
int eye_cfg_check(const bbb_eye_cfg *eye);        // eye_api.hip: the rules of bbb_eye_cfg (BBB_EINVAL with a detail)
inline uint64_t eye_scratch_words(int blocks, uint32_t ncols) { return (uint64_t)blocks * (256u * ncols + 8u); }
int eye_accumulate_launch(const EyeLaunch &a, const int16_t *samples, uint64_t nsamples, uint64_t first_sample,
                          uint32_t *scratch, int blocks, uint64_t *hist, uint64_t *bathtub, hipStream_t st);
// the bits whose eight phase samples 8m + BBB_TX_BIT_SAMPLE0 + p meet samples [first, first + n), and the u64 words that hold
// those of any chunk of up to `chunk` samples: at most chunk / 8 + 1 bits
inline BitRange eye_bit_range(uint64_t first, uint64_t n) {
    return {floor8((int64_t)first - BBB_TX_BIT_SAMPLE0), floor8((int64_t)(first + n - 1) - BBB_TX_BIT_SAMPLE0)};
}
inline uint64_t eye_bits_words(uint64_t chunk) { return (chunk / 8 + 2) / 64 + 3; }

// txsweep_kernels.hip: the BER sweep over transmitter settings (include/bbb.h, bbb_tx_ber_sweep_*)
constexpr int kSweepMaxPairs = 8;                 // settings per launch: two per packed 16-bit lane operation
struct SweepGroup {                               // one launch: settings sharing one shaped-value table
    int table;                                    // index into the object's tables
    int pairs;                                    // 1..kSweepMaxPairs
    bool thr;                                     // some threshold of the group is not 0 after the strict shift
    uint32_t nv2[kSweepMaxPairs], t0[kSweepMaxPairs], t1[kSweepMaxPairs];    // packed (low: setting 2k, high: 2k + 1)
    int32_t idx[2 * kSweepMaxPairs];              // the settings' indices into the counters, -1 for padding
};
struct SweepChunk {                               // what a chunk hands every launch
    const int8_t *noise;                          // noise of the chunk's samples, nullptr: no setting has noise on
    const unsigned long long *bits;               // data bits m0 .. m0 + navail - 1; nullptr for the Pulser
    long long m0;
    unsigned long long navail;
    int source;                                   // 0 PRBS, 1 Pulser
    uint64_t first, n;                            // the chunk's samples [first, first + n), n <= 2^31
};
// the tables (8 x 256 u16 each) of ntab coefficient sets coeffs[ntab][64], built on the device once
int sweep_tables_launch(const int16_t *coeffs_dev, int ntab, uint16_t *tables, hipStream_t st);
// blocks a sweep launch runs with for up to n samples (or a negative BBB_E* code), and its scratch in u32 words
int sweep_grid_blocks(uint64_t n);
inline uint64_t sweep_scratch_words(int blocks) { return (uint64_t)blocks * (2 * kSweepMaxPairs * 8); }
int sweep_launch(const SweepGroup &g, const uint16_t *tables, const SweepChunk &c, uint32_t *scratch, int blocks,
                 uint64_t *counters, hipStream_t st);
// sample n needs the shaper window, bits M-7 .. M with M = floor((n - 17) / 8), and the window of a chunk's last thread reads
// 2 more: at most chunk / 8 + 10 bits
inline BitRange sweep_bit_range(uint64_t first, uint64_t n) {
    return {floor8((int64_t)first - 17) - 7, floor8((int64_t)(first + n - 1) - 17) + 2};
}
inline uint64_t sweep_bits_words(uint64_t chunk) { return (chunk / 8 + 16) / 64 + 2; }

// acf_kernels.hip: the autocorrelation counters (include/bbb.h, bbb_acf_accumulate_i16 / bbb_tx_acf_*)
struct AcfPlan {
    int gx, gy;                                   // workgroups over the stages (gx < 0: the device could not be queried)
    size_t smem;                                  // dynamic LDS per workgroup
    uint64_t partial_words, scratch_words;        // u64 words of the partials slab; of all scratch (slab, count, list)
};
// the grid of launches of up to max_nfirst first elements at nlags on the current device
AcfPlan acf_plan(uint32_t nlags, uint64_t max_nfirst);
int acf_launch(const AcfPlan &p, const int16_t *samples, uint64_t nfirst, uint64_t navail, uint32_t nlags, uint64_t *scratch,
               uint64_t *acf, hipStream_t st);

// nco_kernels.hip: the numerically controlled oscillator (include/bbb.h, bbb_nco_*)
constexpr int kNcoThreads = 512;                  // threads per workgroup
constexpr int kNcoReps = 16;                      // replicas of the ROM in LDS (lane l reads replica l % 16)
constexpr int kNcoScanSteps = 4;                  // workgroup steps of 4096 samples per tile of the fm scan
struct NcoLaunch {                                // one launch: up to 2^31 samples from the state in *in
    const int32_t *fm;                            // per-sample buffers (nullptr: the constant below)
    const uint16_t *am;
    const int16_t *pm;
    int16_t *x;
    uint64_t n;
    uint32_t fcw, am_c;
    int32_t fm_c, pm_c;
    int vec;                                      // every buffer given is 16-byte aligned: 16-byte loads and stores
    const int16_t *rom;                           // the 1024 ROM entries on the device
    const bbb_nco_state *in;                      // the state before the launch ...
    bbb_nco_state *out;                           // ... and after it (another slot)
    uint32_t *tiles;                              // fm scan: nco_tiles(n) tile sums, then offsets
};
uint64_t nco_tiles(uint64_t n);
int nco_launch(const NcoLaunch &a, int grid, hipStream_t st);
int nco_put_state(const bbb_nco_state &s, bbb_nco_state *dst, hipStream_t st);   // one thread, a plain store

// sinc_kernels.hip: the 16x sinc interpolator (include/bbb.h, bbb_sinc_*)
struct SincLaunch {                               // one launch: any number of input samples (64-bit indices)
    const void *in;                               // int8 or int16 samples; in[-1] .. in[-nbefore] readable
    void *out;                                    // 16 n elements of int8 or int16
    uint64_t n;
    uint32_t nbefore;                             // 0..7
    uint32_t shift;                               // int16 input: x8 = clamp(x >> shift, -128, 127)
    int vec;                                      // out is 16-byte aligned: 16-byte stores
    uint32_t words[32];                           // the table as the reference's BRAM words (sinc.py:42-48)
};
int sinc_launch(const SincLaunch &a, bool in16, bool out16, int grid, hipStream_t st);

// fir_kernels.hip: the exact integer FIR filter (include/bbb.h, bbb_fir_*)
constexpr int kFirTile = 2048;                    // input samples per workgroup step
struct FirLaunch {                                // one launch: any number of input samples (64-bit indices)
    const int16_t *in;                            // in[-1] .. in[-nbefore] readable
    void *out;                                    // nout int16 or int32, or ceil(nout / 64) zeroed u64 words of decisions
    uint64_t nin, nout;
    uint32_t nbefore;                             // 0 .. ntaps - 1
    uint32_t ngroups;                             // groups of four tap words (eight taps) in use: 1..32
    uint32_t shift, decim, phase;
    int32_t threshold;
    int strict;
    int in_vec, out_vec;                          // in / out is 16-byte aligned: 16-byte loads / stores
    uint32_t taps[BBB_FIR_MAX_TAPS / 2];          // word p = h[2p + 1] | h[2p] << 16, zero beyond ntaps
};
// mode 0: int16 out (saturating), 1: int32 out, 2: packed decisions against threshold
int fir_launch(const FirLaunch &a, int mode, int grid, hipStream_t st);
// fir_api.hip: the rules of bbb_fir_cfg (BBB_EINVAL with a detail); slice: shift and out_bytes are not looked at
int fir_cfg_check(const bbb_fir_cfg *c, bool slice);
// ... and its taps as the kernels' packed words (zeroed first; returns the groups of four words in use)
uint32_t fir_pack_taps(const bbb_fir_cfg *c, uint32_t words[BBB_FIR_MAX_TAPS / 2]);

// ddc_kernels.hip: the digital down-converter (include/bbb.h, bbb_ddc_run)
struct DdcLaunch {                                // one launch: any number of input samples; in .. in_vec, taps as FirLaunch
    const int16_t *in;
    void *out;                                    // nout pairs of 4 bytes (IQ16, POLAR) or 8 bytes (IQ32)
    uint64_t nin, nout;
    uint32_t nbefore, ngroups, shift, decim, phase;
    uint32_t first;                               // the absolute number of in[0]; its low 24 bits count
    uint32_t fcw, pa0;
    int in_vec, out_vec;
    uint32_t taps[BBB_FIR_MAX_TAPS / 2];
    int16_t rom[1024];                            // bbb_nco_rom: travels with the launch, so the oscillator has no device state
};
// mode: BBB_DDC_IQ16 / IQ32 / POLAR; cus: the device's compute units (the grid is what their LDS holds at once)
int ddc_launch(const DdcLaunch &a, int mode, int cus, hipStream_t st);

// link_kernels.hip: eye and bathtub of the shaped link behind a receive filter (include/bbb.h, bbb_link_sweep_*)
constexpr int kLinkTile = 2048;                   // outputs per workgroup step
constexpr uint64_t kLinkLaunchMax = 1ull << 31;   // samples per launch
struct LinkLaunch {                               // one launch: one setting over one chunk; j is a WAVEFORM sample number
    const int8_t *noise;                          // noise[i] belongs to sample norg + i, i < nnoise; nullptr: the noise is off
    long long norg;                               // >= 0; tb - norg is a multiple of 8
    unsigned long long nnoise;                    // a multiple of 8, all readable
    const unsigned long long *bits;               // data bits from m0 on, nwords u64 words readable; nullptr for the Pulser
    long long m0;                                 // 0, or at most the lowest bit the launch looks at
    unsigned long long nwords;
    int source;                                   // 0 PRBS, 1 Pulser
    int nv;                                       // noise_var, 0 when the noise is off
    const uint16_t *table;                        // the setting's shaped values as sweep_tables_launch leaves them
    long long tb;                                 // sample of the first tile's first output: out_lo - 7 <= tb <= out_lo
    long long out_lo, out_hi;                     // the outputs that count: stream samples [out_lo - delay, out_hi - delay)
    uint32_t delay;
    uint32_t ngroups;                             // groups of four tap words (eight taps) in use: 1..32
    uint32_t shift;                               // z = sat16(acc >> shift)
    int32_t threshold;                            // in units of acc
    int strict;
    uint32_t ncols, eye_shift;                    // the histogram's bbb_eye_cfg fields
    uint64_t col_origin;
    uint32_t taps[BBB_FIR_MAX_TAPS / 2];          // as FirLaunch
};
// blocks a launch may use on the current device (or a negative BBB_E* code); its scratch is eye_scratch_words(blocks, ncols)
int link_grid_blocks(bool hist);
// counters[8][2] and hist[256][ncols] += what stream samples [first, first + n) of the launch give; either may be nullptr
int link_launch(const LinkLaunch &a, bool hist, uint64_t first, uint64_t n, uint32_t *scratch, int blocks, uint64_t *hist_out,
                uint64_t *counters, hipStream_t st);
// a launch whose first tile starts at tb and whose filter reaches `lead` samples back, with outputs up to out_hi: a thread
// looks at the 10 bits of its shaper window and up to 47 bits below them, where the decided bits lie.  One of the words is
// slack behind the last bit (LinkLaunch::nwords, all readable).
inline BitRange link_bit_range(int64_t tb, int64_t lead, int64_t out_hi) {
    return {floor8(std::max<int64_t>(0, tb - lead) - 17) - 47, floor8(out_hi - 1 - 17) + 2};
}
inline uint64_t link_bits_words(uint64_t chunk) { return (chunk / 8 + 160) / 64 + 4; }

// bbb_api.hip: what the eye object needs of a handle (reads fields only) and the bbb_tx_cfg checks of bbb_tx_fill_i16
int lutopt_device(const bbb_lutopt *h);
hipStream_t lutopt_stream(const bbb_lutopt *h);
int tx_cfg_check(const bbb_tx_cfg *cfg);
// ... and what bbb_awgn_hist needs: two more fields, and the staged sample kernel of a range with the caller's kernel as the reader
// of its staging slot (`visit` queues that kernel on the stream it is given; the scheduler's events stay in bbb_api.hip)
int lutopt_k(const bbb_lutopt *h);
int lutopt_staged_level(const bbb_lutopt *h);
typedef int (*lutopt_stage_visitor)(void *ctx, const void *stage, uint64_t nsamples, unsigned L, uint64_t G, unsigned nlanes, hipStream_t st);
int lutopt_stage_visit(bbb_lutopt *h, uint64_t nsamples, uint64_t first_step, lutopt_stage_visitor visit, void *ctx);

// hist_kernels.hip: the histogram of the CLTGRNG samples (include/bbb.h, bbb_awgn_hist)
constexpr unsigned kHistMaxBins = 512;
// blocks a histogram launch may use on the current device (or a negative BBB_E* code); the scratch is blocks x nbins u32
int hist_grid_blocks();
// bins the samples [0, nsamples) of the count planes a staged sample kernel left (256 bins), one partial per block
int hist_planes_launch(const void *stage, uint64_t nsamples, unsigned L, unsigned nlanes, uint32_t *scratch, int blocks, unsigned *used,
                       hipStream_t st);
// bins int8 (elem 1) or int16 (elem 2) samples of a k-bin generator: bin = (x + nbins / 2) mod nbins; nsamples <= 2^31
int hist_samples_launch(const void *samples, int elem, uint64_t nsamples, unsigned nbins, uint32_t *scratch, int blocks, unsigned *used,
                        hipStream_t st);
// hist[b] += the `used` partials
int hist_reduce_launch(const uint32_t *scratch, unsigned used, unsigned nbins, uint64_t *hist, hipStream_t st);

// errstat_kernels.hip: gap, burst and errored-block statistics of a packed error stream (include/bbb.h, bbb_errstat_*)
constexpr uint64_t kErrWaveBits = 65536;          // one wavefront: 8 steps of 64 lanes x 2 words
constexpr uint64_t kErrTileBits = 4 * kErrWaveBits;   // one workgroup of 4 wavefronts
constexpr uint64_t kErrLaunchBits = 1ull << 34;   // bits per launch: 65536 tile summaries
struct ErrLaunch {                                // one launch: nbits <= kErrLaunchBits from the position in res->bits
    const uint64_t *err, *mask;                   // mask may be nullptr
    uint64_t nbits;
    uint32_t guard, nblock;
    uint64_t block[4];                            // the first nblock in use; 0: unused entry
    int vec;                                      // err and mask are 16-byte aligned: 16-byte loads
};
size_t errstat_scratch_bytes();                   // the tile summaries of one launch
// the tile kernel and the stitch behind it: counters and carried state in *res (device) move on by nbits
int errstat_launch(const ErrLaunch &a, bbb_errstat_result *res, void *scratch, hipStream_t st);
int errstat_skip_launch(bbb_errstat_result *res, uint64_t nbits, hipStream_t st);   // one thread: res->bits += nbits

// xcorr_kernels.hip: the correlation of samples with their data bits (include/bbb.h, bbb_xcorr_accumulate_i16 / bbb_tx_xcorr_*)
struct XcorrPlan {
    int gx, gy;                                   // workgroups over the tiles (gx < 0: the device could not be queried), over the lag groups
    int xt;                                       // lag groups per lane: 8, 16 or 32
    uint32_t lw;                                  // lags per row of the grid: xt * spb
    uint64_t scratch_words;                       // u64 words of the partials slab
};
struct XcorrLaunch {                              // one launch: the arguments of bbb_xcorr_accumulate_i16, checked
    const int16_t *samples;
    uint64_t nsamples, first_sample;
    const uint64_t *bits;
    uint64_t bit0, nbits;
    uint32_t spb, nlags;
    uint64_t origin;
};
// the grid of launches of up to max_nsamples samples at spb and nlags on the current device
XcorrPlan xcorr_plan(uint32_t spb, uint32_t nlags, uint64_t max_nsamples);
int xcorr_launch(const XcorrPlan &p, const XcorrLaunch &l, uint64_t *scratch, int64_t *xc, hipStream_t st);
// the Pulser's data bits first_bit .. first_bit + 64 nwords - 1, packed as bbb_prbs_fill packs
int xcorr_pulser_bits_launch(uint64_t *dst, uint64_t first_bit, uint64_t nwords, hipStream_t st);
// the data bits samples [first, first + n) need, n > 0, already clamped at bit 0 (the capture side compares against them);
// the words of a transmitter chunk (spb 8): at most (chunk + nlags - 1) / 8 + 2 bits
inline BitRange xcorr_bit_range(uint64_t first, uint64_t n, const bbb_xcorr_cfg &c) {
    const int64_t f = (int64_t)first - (int64_t)c.origin;
    return {std::max<int64_t>(0, floor_div(f - (int64_t)(c.nlags - 1), c.spb)), floor_div(f + (int64_t)n - 1, c.spb)};
}
inline uint64_t xcorr_bits_words(uint64_t chunk, uint32_t nlags) { return ((chunk + nlags) / 8 + 2) / 64 + 3; }

}  // namespace bbb
