/*
 * bbb.h -- C ABI of libbbb_hip.so: the MI355X (gfx950) implementation of basebandboard's
 * AWGN / PRBS Monte-Carlo path.
 *
 * The reference has no FFI for this path (it is migen gateware plus one numpy script),
 * so each entry point below names the reference interface whose semantics it carries;
 * paths are relative to the reference checkout.  A host in any language binds these
 * directly (INTEGRATION.md shows the ctypes and Rust `extern "C"` stubs).
 *
 * Conventions
 *  - plain C types only; every function returns BBB_OK (0) or a negative BBB_E* code;
 *    nothing throws across the boundary.  bbb_strerror() names a code,
 *    bbb_last_error_detail() gives the failing HIP call of the calling thread.
 *  - pointers named *_dev are device memory on the handle's / call's device (hipMalloc or
 *    a torch tensor's data_ptr()); all other pointers are host memory.
 *  - work is enqueued on the given hipStream_t (passed as void*; NULL = default stream)
 *    and is asynchronous unless the function returns a result to host memory.
 *  - there is NO CPU execution path: a call without a usable gfx950 device fails with
 *    BBB_ENODEV.
 *  - a handle is not thread-safe; different handles may be used from different threads.
 *  - bit order: state bit i of a k-bit state is word[i/64] >> (i%64) & 1, the bit order of
 *    the HDL integer (gateware/bbb/rng.py:135); packed PRBS bit t is word[t/64] >> (t%64) & 1.
 */
#ifndef BBB_H
#define BBB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BBB_OK        0
#define BBB_EINVAL   -1   /* bad argument; includes "k invalid for PRBS" (prbs.py:29-30, 55-56) */
#define BBB_ENOMEM   -2
#define BBB_EHIP     -3   /* a HIP runtime call failed */
#define BBB_EIO      -4   /* matrix file unreadable / malformed */
#define BBB_ENODEV   -5   /* no gfx950 device available */
#define BBB_EUNSUP   -6   /* valid request this build has no kernel for */

#define BBB_ABI_VERSION 1
#define BBB_MAX_K 512

int bbb_abi_version(void);
const char *bbb_strerror(int code);
const char *bbb_last_error_detail(void);
int bbb_device_count(int *count);
/* free() for buffers returned by bbb_lutopt_load_matrix_file */
void bbb_free(void *p);

/* ---- uniform + Gaussian generator: LUTOPT -> CLTGRNG ------------------------------------ */

typedef struct bbb_lutopt bbb_lutopt;

/* Read a recurrence matrix in the text format of software/rnghunt/matrices/N (N lines of N
 * chars '0'/'1', line r char c = A[r][c]; written by software/rnghunt/src/bin/rnghunt.rs:51-53,
 * read by software/rnghunt/util/pack.py:6-18) into packed tap lists: row r's taps are
 * taps[row_off[r] .. row_off[r+1]) -- the `packed` argument of LUTOPT.from_packed
 * (gateware/bbb/rng.py:42-55).  Caller frees *taps and *row_off with bbb_free. */
int bbb_lutopt_load_matrix_file(const char *path, int *k, uint16_t **taps, uint32_t **row_off);

/* LUTOPT(a, init) / LUTOPT.from_packed(packed, init): gateware/bbb/rng.py:21-55.
 * Any k in [2, 512] (LUTOPT puts no constraint on k; gateware/bbb/rng_recurrences.py:105 ships n192,
 * rnghunt searches n = 192: rnghunt.rs:14); every row 1..8 taps.  Only the CLTGRNG entry points
 * (bbb_awgn_fill_*, bbb_tx_fill_i16 with noise) need k to be a power of two (rng.py:72-76) and
 * return BBB_EUNSUP otherwise.
 * init_words = ceil(k/64) words; the reference default is 1 (bit 0 set, rng.py:21).
 * device = -1 makes a host-only handle: bbb_lutopt_state_at works (pure GF(2) algebra), every
 * compute call on it returns BBB_ENODEV. */
int bbb_lutopt_create(bbb_lutopt **h, int k, const uint16_t *taps, const uint32_t *row_off,
                      const uint64_t *init_words, int device);
int bbb_lutopt_destroy(bbb_lutopt *h);
/* Bind the handle to a HIP stream (NULL = the default stream): every later call is ordered on it like a kernel launch -- behind what the
 * caller had queued there, in front of what the caller queues next.  The library orders ITS OWN work across a re-bind (kernels, staging
 * slots, start-state buffers of earlier calls, whichever stream they were made on).  The CALLER's work is the caller's to order, as with
 * any stream-ordered library: a buffer that was filled, or is still being read, under one stream must not be handed to a call under
 * another stream without an event between the two (tests/test_gpu_staged.py's random mix does exactly that). */
int bbb_lutopt_set_stream(bbb_lutopt *h, void *hip_stream);
/* 1 when the handle runs the generated straight-line kernel (the n256 matrix of
 * gateware/bbb/rng_recurrences.py:172-259 used by tx.py:70), 0 for the table-driven one. */
int bbb_lutopt_is_specialised(const bbb_lutopt *h);

/* Device-side timing of the generator kernels with hipEvents recorded on the handle's stream
 * around every bbb_awgn_fill_i8 of a specialised handle: [start, seeding kernels, sample kernel].
 * bbb_lutopt_profile_read waits for the recorded events and returns the accumulated
 * milliseconds (seeding / sample kernel) and the number of calls; reset != 0 clears the sums.
 * A sample kernel that is dispatched while the previous one still holds the machine (the staged form with announced
 * start states) is counted from that kernel's completion, not from its own dispatch: time on the machine. */
int bbb_lutopt_profile(bbb_lutopt *h, int enable);
int bbb_lutopt_profile_read(bbb_lutopt *h, double *seed_ms, double *kernel_ms, uint64_t *calls, int reset);
/* The same for the second kernel of the two-kernel form (the mover): accumulated milliseconds
 * and number of movers since the last reset. */
int bbb_lutopt_profile_read_mover(bbb_lutopt *h, double *mover_ms, uint64_t *calls, int reset);

/* LUTOPT.x after `nsteps` clocks from reset (rng.py:38-40), by GF(2) jump-ahead
 * (the x' = A x algebra of software/rnghunt/src/binary_matrix.rs:53-76). Host result. */
int bbb_lutopt_state_at(bbb_lutopt *h, uint64_t nsteps, uint64_t *state_words);

/* LUTOPT.x in bulk -- the uniform word stream itself (rng.py:29-40: "outputs x ... on each clock"; the
 * reference dumps it for dieharder in software/rnghunt/util/verify.py:37-52, 200 000 states as 32-bit
 * words).  State A^(first_step + i + 1) init, 0 <= i < nstates, as k/32 consecutive words:
 *   dst_dev[i * (k/32) + j] = state bits 32j .. 32j+31,
 *   msb_first = 0: bit 32j is the LSB (the HDL integer of rng.py:135, little-endian words);
 *   msb_first = 1: bit 32j is the MSB (verify.py:46-52 prints x[0] x[1] ... and reads 32 characters as a
 *                  binary number) -- the words of its `outnums` file in order.
 * k must be a multiple of 32.  Asynchronous on the handle's stream. */
int bbb_lutopt_fill_words(bbb_lutopt *h, uint32_t *dst_dev, uint64_t nstates, uint64_t first_step, int msb_first);

/* The CLTGRNG sample stream (gateware/bbb/rng.py:70-108; tx.py:70-71):
 *   dst_dev[i] = trunc_signed_log2k( tree( A^(first_step + i + 1) * init ) ),  0 <= i < nsamples
 * i.e. sample i is the adder-tree value of the LUTOPT state after first_step+i+1 clocks,
 * exactly the sequential stream a single CLTGRNG emits (pipeline delay removed).
 * Output is int8 (for k = 256: -128..127, +128 wraps to -128 as the 8-bit Signal does).
 * dst_dev must be 16-byte aligned.  Asynchronous on the handle's stream. */
int bbb_awgn_fill_i8(bbb_lutopt *h, int8_t *dst_dev, uint64_t nsamples, uint64_t first_step);
/* Optional hint: the NEXT bbb_awgn_fill_i8 on this handle will ask for exactly (nsamples, first_step).
 * The start states of that fill are then derived right away on an internal side stream -- the small
 * seeding kernels fit beside the running sample kernel (which leaves ~110 registers per SIMD and
 * 32 KiB of LDS per CU unused) -- and the matching fill only waits for them.  A fill with other
 * arguments ignores the hint.  Results are identical with or without it. */
int bbb_awgn_prefetch(bbb_lutopt *h, uint64_t nsamples, uint64_t first_step);
/* Choose the two-kernel ("staged") form of the k = 256 sample stream for this handle's large fills
 * (bbb_awgn_fill_i8, bbb_tx_fill_i16 of 2^24 samples and more).  Results are identical; what changes is how the
 * bytes reach HBM.  The one-kernel form writes every generator's 16 new bytes straight to their place: 62.5 M
 * scattered pieces per 1e9 samples, one DRAM row activation each.  The staged form has the sample kernel leave its
 * pieces in an internal buffer as full lines and a second kernel move them with full-line reads and writes.  That
 * second kernel runs on the caller's stream, which first waits for the sample kernel (on an internal stream): anything
 * queued after the call sees the output complete, as before; but the NEXT fill's arithmetic does not wait for it -- the
 * mover (memory bound) and the next
 * arithmetic (integer-issue bound) share the machine.  Worth it for back-to-back fills; a single isolated fill
 * finishes later than in the one-kernel form.  Costs two staging buffers of the fill's size.
 * enable = m in 2..8 adds LOOK-AHEAD for bbb_awgn_fill_i8 (and for bbb_tx_fill_i16 with noise on this handle, while the
 * configuration stays the same and m n < 2^34): a fill of n samples at `first` lets its sample kernel produce
 * the m n samples from `first` (one seeding, one launch for m fills; the rest waits in the staging buffer); while the
 * following fills ask for exactly (n, first + n), (n, first + 2 n) ... -- a consumer reading the one sequential stream
 * the reference's generator emits -- each only costs its piece mover.  A fill elsewhere discards what still waits (that
 * work was wasted).  Staging buffers are m times as large.  Results are identical in every mode; calling this function
 * (with any value) drops whatever waits. */
int bbb_lutopt_set_staged(bbb_lutopt *h, int enable);
/* Same stream as int16 (needed for k = 512, whose CLTGRNG output is 9 bits: rng.py:78). */
int bbb_awgn_fill_i16(bbb_lutopt *h, int16_t *dst_dev, uint64_t nsamples, uint64_t first_step);

/* The sample stream as an OBJECT that is drained sequentially -- what a CLTGRNG is: one value per clock, in order
 * (gateware/bbb/rng.py:70-108; tx.py:70-71 is its only consumer).  The stream owns everything a fast sequential reader
 * would otherwise have to choreograph with bbb_lutopt_set_staged / bbb_awgn_prefetch: it turns the two-kernel form on
 * for the handle (with two reads per sample kernel, level 2 of bbb_lutopt_set_staged, unless the caller had chosen a
 * level: staging then takes 4 bytes per sample of a read), announces every next read itself (so the start states are
 * derived beside the running kernel) and restores the handle's mode when it is closed.  A host simply calls
 * bbb_awgn_stream_next in a loop.
 *   open   nsamples_per_call = the length bbb_awgn_stream_next delivers (and the length the stream prepares for);
 *          first_step = LUTOPT clocks before the first sample, as in bbb_awgn_fill_i8; elem_bytes 1 (int8, k <= 256)
 *          or 2 (int16).  One stream per handle at a time (BBB_EINVAL otherwise); the handle must outlive it.
 *   next   the next nsamples_per_call samples to dst_dev (16-byte aligned, elem_bytes * nsamples_per_call bytes),
 *          asynchronous on the handle's stream like bbb_awgn_fill_i8.
 *   read   the next `nsamples` samples, any length (a ragged tail, a short probe): the stream continues behind them.
 *   seek   continue at another position (what was produced ahead at the old one is dropped, the next read announced there).
 *   tell   *next_step = clocks before the sample the next read starts with.
 * Other calls on the handle between two reads are allowed (they cost the pending announcement at most).  Every byte is
 * the one bbb_awgn_fill_i8 / _i16 would deliver for the same position. */
typedef struct bbb_awgn_stream bbb_awgn_stream;
int bbb_awgn_stream_open(bbb_lutopt *h, uint64_t nsamples_per_call, uint64_t first_step, int elem_bytes, bbb_awgn_stream **s);
int bbb_awgn_stream_next(bbb_awgn_stream *s, void *dst_dev);
int bbb_awgn_stream_read(bbb_awgn_stream *s, void *dst_dev, uint64_t nsamples);
int bbb_awgn_stream_seek(bbb_awgn_stream *s, uint64_t first_step);
int bbb_awgn_stream_tell(const bbb_awgn_stream *s, uint64_t *next_step);
int bbb_awgn_stream_close(bbb_awgn_stream *s);

/* The HISTOGRAM of the sample stream -- the counting half of software/clt-grng/clt-grng-evaluate.py:18-50, over a range of
 * the stream instead of 100 000 draws, without the samples ever being handed to the caller:
 *   for every i < nsamples:  hist_dev[x_i + k/2] += 1,   x_i = the sample bbb_awgn_fill_i8 / _i16 delivers at position i of
 *                                                         (nsamples, first_step)
 * hist_dev: k uint64 device counters (256 for the n256 generator, 512 for n512), 8-byte aligned.  The bin is that of the
 * DELIVERED, truncated sample: the tree value +k/2 lands in bin 0, as the log2(k)-bit Signal wraps it to -k/2.
 * The call ADDS into the counters (as bbb_eye_accumulate_i16): a range may be cut into calls at any point, and a multi-GPU
 * host reduces the counters with one collective.  Any nsamples (0: nothing is done) and any first_step; a long range is cut
 * into launches internally, so that every partial count is exact.  Asynchronous on the handle's stream, ordered like a fill;
 * the handle's staging mode is the same after the call as before (a look-ahead half that waited is dropped, as by
 * bbb_lutopt_set_staged).  On the shipped n256 matrix pieces of 2^24 samples and more are counted by a guest kernel beside
 * the sample kernel, straight from its staging buffer (two buffers of up to 1 GiB); every other generator fills an internal
 * buffer of at most 2^26 samples and counts that.
 * Errors: BBB_EUNSUP where k is not a power of two, BBB_ENODEV on a host-only handle, BBB_EINVAL for a null or misaligned
 * pointer. */
int bbb_awgn_hist(bbb_lutopt *h, uint64_t *hist_dev, uint64_t nsamples, uint64_t first_step);

/* CLTGRNG adder tree on caller-supplied uniform words (the loop body of
 * software/clt-grng/clt-grng-evaluate.py:8-16): states_dev holds nstates states of
 * ceil(k/64) u64 words each; out_dev[i] = un-truncated tree value (int16). */
int bbb_clt_tree_i16(int k, const uint64_t *states_dev, uint64_t nstates, int16_t *out_dev,
                     int device, void *hip_stream);

/* ---- PRBS generator / checker ---------------------------------------------------------- */

/* PRBS(k).x (gateware/bbb/prbs.py:23-35; TAPS prbs.py:14): bits first_bit .. first_bit+nbits-1
 * of the sequence started from LFSR state init_state (reference reset value 1), packed
 * LSB-first into u64 words.  Writes ceil(nbits/64) words; unused high bits of the last
 * word are zero.  dst_dev must be 16-byte aligned. */
int bbb_prbs_fill(int k, uint64_t init_state, uint64_t first_bit, uint64_t nbits,
                  uint64_t *dst_packed_dev, int device, void *hip_stream);
/* The same fill with a hint about what the caller does next.  BBB_PRBS_WILL_READ_BACK: the buffer is about to be read
 * back (a loopback: bbb_prbs_check / bbb_prbs_detector_stream right behind the fill).  The generator then writes with
 * non-temporal stores: the fill itself takes ~15 % longer, but it leaves no dirty lines in the memory-side cache for the
 * reader to write back, and fill + check together finish sooner.  Same bits either way. */
#define BBB_PRBS_WILL_READ_BACK 1u
int bbb_prbs_fill_hint(int k, uint64_t init_state, uint64_t first_bit, uint64_t nbits,
                       uint64_t *dst_packed_dev, unsigned flags, int device, void *hip_stream);
/* Phase-known checker: number of positions where src differs from the same PRBS.  This is
 * the steady-state (`reload == 0`) behaviour of PRBSErrorDetector.err (prbs.py:79) summed
 * over the stream.  *nerr is a host result (the call synchronises the stream). */
int bbb_prbs_check(int k, uint64_t init_state, uint64_t first_bit, uint64_t nbits,
                   const uint64_t *src_packed_dev, uint64_t *nerr, int device, void *hip_stream);
/* Same, accumulating into a device counter (no synchronisation): *nerr_dev += mismatches. */
int bbb_prbs_check_dev(int k, uint64_t init_state, uint64_t first_bit, uint64_t nbits,
                       const uint64_t *src_packed_dev, uint64_t *nerr_dev, int device,
                       void *hip_stream);
/* LFSR state after nbits clocks (prbs.py:35 iterated), by jump-ahead.  Host result. */
int bbb_prbs_state_at(int k, uint64_t init_state, uint64_t nbits, uint64_t *state);

/* PRBSErrorDetector (gateware/bbb/prbs.py:43-99), cycle exact, for `nstreams` independent
 * detectors run in parallel (one per GPU lane).  bits_dev[s*n + i] is the input wire of
 * stream s during clock i (0/1); err_dev / reload_dev [s*n + i] are `err` and `reload`
 * sampled after that clock edge -- what the reference testbench reads (prbs.py:146-150).
 * Either output may be NULL. */
int bbb_prbs_detector_run(int k, const uint8_t *bits_dev, uint64_t nstreams, uint64_t n,
                          uint8_t *err_dev, uint8_t *reload_dev, int device, void *hip_stream);

/* The same detector over ONE long stream (chunked execution with state
 * hand-off).  bits_packed_dev: input wire during clock t at word t/64, bit t%64 (the layout
 * bbb_prbs_fill / bbb_rx_slice write).  err_packed_dev / reload_packed_dev (either may be NULL,
 * ceil(nbits/64) words): `err` / `reload` sampled after clock t, same packing.  The stream is cut
 * into chunks of chunk_bits (a multiple of 64; 0: chosen by the length -- 4096 ... 32768 bits up to 8.6e9 bits, beyond that
 * 512 ... 1024 words, whichever spreads the blocks of 256 chunks most evenly over the device's CUs: 640 words for 1e10 bits on
 * 256 CUs), each run by one GPU lane from a
 * speculative state obtained by running the reset detector over the warm_bits (0: 1024) before the
 * chunk; every chunk whose speculative start differs from its predecessor's true end state is run
 * again from that state until the chain is consistent, so the outputs equal the serial machine's
 * bit for bit (prbs.py:61-99).  (A re-run stops where its state meets the speculative run's: from there on the chunk
 * is what the first pass made of it.)  *stats is a host result (the call synchronises the stream).  The call's device
 * workspace (72 bytes per chunk: 22 MB at 1e10 bits; kept up to 256 MiB) and a pinned read-back buffer stay allocated
 * between calls, one set per device and concurrent call.
 * Alignment: the three pointers need 8 bytes, no more.  An input aligned to 16 bytes selects the sparse forms (k != 20: the
 * stream is classified at memory speed and the machine runs only where it has to); an input at 8 mod 16 bytes is run by the
 * dense pass, lane by lane -- the same result, several times slower.  The alignment of the outputs selects nothing. */
typedef struct {
    uint64_t bits;            /* clocks processed */
    uint64_t errors;          /* clocks with err == 1 and reload == 0 (what the reference test compares, prbs.py:152-163) */
    uint64_t errors_raw;      /* clocks with err == 1 */
    uint64_t reload_clocks;   /* clocks with reload == 1 */
    uint64_t resyncs;         /* times err_count exceeded k/2 (prbs.py:92), the reload out of reset included */
    uint64_t chunks;          /* execution detail: chunks, chunk re-runs needed, 1 if the serial guard ran */
    uint64_t chunks_rerun;
    uint64_t serial_fallback;
} bbb_detector_stats;
int bbb_prbs_detector_stream(int k, const uint64_t *bits_packed_dev, uint64_t nbits, uint64_t *err_packed_dev,
                             uint64_t *reload_packed_dev, bbb_detector_stats *stats, uint64_t chunk_bits,
                             uint64_t warm_bits, int device, void *hip_stream);

/* A sample kernel built for the handle's own matrix (one that is not among the shipped ones, e.g. a result of
 * bbb_lutopt_search): `fn` launches it on hip_stream for the bit-plane start states the library prepares
 * (planes_dev[p * nlanes + lane_global] = state bit p of 32 generators, the state BEFORE the first sample; generator
 * numbering and segment geometry as csrc/custom_fill_template.hip uses them) and returns 0 or a hipError_t.
 * bbb_awgn_fill_i8 then calls it instead of the table-driven kernel.  basebandboard_amd.LUTOPT.specialise() generates,
 * compiles (hipcc) and attaches such a kernel; fn == NULL detaches.  k must be a power of two <= 256. */
typedef int (*bbb_custom_fill_fn)(const uint32_t *planes_dev, int8_t *dst_dev, uint64_t nsamples, uint32_t L, uint64_t G,
                                  uint32_t nlanes, void *hip_stream);
int bbb_lutopt_set_custom_fill(bbb_lutopt *h, bbb_custom_fill_fn fn);
/* The same for the fused BER trial (k = 256 only): `trials` points at the library's internal per-trial records
 * (csrc/awgn_launch.hpp, TrialDev) and is passed through unchanged; returns 0 or a BBB_E* code.  Here planes_dev holds
 * the state OF the first sample (one clock further than for the sample kernel), and a continued trial (bbb_ber_run_*)
 * has the kernel write the states it ends in back to both buffers. */
typedef int (*bbb_custom_ber_fn)(uint32_t *planes_dev, uint32_t *prbs_planes_dev, const void *trials, int ncfg,
                                 uint32_t nlanes, uint64_t *counters_dev, void *hip_stream);
int bbb_lutopt_set_custom_ber(bbb_lutopt *h, bbb_custom_ber_fn fn);
/* Load a library built from csrc/custom_fill_template.hip for THIS handle's matrix (basebandboard_amd/
 * gen_lutopt_kernel.py <taps> custom_gen.inc; hipcc --offload-arch=gfx950 -shared -DBBB_N=k -DBBB_LOG=log2 k ...)
 * and attach what it exports: the sample kernel (bbb_custom_fill) and, for k = 256, the BER kernels
 * (bbb_custom_ber).  The C-ABI form of LUTOPT.specialise(): a host without Python generates and compiles the
 * library at build time and attaches it here.  The library stays loaded for the life of the process. */
int bbb_lutopt_attach_custom_library(bbb_lutopt *h, const char *path);

/* ---- fused Monte-Carlo trial: PRBS -> BPSK + scaled CLT noise -> slicer -> error count --- */

/* One trial.  Bit t (0 <= t < nbits) uses PRBS bit first_bit+t and the CLT sample of LUTOPT
 * state A^(warmup+first_bit+t+1) init; the channel is the TX noise path and RX slicer:
 *   noise = wrap12(sample * noise_var)            gateware/bbb/tx.py:75-77
 *   x     = wrap12((bit ? +amp : -amp) + noise)   gateware/bbb/tx.py:80-81
 *   bit^  = (x >= 0)                              gateware/bbb/rx.py:29
 * and an error is bit^ != bit.  The counters and the (amp, noise_var) <-> Eb/N0 mapping are
 * build-defined: the reference has neither. */
typedef struct {
    int32_t  prbs_k;       /* 7, 9, 11, 15, 20, 23 or 31 */
    int32_t  amp;          /* 0..2047 */
    int32_t  noise_var;    /* 0..15 (4-bit unsigned, tx.py:52) */
    int32_t  reserved;
    uint64_t prbs_state;   /* initial LFSR state, non-zero, < 2^k */
    uint64_t warmup;       /* LUTOPT clocks discarded first (rng.py:161-162 uses 2*log2 k) */
    uint64_t first_bit;
    uint64_t nbits;
} bbb_trial_cfg;

typedef struct { uint64_t bits, errors; } bbb_ber;

/* Run ncfg trials on the handle's generator; out[i] (host) receives trial i's counters. */
int bbb_ber_trials(bbb_lutopt *h, const bbb_trial_cfg *cfgs, int ncfg, bbb_ber *out);
/* Same, adding into device counters counters_dev[2*i] (bits), [2*i+1] (errors) without
 * synchronising -- the buffer a multi-GPU host hands to one RCCL all-reduce (ncclUint64, sum).
 * Calls queued back to back overlap: the start states of a trial (generators and PRBS) are derived on internal streams into
 * a second set of buffers while the kernel of the trial before runs on the handle's stream, and its kernel follows directly. */
int bbb_ber_trials_dev(bbb_lutopt *h, const bbb_trial_cfg *cfgs, int ncfg, uint64_t *counters_dev);

/* A trial group CONTINUED over several calls (round 4).  One bbb_ber_trials call spends 0.16 ms in front of its kernel on
 * the start states of 2 M generators, whatever its length; a Monte-Carlo run that keeps adding bits until it has seen
 * enough errors pays that per call.  Here a BLOCK of calls_per_block (m) calls shares ONE seeding: the block's m * nbits
 * bits are cut into the generators' segments once, call c runs the c-th m-th of every segment and the kernel leaves the
 * generators' and the PRBS states where the next call finds them (in buffers the run owns: other calls on the handle do
 * not disturb it).  cfgs: up to BBB_BER_MAX_GROUP settings that share prbs_k, prbs_state, warmup, first_bit and nbits
 * (= bits per call; single-threshold channels unless ncfg = 1) -- one pass over the noise stream serves all of them.
 * Block b covers bits [first_bit + b m nbits, first_bit + (b + 1) m nbits).  The (bit, sample) pairs of a block are
 * exactly those of one bbb_ber_trials call over it, visited in another order: after every m-th call the totals equal
 * that call's counters bit for bit (between block ends a call may count up to one segment fewer or more bits than
 * nbits; `bits` always says how many were counted).  The reference's counterpart is the free-running generator itself:
 * one LFSR, one LUTOPT, clocked for as long as the test lasts (gateware/bbb/tx.py:56-81, prbs.py:32-35).
 * _next: runs the next call on the handle's stream and returns the running totals of the whole run (host, synchronises;
 * totals may be NULL: no read-back, no synchronisation).  _next_dev: ADDS the call's counters to counters_dev
 * ([ncfg][2] uint64, device) without synchronising.  _tell: calls made so far / first bit of the next block to start.
 * LIFETIME: a run borrows its handle -- every call on the run, _close included, uses the handle's streams and plans: close
 * the run BEFORE bbb_lutopt_destroy of its handle (a run that outlives its handle is a use after free). */
typedef struct bbb_ber_run bbb_ber_run;
int bbb_ber_run_open(bbb_lutopt *h, const bbb_trial_cfg *cfgs, int ncfg, uint32_t calls_per_block, bbb_ber_run **out);
int bbb_ber_run_next(bbb_ber_run *r, bbb_ber *totals);
int bbb_ber_run_next_dev(bbb_ber_run *r, uint64_t *counters_dev);
int bbb_ber_run_tell(const bbb_ber_run *r, uint64_t *calls_done, uint64_t *next_block_first_bit);
int bbb_ber_run_close(bbb_ber_run *r);

/* The sweep sharded over the GPUs of ONE process (BASELINE.json configs[4]).  The
 * reference's only multi-worker program has this shape -- workers plus one channel back,
 * software/rnghunt/src/bin/rnghunt.rs:16-18,54-65 -- and no collective of its own; here the channel back is the
 * path's single collective.  handles[r] is a generator created on device r's GPU (all on distinct devices, same
 * matrix).  One host thread per device runs that device's share of the trials, then ONE
 * ncclAllReduce(ncclUint64, ncclSum) of the uint64[2 * ncfg] {bits, errors} counters over xGMI (RCCL,
 * ncclCommInitAll over the handles' devices; the communicators are cached per device list) leaves the totals on
 * every device; out[i] (host) receives them.  Integer sums: the result does not depend on ndev or on the order
 * of the reduction.  mode selects the share of rank r (bbb_sweep_shard computes it, host only):
 *   BBB_SHARD_TRIALS  trial i runs on rank i % ndev (independent trials, round robin);
 *   BBB_SHARD_SEEDS   every rank runs EVERY trial on its own handle -- give the handles different reset states
 *                     (seeds): the points x seeds form, N times the bits per point in the time of one sweep;
 *   BBB_SHARD_BITS    every rank runs every trial over ITS slice of the trial's bit range
 *                     [first_bit + r nbits / ndev, first_bit + (r+1) nbits / ndev) -- same reset state on all
 *                     handles; the totals equal the single-device counters of the same trials exactly;
 *   BBB_SHARD_GROUPS  consecutive trials that read the same noise and PRBS streams (same prbs_k, prbs_state, warmup,
 *                     first_bit, nbits: an Eb/N0 sweep on one seed) stay together -- group q runs on rank q % ndev, in one
 *                     pass over its streams as on one device.  The form of BASELINE configs[4]: 11 points x 8 seeds given
 *                     as 8 groups of 11 trials (the seeds as stretches of the one cycle: warmup = 16 + (s << 48)) is one
 *                     11-point sweep per device on eight devices and eight sweeps back to back on one; the totals do not
 *                     depend on ndev. */
#define BBB_SHARD_TRIALS 0
#define BBB_SHARD_SEEDS 1
#define BBB_SHARD_BITS 2
#define BBB_SHARD_GROUPS 3
int bbb_ber_sweep_multi(bbb_lutopt *const *handles, int ndev, const bbb_trial_cfg *cfgs, int ncfg, int mode,
                        bbb_ber *out);
/* The share of `rank` among `ndev`: mine[i] is trial i as that rank runs it (nbits = 0: not at all). */
int bbb_sweep_shard(const bbb_trial_cfg *cfgs, int ncfg, int ndev, int rank, int mode, bbb_trial_cfg *mine);
/* What the last bbb_ber_sweep_multi of this process ran on, for a caller (or a first multi-GPU run) that wants to check
 * itself: the number of handles it was given, the rank count the RCCL communicator reports (ncclCommCount), the file the
 * RCCL entry points were resolved from and whether that library was already mapped in the process (a PyTorch process holds
 * its own copy: it is reused, not loaded a second time). */
typedef struct {
    int32_t n_devices;      /* handles of the call */
    int32_t n_ranks_seen;   /* ncclCommCount of its communicator (0: no call yet) */
    int32_t rccl_reused;    /* 1: found with RTLD_NOLOAD */
    int32_t reserved;
    char    rccl_path[256];
} bbb_multi_info;
int bbb_multi_last_info(bbb_multi_info *out);
/* Destroy the cached RCCL communicators and the library's pooled internal streams (optional; before unloading the
 * library or resetting devices: destroy every handle first -- handles created afterwards get fresh streams). */
int bbb_multi_release(void);

/* ---- pulse shaper and transmitter output (8 samples per data bit) -------------------------- */

/* PRBSShaper (gateware/bbb/bitshaper.py:12-86) and TX (gateware/bbb/tx.py:33-81).
 * Sample n of the shaper is  sum_{idx<8} (bit[M-idx] ? +1 : -1) * coeffs[8*idx + ph]  (12-bit
 * signed), M = floor((n-17)/8), ph = (n-17) mod 8: the 64-tap pulse applied to +-1 impulses at the
 * middle of each 8-sample bit period with the 13-sample pipeline delay the reference's own test
 * compensates (bitshaper.py:143-155); data bits before the first one count as 0 (reset shift
 * register).  From sample 73 on this equals scipy.signal.lfilter(coeffs, [1], impulses)[n-13].
 * TX.x = wrap12(bit_en * shaped + noise_en * wrap12(g * noise_var)), g = CLT sample of LUTOPT
 * state A^(warmup + n + 1) init (tx.py:70-81); the relative alignment of noise and bits is
 * build-defined. */
typedef struct {
    int16_t  coeffs[64];   /* one coefficient set, each in (-256, 255] (bitshaper.py:19-21) */
    int32_t  source;       /* 0 = PRBS (tx.py src_sel 0), 1 = Pulser: one 1 every 256 bits (tx.py:20-30) */
    int32_t  prbs_k;
    uint64_t prbs_state;
    int32_t  bit_en, noise_en, noise_var, reserved;   /* tx.py:39-52 */
    uint64_t warmup;       /* LUTOPT clocks before the first noise sample */
} bbb_tx_cfg;

/* PRBSShaper.x: samples first_sample .. first_sample+nsamples-1 as int16 (only cfg->coeffs,
 * source, prbs_k, prbs_state are used).  out_dev must be 16-byte aligned. */
int bbb_shaper_fill_i16(const bbb_tx_cfg *cfg, int16_t *out_dev, uint64_t nsamples, uint64_t first_sample,
                        int device, void *hip_stream);
/* TX.x on the handle's generator and stream. */
int bbb_tx_fill_i16(bbb_lutopt *h, const bbb_tx_cfg *cfg, int16_t *out_dev, uint64_t nsamples,
                    uint64_t first_sample);
/* TX.x as a sequential stream (tx.py:39-81: one sample per clock), the counterpart of bbb_awgn_stream_* for the waveform:
 * open keeps a copy of *cfg, turns the two-kernel form on for the handle (level 2 of bbb_lutopt_set_staged: one noise
 * kernel per two calls, a shaping mover per call -- unless the caller had chosen a level) and announces the first call;
 * next delivers nsamples_per_call samples at the stream position and announces the call after it; read is next with
 * another length (a ragged tail); seek moves the position (what waits ahead is dropped); close restores the handle's
 * staging level.  Every call is bbb_tx_fill_i16 on the handle's stream: same samples, same errors.  One open stream per
 * handle (noise or transmitter). */
typedef struct bbb_tx_stream bbb_tx_stream;
int bbb_tx_stream_open(bbb_lutopt *h, const bbb_tx_cfg *cfg, uint64_t nsamples_per_call, uint64_t first_sample, bbb_tx_stream **s);
int bbb_tx_stream_next(bbb_tx_stream *s, int16_t *out_dev);
int bbb_tx_stream_read(bbb_tx_stream *s, int16_t *out_dev, uint64_t nsamples);
int bbb_tx_stream_seek(bbb_tx_stream *s, uint64_t first_sample);
int bbb_tx_stream_tell(const bbb_tx_stream *s, uint64_t *next_sample);
int bbb_tx_stream_close(bbb_tx_stream *s);

/* Receiver front end: sign slicer (gateware/bbb/rx.py:29: bit = sample >= 0), sampling phase
 * (the BitDelayLine of rx.py:32-33, delayline.py:45-66) and clock division (rx.py:35-43); with
 * strict != 0 the threshold of software/memdump/decode.py:15-16 (sample > 0, there with stride 4).
 * Bit j = decide(samples_dev[phase + j*stride]) for every j with phase + j*stride < nsamples,
 * packed LSB first into u64 words (the layout bbb_prbs_check reads); *nbits_out (host, may be
 * NULL) receives the number of bits.  bits_packed_dev needs ceil(nbits/64) words. */
int bbb_rx_slice(const int16_t *samples_dev, uint64_t nsamples, uint64_t stride, uint64_t phase, int strict,
                 uint64_t *bits_packed_dev, uint64_t *nbits_out, int device, void *hip_stream);

/* The reference's sampling-phase knob (`sample_delay`, rx.py:19,32-33: 0..samples_per_bit) tried at
 * every setting: for phase p in [0, nphases) slice bit j = decide(samples_dev[p + j*stride]) and run
 * the exact detector over the resulting stream; stats_out[p] (host) receives the totals.  The best
 * phase is the one with the fewest `errors`; nothing here chooses for the caller. */
int bbb_rx_phase_search(const int16_t *samples_dev, uint64_t nsamples, uint64_t stride, uint64_t nphases, int strict,
                        int k, bbb_detector_stats *stats_out, int device, void *hip_stream);

/* ---- eye diagram and bathtub (gateware/bbb/dso.py, drawn by ui.py; software/memdump/eye.py) ---- */

/* The DSO (dso.py:12-72) keeps 256 rows x 64 columns; a sample's row is 127 - sample (8-bit signed), its column is its
 * position after a line trigger.  Here every sample is COUNTED:
 *   row(x) = 127 - clamp(x >> shift, -128, 127)   (arithmetic shift; saturating where dso.py:68 truncates to 8 bits)
 *   col(n) = (n - col_origin) mod ncols            (n = absolute sample number)
 *   hist[row * ncols + col] += 1                   (uint64; for ncols = 64 the DSO address row << 6 | col, so hist > 0
 *                                                   is the DSO's persistence image)
 * Bathtub (transmitter side only).  The shaper formula above makes data bit m contribute coeffs[n - 17 - 8m] to sample n;
 * tap 32 is the pulse centre (t = 0 of np.arange(-32, 32), bitshaper.py:99,123), so bit m peaks at n = 8m + 49.  Phase p
 * (0..7) decides bit m from sample n = 8m + BBB_TX_BIT_SAMPLE0 + p (phase 4 is the pulse centre) with
 *   decision = strict ? x > threshold : x >= threshold      (rx.py:29 at threshold 0; software/memdump/decode.py:15)
 * bathtub[2p] += bits decided at phase p, bathtub[2p+1] += those whose decision differs from data bit m of the
 * transmitter's source (PRBS-k from prbs_state, or the Pulser).  Only bits m >= 0 whose sample lies in the range count.
 * Both outputs are ADDED TO (never overwritten), like bbb_ber_trials_dev: the totals do not depend on how a range is cut
 * into calls, and a multi-GPU host reduces them with one collective. */
#define BBB_TX_BIT_SAMPLE0 45
typedef struct {
    uint32_t ncols;       /* 8, 16, 32 or 64 columns (dso.py: 64) */
    uint32_t shift;       /* 0..15: row = 127 - clamp(x >> shift, -128, 127) */
    uint64_t col_origin;  /* sample n lands in column (n - col_origin) mod ncols */
    int32_t  threshold;   /* bathtub decision: x >= threshold ... */
    int32_t  strict;      /* ... or, with strict != 0, x > threshold */
} bbb_eye_cfg;

/* Capture side: the eye of any int16 samples already on the device (ADC captures, bbb_tx_fill_i16 output); samples_dev[i]
 * is sample number first_sample + i.  hist_dev: [256][ncols] uint64, added to.  Any alignment of samples_dev (2 bytes).
 * Asynchronous on hip_stream. */
int bbb_eye_accumulate_i16(const int16_t *samples_dev, uint64_t nsamples, uint64_t first_sample, const bbb_eye_cfg *eye,
                           uint64_t *hist_dev, int device, void *hip_stream);
/* Transmitter side: eye and bathtub of TX.x (bbb_tx_fill_i16 of *cfg on the handle) over any sample range, the waveform never
 * handed to the caller.  The object keeps copies of *cfg and *eye and owns its scratch: an int16 chunk of chunk_samples
 * (0: 2^26, which fits the Infinity Cache), the chunk's data bits and the per-block partial histograms.  run covers samples
 * [first_sample, first_sample + nsamples) chunk by chunk on the handle's stream (fill, data bits, accumulate), adding into
 * hist_dev ([256][ncols] uint64) and bathtub_dev ([8][2] uint64); either may be NULL, not both.  Asynchronous.
 * LIFETIME: as bbb_ber_run -- close the object BEFORE bbb_lutopt_destroy of its handle. */
typedef struct bbb_tx_eye bbb_tx_eye;
int bbb_tx_eye_open(bbb_lutopt *h, const bbb_tx_cfg *cfg, const bbb_eye_cfg *eye, uint64_t chunk_samples, bbb_tx_eye **out);
int bbb_tx_eye_run(bbb_tx_eye *e, uint64_t first_sample, uint64_t nsamples, uint64_t *hist_dev, uint64_t *bathtub_dev);
int bbb_tx_eye_close(bbb_tx_eye *e);

/* ---- BER of the shaped link over many transmitter settings in one pass --------------------------------------------- */

/* One setting of the transmitter's knobs (tx.py:39-54: the shape set, bit_en, noise_en, noise_var) and of the receiver's
 * decision (as bbb_eye_cfg).  coeffs each in (-256, 255]; noise_var 0..15; reserved must be 0. */
typedef struct {
    int16_t coeffs[64];          /* one coefficient set, as bbb_tx_cfg */
    int32_t bit_en, noise_en, noise_var;
    int32_t threshold, strict;   /* decision, as bbb_eye_cfg */
    int32_t reserved;            /* must be 0 */
} bbb_tx_setting;
/* The bathtub of bbb_tx_eye_run for nset settings at once.  counters_dev is [nset][8][2] uint64 and is ADDED TO: entry
 * [i][p] receives exactly what bathtub_dev[p] of bbb_tx_eye_run receives for the bbb_tx_cfg equal to *base with coeffs,
 * bit_en, noise_en and noise_var taken from settings[i], and an eye cfg with settings[i]'s threshold / strict, over the same
 * range.  *base supplies source, prbs_k, prbs_state and warmup; its other fields are ignored.  nset is 1..512 (the 32 x 16
 * shape x noise_var grid of the board fits one object).  The noise sample and the data bits of a sample are the same for
 * every setting, so run generates them once per chunk (chunk_samples, 0: 2^26 int8 samples, which stay in the Infinity
 * Cache) and every group of settings re-reads them from there: the noise stream is generated once, whatever nset is.
 * Handles that bbb_tx_fill_i16 refuses with noise on get the same BBB_EUNSUP from run when a setting has noise_en.
 * Asynchronous on the handle's stream.  LIFETIME: as bbb_tx_eye -- close the object BEFORE bbb_lutopt_destroy of its handle. */
typedef struct bbb_tx_ber_sweep bbb_tx_ber_sweep;
int bbb_tx_ber_sweep_open(bbb_lutopt *h, const bbb_tx_cfg *base, const bbb_tx_setting *settings, int nset,
                          uint64_t chunk_samples, bbb_tx_ber_sweep **out);
int bbb_tx_ber_sweep_run(bbb_tx_ber_sweep *s, uint64_t first_sample, uint64_t nsamples, uint64_t *counters_dev);
int bbb_tx_ber_sweep_close(bbb_tx_ber_sweep *s);

/* ---- autocorrelation counters: the waveform in frequency (software/memdump/fftplot.py) ------------------------------ */

/* Exact integer counters from which a host computes the power spectrum (a Blackman-Tukey estimate: with a Bartlett lag
 * window it is the expected averaged periodogram of nlags-sample segments, what a spectrum analyser shows with averaging).
 * Capture side: for l in [0, nlags)
 *   acf_dev[l]     += sum_{i < nfirst} x[i] * x[i + l]     with x[j] = samples_dev[j] for j < navail, 0 beyond
 *   acf_dev[nlags] += sum_{i < nfirst} x[i]
 * int64, added to modulo 2^64.  Exact while the true sums fit int64: more than 2^41 first elements for |x| <= 2048,
 * more than 2^32 for full-range int16.  navail >= nfirst.  navail = nfirst is the biased estimate of one whole capture;
 * navail = nfirst + nlags - 1 lets consecutive slices of one long record add up to the record's counters exactly.
 * nlags 1..BBB_ACF_MAX_LAGS; nfirst = 0 is a no-op.  Any 2-byte alignment.  Asynchronous on hip_stream.
 * MEMORY: a call's scratch (8 bytes per 4096 first elements for every started 320 lags, plus a few MiB of partials) comes
 * from a memory pool the library creates per device and never releases: what the largest call took stays reserved for the
 * rest of the process, outside any other allocator's view, and is reused by later calls. */
#define BBB_ACF_MAX_LAGS 4096
int bbb_acf_accumulate_i16(const int16_t *samples_dev, uint64_t nfirst, uint64_t navail, uint32_t nlags,
                           int64_t *acf_dev, int device, void *hip_stream);
/* Transmitter side: the same counters over TX.x (bbb_tx_fill_i16 of *cfg on the handle), first elements
 * [first_sample, first_sample + nsamples).  The partners always exist, because the waveform continues.  The object keeps a
 * copy of *cfg and owns an int16 chunk of chunk_samples + nlags - 1 samples (chunk_samples 0: 2^26) and the partials;
 * run fills and correlates chunk by chunk on the handle's stream.  nsamples = 0 is a no-op.  Asynchronous.
 * LIFETIME: as bbb_tx_eye -- close the object BEFORE bbb_lutopt_destroy of its handle. */
typedef struct bbb_tx_acf bbb_tx_acf;
int bbb_tx_acf_open(bbb_lutopt *h, const bbb_tx_cfg *cfg, uint32_t nlags, uint64_t chunk_samples, bbb_tx_acf **out);
int bbb_tx_acf_run(bbb_tx_acf *a, uint64_t first_sample, uint64_t nsamples, int64_t *acf_dev);
int bbb_tx_acf_close(bbb_tx_acf *a);

/* ---- pulse response: the correlation of a waveform with its own data bits ------------------------------------------ */

/* What a link tester measures first: the received samples correlated with the known data bits.  With spb samples per data
 * bit, bit m >= 0 of sign s[m] = bit ? +1 : -1, absolute sample numbers n and `origin` the sample at which bit 0 has lag 0:
 * for every sample n in [first_sample, first_sample + nsamples) and every lag l in [0, nlags) with (n - origin - l)
 * divisible by spb and m = (n - origin - l) / spb >= 0
 *   xc_dev[l] += s[m] * x[n]           int64, added to modulo 2^64 (never overwritten)
 * The rule is keyed on samples, so the totals do not depend on how a range is cut into calls (the convention of the bathtub
 * and of the ACF); terms with m < 0 do not count.  Exact for full-range int16, -32768 included, while the true sums fit
 * int64.  xc[l] divided by the number of terms of lag l estimates the link's pulse response h[l]: for the transmitter
 * origin = BBB_TX_BIT_ORIGIN and spb = 8, where bit m contributes coeffs[n - 17 - 8m] to sample n (see the eye section), so
 * lag l lines up with coeffs[l].
 * spb is 1, 2, 4, 8, 16 or 32; nlags 1 .. min(64 * spb, BBB_XCORR_MAX_LAGS): a sample never looks back over more than 64
 * bits; origin <= 2^62.  samples_dev[i] is sample first_sample + i (any 2-byte alignment).  bits_packed_dev holds data bits
 * bit0 .. bit0 + nbits - 1 LSB first in u64 words, 8-byte aligned, as bbb_prbs_fill writes them (bit0 + nbits <= 2^62).  The
 * call needs bits max(0, floor((first_sample - origin - (nlags - 1)) / spb)) .. floor((first_sample + nsamples - 1 - origin)
 * / spb); a bit range that does not cover them is BBB_EINVAL, decided from the numbers alone.  A call whose samples all lie
 * below bit 0 needs no bits and adds nothing.  nsamples = 0 is a no-op.  Every argument check comes before the device is
 * touched.  Asynchronous on hip_stream; the call's scratch is a stream-ordered allocation, as bbb_eye_accumulate_i16's. */
#define BBB_XCORR_MAX_LAGS 1024
#define BBB_TX_BIT_ORIGIN 17
typedef struct { uint32_t spb; uint32_t nlags; uint64_t origin; } bbb_xcorr_cfg;
int bbb_xcorr_accumulate_i16(const int16_t *samples_dev, uint64_t nsamples, uint64_t first_sample,
                             const uint64_t *bits_packed_dev, uint64_t bit0, uint64_t nbits,
                             const bbb_xcorr_cfg *cfg, int64_t *xc_dev, int device, void *hip_stream);
/* Transmitter side: the counters of bbb_xcorr_accumulate_i16 over TX.x (bbb_tx_fill_i16 of *cfg on the handle) with spb 8 and
 * origin BBB_TX_BIT_ORIGIN, against the bits of the transmitter's source (PRBS-k from prbs_state, or the Pulser), samples
 * [first_sample, first_sample + nsamples).  nlags 1..512.  The object keeps a copy of *cfg and owns an int16 chunk of
 * chunk_samples (0: 2^26), the chunk's data bits and the partials; run fills, generates the bits and correlates chunk by
 * chunk on the handle's stream, adding into xc_dev ([nlags] int64).  nsamples = 0 is a no-op.  Asynchronous.
 * LIFETIME: as bbb_tx_acf -- close the object BEFORE bbb_lutopt_destroy of its handle. */
typedef struct bbb_tx_xcorr bbb_tx_xcorr;
int bbb_tx_xcorr_open(bbb_lutopt *h, const bbb_tx_cfg *cfg, uint32_t nlags, uint64_t chunk_samples, bbb_tx_xcorr **out);
int bbb_tx_xcorr_run(bbb_tx_xcorr *x, uint64_t first_sample, uint64_t nsamples, int64_t *xc_dev);
int bbb_tx_xcorr_close(bbb_tx_xcorr *x);

/* ---- numerically controlled oscillator: the board's tone source (gateware/bbb/nco.py) ------------------------------ */

/* NCO(fcw, am, fm, pm) with n = 24, m = 10, p = 16 (nco.py:25-44), clocked once per output sample t:
 *   adr(t) = ((pa >> 14) + pm(t)) mod 1024          pa' = (pa + fcw + fm(t)) mod 2^24
 *   q' = rom[adr(t)]   w' = q   y' = am(t) * w       x(t) = y >> 16   (arithmetic: y[16:32], nco.py:43)
 * rom[i] = round_half_even(32767 * sin(2 pi i / 1023)), i = 0 .. 1023 (np.linspace(0, 2 pi, 1024), nco.py:30-31: the
 * table's period is 1023 steps, rom[0] = rom[1023] = 0).  q is the ROM port's registered output (migen's synchronous read
 * port), so x(t) = (am(t - 1) * rom[adr(t - 3)]) >> 16 from reset, where the first three outputs are 0 (the latency
 * test_nco pins, nco.py:47-66).  When each input enters (fm before pa, pm at the address, am at the product) is read from
 * the module's text; the reference's test pins only constant inputs.
 * Each input is a constant of the object's cfg or, per call, a device buffer of one value per sample.  Buffer values are
 * taken modulo their widths: the low 24 bits of fm (two's complement), the low 10 bits of pm; am is uint16 as it is.
 * cfg ranges (else BBB_EINVAL): fcw < 2^24, am < 2^16, fm in [-2^23, 2^23), pm in [-512, 512). */
typedef struct { uint32_t fcw; uint32_t am; int32_t fm; int32_t pm; } bbb_nco_cfg;
/* The module's registers; all 0 = reset.  pa < 2^24, q and w in int16, y any int32. */
typedef struct { uint32_t pa; int32_t q, w, y; } bbb_nco_state;
typedef struct bbb_nco bbb_nco;
/* The ROM (host only, works without a GPU). */
int bbb_nco_rom(int16_t rom[1024]);
/* An oscillator in the reset state on `device`, its work ordered on hip_stream.  The object keeps its state on the device,
 * so that consecutive runs never wait on the host.  A device without gfx950 gives BBB_ENODEV. */
int bbb_nco_open(const bbb_nco_cfg *cfg, int device, void *hip_stream, bbb_nco **out);
/* Retune between runs (the state is kept); ordered behind the runs already queued. */
int bbb_nco_set_cfg(bbb_nco *o, const bbb_nco_cfg *cfg);
/* Move the object's later work to another stream, behind everything it queued on the old one (as bbb_lutopt_set_stream). */
int bbb_nco_set_stream(bbb_nco *o, void *hip_stream);
/* nsamples clocks from the object's state: x_dev[t] = x(t); fm_dev / am_dev / pm_dev give the input of clock t where not
 * NULL, the cfg's constant where NULL.  Any alignment of the element types; 16-byte aligned buffers take the wide path.
 * Consecutive runs continue one waveform.  nsamples = 0 is a no-op.  Asynchronous on the object's stream. */
int bbb_nco_run(bbb_nco *o, const int32_t *fm_dev, const uint16_t *am_dev, const int16_t *pm_dev, uint64_t nsamples,
                int16_t *x_dev);
/* The registers after every run queued so far (waits for the object's stream) / replace them (ordered on the stream). */
int bbb_nco_get_state(bbb_nco *o, bbb_nco_state *st);
int bbb_nco_set_state(bbb_nco *o, const bbb_nco_state *st);
int bbb_nco_close(bbb_nco *o);

/* ---- 16x sinc interpolator: the scope's SincInterpolator (gateware/bbb/sinc.py) -------------------------------------- */

/* 16 output samples per input sample through an 8-tap polyphase windowed sinc (sinc.py:12-49, 91-98):
 *   h[k] = trunc_toward_zero(127 * sinc(t_k) * hamming_k), t = linspace(-4, 4, 128), symmetric 128-point Hamming window, int8
 *   acc(m, c)   = sum_{i=0..7} h[16 i + c] * x[m - i]       m >= 0 the input sample, c = 0..15 the phase;
 *                                                           x[j] = 0 before the start of the record
 *   y[16 m + c] = int8(acc(m, c) >> 8)                      arithmetic shift
 * The module's 16-bit adders never wrap (max_c sum_i |h[16 i + c]| = 203, so |acc| <= 25 984) and y lies in -102 .. 101.
 * The DC gain per phase is 125/256 or 126/256: the reference halves the amplitude, and so does this.
 * The module itself (72 inputs with no history in, 1024 samples out, as test_sinc pins it) is y[109 .. 1132]. */
#define BBB_SINC_UP   16      /* output samples per input sample */
#define BBB_SINC_TAPS 8       /* input samples per output sample */
/* The table h (host only, works without a GPU).  Tap i of phase c is h[16 i + c]; the reference's BRAM word 2c is
 * h[c] << 24 | h[16 + c] << 16 | h[32 + c] << 8 | h[48 + c] (bytes), word 2c + 1 the same of h[64 + c ..]. */
int bbb_sinc_coefficients(int8_t h[128]);

typedef struct {
    uint32_t in_bytes;    /* 1: int8 samples (sinc.py's port).  2: int16 samples, x8 = clamp(x >> shift, -128, 127), the
                             row rule of bbb_eye_cfg */
    uint32_t out_bytes;   /* 1: int8 (the reference's port).  2: the same values as int16, for bbb_eye_accumulate_i16,
                             bbb_acf_accumulate_i16, bbb_rx_slice, bbb_rx_phase_search */
    uint32_t shift;       /* 0..15 with in_bytes = 2; must be 0 with in_bytes = 1 */
} bbb_sinc_cfg;

/* out_dev[16 m + c] = y[16 m + c] for m in [0, nin): 16 nin elements of out_bytes each.  in_dev[-1] .. in_dev[-nbefore]
 * (elements) must be readable and are the record's earlier samples (only the nearest 7 are used); history beyond them is
 * 0, so a call that is given the 7 samples in front of its first input continues the stream exactly.  Any element
 * alignment of both pointers; an out_dev aligned to 16 bytes takes the wide stores.  nin = 0 is a no-op.  Asynchronous
 * on hip_stream. */
int bbb_sinc_interpolate(const void *in_dev, uint64_t nin, uint32_t nbefore, const bbb_sinc_cfg *cfg, void *out_dev,
                         int device, void *hip_stream);

/* The eye of the interpolated record without handing it to the caller: exactly what bbb_eye_accumulate_i16(eye) counts
 * over the int16 interpolated stream whose sample number is 16 * (first_sample + m) + c.  run works chunk by chunk
 * through a buffer the object owns (chunk_in input samples, at most 2^27; 0: 2^24, 512 MiB of int16) on hip_stream;
 * hist_dev ([256][ncols] uint64) is added to.  cfg->out_bytes is ignored.  first_sample + nin <= 2^58. */
typedef struct bbb_sinc_eye bbb_sinc_eye;
int bbb_sinc_eye_open(const bbb_sinc_cfg *cfg, const bbb_eye_cfg *eye, uint64_t chunk_in, int device, void *hip_stream,
                      bbb_sinc_eye **out);
int bbb_sinc_eye_run(bbb_sinc_eye *e, const void *in_dev, uint64_t nin, uint32_t nbefore, uint64_t first_sample,
                     uint64_t *hist_dev);
int bbb_sinc_eye_close(bbb_sinc_eye *e);

/* ---- exact integer FIR filter: receive filter, decimator, filtered slicer (gateware/bbb/average.py, rx.py:24-26) ---- */

/*   acc(n) = sum_{i < ntaps} h[i] * x[n - i]       x[j], j < 0: in_dev[j] while j >= -nbefore, 0 beyond
 *   y[q]   = sat(acc(phase + q * decim) >> shift)   q in [0, nout), arithmetic shift
 *   nout   = phase < nin ? (nin - phase + decim - 1) / decim : 0
 * With sum |h[i]| <= 65535 and int16 samples |acc| <= 65535 * 32768 < 2^31: exact int32 arithmetic is the definition and
 * the int32 output never saturates.  The reference's MovingAverage (average.py:26-33), stepped clock by clock, is
 * x(t) = s(t-3) + s(t-4) + s(t-5) + s(t-6): taps {0, 0, 0, 1, 1, 1, 1} at shift 0 (its own test expects that timing with
 * shift 2); software/memdump/adcplot.py:34-36 is taps {1, 1, 1, 1}, decim 4, phase 3. */
#define BBB_FIR_MAX_TAPS 256
typedef struct {
    uint32_t ntaps;       /* 1..256 */
    int16_t  taps[256];   /* h[0..ntaps-1]; sum |h[i]| <= 65535, else BBB_EINVAL */
    uint32_t shift;       /* 0..31, arithmetic */
    uint32_t decim;       /* 1..256: one output per decim inputs */
    uint32_t phase;       /* < decim: output q sits at input index phase + q * decim */
    uint32_t out_bytes;   /* 2: int16, saturating.  4: int32 */
} bbb_fir_cfg;

/* The moving average as a preset (host only, works without a GPU): taps {1, 1, 1, 1}, or with `pipeline` the module's
 * registers {0, 0, 0, 1, 1, 1, 1}; shift 0, decim 1, phase 0, out_bytes 2. */
int bbb_fir_moving_average(bbb_fir_cfg *cfg, int pipeline);

/* out_dev[q] = y[q] for q in [0, nout); *nout_out (host, may be NULL) receives nout.  The history convention is
 * bbb_sinc_interpolate's: in_dev[-1] .. in_dev[-nbefore] must be readable and are the record's earlier samples (only the
 * nearest ntaps - 1 are used), history beyond them is 0, so a call that is given them continues a stream exactly.  in_dev
 * may have any 2-byte alignment (an in_dev aligned to 16 bytes takes the wide loads), out_dev any element alignment (an
 * out_dev aligned to 16 bytes takes the wide stores).  nin = 0 is a no-op.  An out_dev that overlaps the samples read is
 * BBB_EINVAL, as is everything wrong with cfg, which is checked before the device is touched.  Asynchronous on hip_stream. */
int bbb_fir_filter(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, const bbb_fir_cfg *cfg, void *out_dev,
                   uint64_t *nout_out, int device, void *hip_stream);

/* The receiver of rx.py:24-26 (MovingAverage, then `avg.x > 0`) without the filtered samples ever reaching memory:
 * bit q = acc(phase + q * decim) >= threshold (> threshold with strict != 0), threshold in units of acc; packed LSB first
 * into u64 words, the layout bbb_rx_slice writes, the unused bits of the last word 0.  cfg->shift and cfg->out_bytes are
 * ignored.  bits_packed_dev needs ceil(nbits / 64) words; *nbits_out (host, may be NULL) receives nbits = nout. */
int bbb_fir_slice(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, const bbb_fir_cfg *cfg, int32_t threshold,
                  int strict, uint64_t *bits_packed_dev, uint64_t *nbits_out, int device, void *hip_stream);

/* ---- digital down-converter: quadrature mixer, FIR, I/Q or polar outputs (the receive half of gateware/bbb/nco.py) ---- */

/* An int16 capture at a carrier taken to baseband.  All integers, >> arithmetic, rom = bbb_nco_rom:
 *   j(n)   = (first_sample + n) mod 2^24               n < 0 (history) in two's complement
 *   pa(n)  = (pa0 + j(n) * fcw) mod 2^24               adr(n) = pa(n) >> 14
 *   c(n)   = rom[(adr(n) + 256) mod 1024]              s(n) = rom[adr(n)]
 *   mi(n)  = (x(n) * c(n)) >> 15                       mq(n) = (x(n) * -s(n)) >> 15          both in [-32767, 32767]
 *   x(n), n < 0: in_dev[n] while n >= -nbefore, 0 beyond (bbb_fir_filter's history rule)
 *   ai(n)  = sum_{i < ntaps} h[i] * mi(n - i)          aq(n) likewise: exact int32 under the rules of bbb_fir_cfg
 *   I[q]   = sat16(ai(phase + q * decim) >> shift)     Q[q] likewise; nout as in bbb_fir_cfg
 * The oscillator has no state: it is a function of the absolute sample number, so a capture cut anywhere and continued with
 * nbefore / first_sample gives the outputs of one call.  pa0 = (-3 * fcw) mod 2^24 lines it up with a bbb_nco of the same fcw
 * run from reset (whose output lags its phase accumulator by 3 samples).
 * mode BBB_DDC_IQ16: out_dev[q] = (I, Q) as two int16 (4-byte aligned).  BBB_DDC_IQ32: (ai >> shift, aq >> shift) as two
 * int32, unsaturated (8-byte aligned).  BBB_DDC_POLAR: (mag: uint16, phase: int16 in 1/65536 turn) of the IQ16 pair
 * (4-byte aligned), by this CORDIC: (0, 0) gives (0, 0); otherwise, with neg = I < 0,
 *   X = (neg ? -I : I) << 14   Y = (neg ? -Q : Q) << 14   Z = neg ? 2^31 : 0 (mod 2^32)
 *   k = 0..15: d = Y >= 0; (X, Y) = d ? (X + (Y >> k), Y - (X >> k)) : (X - (Y >> k), Y + (X >> k)); Z += d ? A[k] : -A[k]
 *   A[k] = round(atan(2^-k) / (2 pi) * 2^32)
 *   mag = (int64(X) * 39797 + 2^29) >> 30            phase = int16(((Z + 2^15) >> 16) mod 2^16)
 * in int32 (|X|, |Y| < 2^31 for every pair); mag <= 46341 is within 0.59 of hypot, phase within 1 unit of atan2. */
#define BBB_DDC_IQ16  0
#define BBB_DDC_IQ32  1
#define BBB_DDC_POLAR 2
typedef struct { uint32_t fcw; uint32_t pa0; uint32_t mode; /* BBB_DDC_IQ16 | IQ32 | POLAR */ } bbb_ddc_cfg;
/* out_dev[q] for q in [0, nout); *nout_out (host, may be NULL) receives nout.  in_dev as in bbb_fir_filter (any 2-byte
 * alignment; 16-byte aligned takes the wide loads), out_dev aligned to its element (16 bytes: the wide stores of decim 1).
 * BBB_EINVAL before the device is touched: nulls, fcw or pa0 >= 2^24, a mode that is none of the three, every rule of
 * bbb_fir_cfg but out_bytes (ignored), first_sample + nin > 2^58, an out_dev that overlaps the samples read.  nin = 0 is a
 * no-op.  Asynchronous on hip_stream; a device without gfx950 gives BBB_ENODEV. */
int bbb_ddc_run(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, uint64_t first_sample,
                const bbb_ddc_cfg *ddc, const bbb_fir_cfg *fir /* out_bytes ignored */,
                void *out_dev, uint64_t *nout_out, int device, void *hip_stream);
/* The CORDIC of BBB_DDC_POLAR for one pair (host only, works without a GPU). */
int bbb_ddc_polar_host(int16_t i, int16_t q, uint16_t *mag, int16_t *phase);

/* ---- decision-feedback equalizer: feed-forward FIR, up to 4 feedback taps, exact whatever the data are ------------------- */

/* The receiver's step behind the linear equalizer: the post-cursor interference of the bits already decided is subtracted
 * before the next decision.  With ff a bbb_fir_cfg under its own rules (decim = samples per bit, phase = sampling phase,
 * acc(n) exact in int32, history by nbefore) and nsym = nout of ff, for symbol k in [0, nsym):
 *   a[k]   = acc(phase + k * decim)
 *   v[k]   = a[k] - sum_{i = 1..nfb} fb[i - 1] * d[k - i]        d[j] = +1 if bit[j] else -1
 *   bit[k] = v[k] >= threshold      (> threshold with strict != 0)
 * nfb is 0..BBB_DFE_MAX_FB, fb[] in units of acc; 32768 * sum |ff.taps| + sum |fb| <= 2^31 - 1 keeps v exact in int32 in any
 * order (BBB_EINVAL otherwise).  The decisions in front of symbol 0 are the state word: bit i is the decision of symbol
 * k - 1 - i; bits from nfb on are ignored on input and written as 0; a zeroed word is the shift register out of reset
 * (earlier bits count as 0, the shaper's convention).  nfb = 0 is bbb_fir_slice bit for bit.
 * region_symbols / warmup_symbols (0: the defaults of bbb_dfe_geometry) only place the boundaries of the work on the device:
 * no output depends on them. */
#define BBB_DFE_MAX_FB 4
typedef struct {
    bbb_fir_cfg ff;          /* shift and out_bytes count only where soft values are asked for */
    uint32_t nfb;            /* 0..4 */
    int32_t  fb[4];          /* fb[i] weighs the decision i + 1 symbols back */
    int32_t  threshold;
    uint32_t strict;
    uint32_t region_symbols; /* symbols one workgroup owns; 0: the default */
    uint32_t warmup_symbols; /* symbols run in front of a region to find its start state; 0: the default */
} bbb_dfe_cfg;

/* bits_packed_dev: bit[k] LSB first in u64 words, the layout of bbb_fir_slice, the unused bits of the last word 0
 * (ceil(nsym / 64) words, 8-byte aligned).  soft_dev (may be NULL): nsym values, sat16(v[k] >> ff.shift) as int16 with
 * ff.out_bytes 2, v[k] itself as int32 with ff.out_bytes 4 -- the equalized eye that bbb_eye_accumulate_i16 and the
 * histogram read.  state_dev: ONE uint32 on the device, read at the start and written at the end, so a record handed over in
 * pieces (each with its nbefore samples and this word) never synchronises and gives the bits, soft values and final state
 * of one call.  stats_dev (may be NULL): uint64[4] on the device, ADDED TO: regions, regions whose start state was not proven
 * by their warm-up, regions walked a second time, symbols.  *nbits_out (host, may be NULL) receives nsym.  in_dev as in
 * bbb_fir_filter.  BBB_EINVAL before the device is touched: everything wrong with cfg, nulls, misaligned pointers, outputs
 * that overlap the samples read or each other, more than 2^26 regions.  nin = 0 only rewrites the state word (masked to nfb
 * bits).  The call's scratch (24 bytes per region) comes from the device's memory pool on hip_stream.  Asynchronous. */
int bbb_dfe_run(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, const bbb_dfe_cfg *cfg, uint32_t *state_dev,
                uint64_t *bits_packed_dev, void *soft_dev, uint64_t *stats_dev, uint64_t *nbits_out, int device,
                void *hip_stream);
/* Where the device cuts the work (host only, works without a GPU; every pointer may be NULL): a workgroup stages
 * *step_samples inputs at a time, which hold at most *step_symbols symbols at this decim (symbol k lies in step
 * (phase + k * decim) / *step_samples); a wave scans the *wave_symbols symbols k with equal k / *wave_symbols (64; 512 at decim 1,
 * where a lane owns eight consecutive symbols); the defaults of region_symbols and warmup_symbols. */
int bbb_dfe_geometry(uint32_t decim, uint64_t *step_samples, uint64_t *step_symbols, uint64_t *wave_symbols,
                     uint64_t *region_symbols, uint64_t *warmup_symbols);
/* The definition as a plain serial loop over host memory (works without a GPU): in[-1] .. in[-nbefore] readable, *state the
 * state word (read and written), bits_packed / soft / *nbits_out as in bbb_dfe_run. */
int bbb_dfe_model_host(const int16_t *in, uint64_t nin, uint32_t nbefore, const bbb_dfe_cfg *cfg, uint32_t *state,
                       uint64_t *bits_packed, void *soft, uint64_t *nbits_out);

/* ---- Viterbi sequence detector (MLSE): feed-forward FIR, a target of up to 4 symbols of memory, exact -------------------- */

/* The receiver's strongest detector: the most likely SEQUENCE of bits behind a channel with inter-symbol interference,
 * where the DFE decides bit by bit and propagates its errors.  All integers.  ff is a bbb_fir_cfg under its own rules
 * (decim = samples per bit, phase = sampling phase, history by nbefore), mem = L is 1..BBB_MLSE_MAX_MEM, g[0..L] the target
 * taps in units of y, NS = 2^L:
 *   y[k]      = sat16(acc(phase + k * decim) >> ff.shift)      what bbb_fir_filter writes as int16; k counted from the call
 *   K         = first_symbol + k                               the absolute symbol number
 *   state h   : L bits, bit i = the decision of symbol K - 1 - i (the DFE's convention)
 *   s(h, b)   = g[0] d(b) + sum_{i = 1..L} g[i] d(bit i - 1 of h)        d(1) = +1, d(0) = -1
 *   gain(h,b) = 2 y s(h, b) - s(h, b)^2                        maximised: -(y - s)^2 with y^2 dropped
 *   h'        = ((h << 1) | b) & (NS - 1)
 * ACS: the predecessors of h' are h = (h' >> 1) | (c << (L - 1)), c = 0, 1; the larger m[h] + gain(h, h' & 1) survives, a tie
 * goes to c = 0.
 * Blocks on ABSOLUTE symbol numbers: block j is the symbols [j B, (j + 1) B); its bits come from ONE Viterbi run over the
 * window [max(0, j B - W), min(Nend, (j + 1) B + D)).  A window that starts at symbol 0 allows init_state (masked to L bits)
 * alone, any other window starts every state at metric 0.  At the window's end the largest metric is the best state, on a
 * tie the lowest index; the path is traced back along the survivors, the decision of symbol K is bit 0 of the path's state
 * behind symbol K, and only the block's own symbols are emitted.  B = block_symbols, W = warmup_symbols and D =
 * lookahead_symbols (0: 192, 32, 32) ARE part of the definition; 1 <= B, W <= 128, D <= 128, B + W + D <= 512.  Nend is the
 * record's end, known only to a call with final != 0: Nend = first_symbol + nsym, and such a call decides all its nsym
 * symbols.  A call with final == 0 decides the symbols below the largest block boundary E with E + D <= first_symbol + nsym:
 * the whole blocks whose unclipped window lies inside it.  first_symbol may sit anywhere inside a block: the block's window
 * is the same absolute one, its symbols in front of the call are read through nbefore (and are 0-filled beyond it, the FIR's
 * rule).  So a capture cut at block boundaries E, each piece with its history, gives the bits of one call; the detector has
 * no state on the device.
 * sum |g[i]| <= 2^20: with |y| <= 32768 and at most 512 symbols every path metric stays below 2^50, int64 is exact. */
#define BBB_MLSE_MAX_MEM 4
typedef struct {
    bbb_fir_cfg ff;             /* out_bytes must be valid and is otherwise ignored: y is the int16 form */
    uint32_t mem;               /* 1..4 */
    int32_t  g[5];              /* g[0]: the cursor, g[i]: the symbol i back; entries beyond mem are ignored */
    uint32_t init_state;        /* the decisions in front of symbol 0, bit i = symbol -1 - i */
    uint32_t block_symbols, warmup_symbols, lookahead_symbols;      /* 0: the default */
} bbb_mlse_cfg;

/* The sizes of a call, from sizes alone (host only, works without a GPU; the three outputs may be NULL): *nsym = nout of
 * ff, *ndecided as above, *nbefore_wanted the history in samples with which the call's first window is not zero-filled:
 * (first_symbol - the window's first symbol) * decim + ntaps - 1 less the `phase` samples the call itself holds; at a block
 * boundary that is min(first_symbol, W) * decim + ntaps - 1 - phase.  BBB_EINVAL for everything wrong with cfg and for
 * first_symbol + nsym > 2^58. */
int bbb_mlse_plan(const bbb_mlse_cfg *cfg, uint64_t nin, uint64_t first_symbol, int final, uint64_t *nsym, uint64_t *ndecided,
                  uint64_t *nbefore_wanted);
/* bits_packed_dev: the decision of symbol first_symbol + k is bit k, LSB first in u64 words, the layout of bbb_fir_slice,
 * the unused bits of the last word 0 (ceil(ndecided / 64) words, 8-byte aligned; words beyond them are not touched).
 * stats_dev (may be NULL): uint64[2] on the device, ADDED TO: windows walked, symbols decided.  *ndecided_out (host, may be
 * NULL) receives ndecided, which is bbb_mlse_plan's.  in_dev as in bbb_fir_filter; of nbefore only what the first window
 * reaches (nbefore_wanted) is read.  BBB_EINVAL before the device is touched: everything wrong with cfg (ff's own rules,
 * mem, sum |g|, the geometry), nulls, misaligned pointers, an output that overlaps the samples read, first_symbol + nsym >
 * 2^58.  nin = 0 or ndecided = 0 writes nothing.  Asynchronous on hip_stream; a device without gfx950 gives BBB_ENODEV. */
int bbb_mlse_run(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, uint64_t first_symbol, int final, const bbb_mlse_cfg *cfg,
                 uint64_t *bits_packed_dev, uint64_t *stats_dev, uint64_t *ndecided_out, int device, void *hip_stream);
/* The definition as a plain serial loop over host memory (works without a GPU): in[-1] .. in[-nbefore] readable,
 * bits_packed / *ndecided_out as in bbb_mlse_run. */
int bbb_mlse_model_host(const int16_t *in, uint64_t nin, uint32_t nbefore, uint64_t first_symbol, int final, const bbb_mlse_cfg *cfg,
                        uint64_t *bits_packed, uint64_t *ndecided_out);

/* ---- symbol timing recovery: a block-wise early/late tracker of the sampling phase, exact whatever the data are ---------- */

/* Every decision above is taken at phase + k * decim: one sampling phase for the whole record.  A capture from an ADC with
 * its own clock drifts; this tracker follows it and hands out one decision (and soft value) per symbol.  All integers.
 * ff is a bbb_fir_cfg under its own rules with decim == 1 and phase == 0 (one tap {1}: no filter); a(n) = acc(n) for n in
 * [-1, nin), history by bbb_fir_filter's rule.  P = spb (3..256) samples per bit, L = block_symbols (8..1024, L * P <= 65536;
 * 0: 64), h = hysteresis_shift (1..63; 0: 4), threshold and strict as in bbb_dfe_cfg, init_phase < P or BBB_TIMING_ACQUIRE.
 * Block j is the samples [j L P, (j + 1) L P) inside [0, nin); nblocks = final ? ceil(nin / (L P)) : floor(nin / (L P)), so
 * only the last block of a final call may be partial.  Its metric, for p in [0, P):
 *   E_j[p] = sum over i in [0, L) with t = j L P + i P + p < nin of |a(t) - threshold|              int64, below 2^43
 * The state is (locked, phi); a zeroed state is out of reset.
 *   first block after reset: phi_j = init_phase if that is below P, else the p with the largest E_j[p] (the lowest on a
 *                            tie); m_j = 0
 *   every other block:       phi = phi_(j-1), cur = E_j[phi], up = E_j[(phi + 1) mod P], dn = E_j[(phi + P - 1) mod P],
 *                            margin = cur >> h; m_j = +1 if up > cur + margin and up >= dn, else -1 if dn > cur + margin,
 *                            else 0; phi_j = (phi + m_j) mod P
 *   wrap:                    w_j = +1 if m_j = +1 and phi_j = 0; -1 if m_j = -1 and phi_j = P - 1; else 0
 * Block j emits the instants t = j L P + phi_j + i P for i = w_j .. L - 1 with t < nin: L - 1 bits after a wrap up, L + 1 after
 * a wrap down (the first of them one sample in front of the block; for block 0 that is a(-1), read through the history),
 * L otherwise.  No bit is sampled twice or skipped; consecutive instants are P - 1, P or P + 1 samples apart.
 * bit = a(t) >= threshold (> with strict); soft value sat16(a(t) >> ff.shift) with out_bytes 2, a(t) with out_bytes 4; both
 * go out in order of t from bit 0 / element 0 of the call's outputs.
 * chunk_blocks (0: the default) only places the boundaries of the device's work: no output depends on it. */
#define BBB_TIMING_ACQUIRE 0xFFFFFFFFu
typedef struct {
    bbb_fir_cfg ff;            /* decim 1, phase 0; shift and out_bytes count only where soft values are asked for */
    uint32_t spb;              /* P: 3..256 */
    uint32_t block_symbols;    /* L: 8..1024, L * P <= 65536; 0: 64 */
    uint32_t hysteresis_shift; /* h: 1..63; 0: 4 */
    int32_t  threshold;
    uint32_t strict;
    uint32_t init_phase;       /* < P, or BBB_TIMING_ACQUIRE */
    uint32_t chunk_blocks;     /* blocks one workgroup walks; 0: the default */
} bbb_timing_cfg;

/* The sizes of a call, from sizes alone (host only, works without a GPU; every output may be NULL): *nblocks as above,
 * *nconsumed = min(nin, nblocks * L * P), *max_bits = nblocks * (L + 1), *nbefore_wanted = ntaps (ntaps - 1 for the filter,
 * one for the early instant).  BBB_EINVAL for everything wrong with cfg. */
int bbb_timing_plan(const bbb_timing_cfg *cfg, uint64_t nin, int final, uint64_t *nblocks, uint64_t *nconsumed, uint64_t *max_bits,
                    uint64_t *nbefore_wanted);
/* state_dev: uint64[2] on the device, read at the start and written at the end: [0] bit 63 is `locked`, the low bits are
 * phi of the last block; [1] the bits emitted since reset (added to).  A record cut at multiples of L P, each piece with
 * ntaps samples of history and these words, `final` on the last piece only, gives the bits, soft values, phases and state
 * of one call.  bits_packed_dev: LSB first in u64 words, all ceil(max_bits / 64) words are written, the bits from nbits on
 * are 0.  soft_dev (may be NULL): room for max_bits elements, nbits of them written.  phase_dev (may be NULL):
 * uint8[nblocks], phi_j.  stats_dev (may be NULL): uint64[4], ADDED TO: blocks, moves, wraps up, wraps down.  nbits_dev:
 * one uint64 on the device, written: the count depends on the data, so the host learns it by reading this.  nblocks == 0
 * only rewrites the state; a call that is not final ignores the samples beyond nconsumed.  in_dev as in bbb_fir_filter, of
 * nbefore the nearest ntaps are used.  BBB_EINVAL before the device is touched: everything wrong with cfg (ff's own rules,
 * decim != 1, the ranges above), nulls, misaligned pointers, outputs that overlap the samples read or each other.  The
 * call's scratch (P + 10 bytes per block and some per chunk) comes from the device's memory pool on hip_stream; there is no
 * host round trip inside the call.  Asynchronous; a device without gfx950 gives BBB_ENODEV. */
int bbb_timing_run(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, int final, const bbb_timing_cfg *cfg, uint64_t *state_dev,
                   uint64_t *bits_packed_dev, void *soft_dev, uint8_t *phase_dev, uint64_t *stats_dev, uint64_t *nbits_dev, int device,
                   void *hip_stream);
/* The definition as a plain serial loop over host memory (works without a GPU): in[-1] .. in[-nbefore] readable, state[2],
 * bits_packed / soft / phase / stats as in bbb_timing_run, *nbits_out (may be NULL) the bits emitted. */
int bbb_timing_model_host(const int16_t *in, uint64_t nin, uint32_t nbefore, int final, const bbb_timing_cfg *cfg, uint64_t *state,
                          uint64_t *bits_packed, void *soft, uint8_t *phase, uint64_t *stats, uint64_t *nbits_out);

/* ---- carrier recovery: block phase estimate by squaring, unwrap, derotator, exact whatever the data are ------------------ */

/* bbb_ddc_run's oscillator is a function of the sample number: nothing follows the transmitter's carrier.  With the two a few
 * ppm apart the baseband vector of a BPSK signal turns slowly and neither I nor Q can be decided.  This block estimates the
 * vector's angle block by block, unwraps it and turns every pair back, so that the data axis lands on I.  All integers, >>
 * arithmetic, rom = bbb_nco_rom.
 * in_dev: nin pairs (I, Q) of int16, the element BBB_DDC_IQ16 writes, 4-byte aligned.  L = block_pairs (a multiple of 8 in
 * 8..1024; 0: 32).  Block j is the pairs [j L, (j + 1) L) below nin; nblocks = final ? ceil(nin / L) : floor(nin / L), so only
 * the last block of a final call may be partial; a call that is not final ignores the pairs beyond nblocks * L.
 *   block sums     SR_j = sum(I * I - Q * Q), SI_j = 2 * sum(I * Q) over the block's pairs: int64, at most 2^41 in magnitude
 *                  (I * Q is summed and the sum doubled: 2 * I * Q of (-32768, -32768) does not fit int32)
 *   doubled angle  m = max(|SR|, |SI|), s = max(0, bitlength(m) - 15); theta2_j = the phase of BBB_DDC_POLAR's CORDIC for the
 *                  pair (SR >> s, SI >> s), both of which lie in [-32768, 32767]; (0, 0) gives 0
 *                  h_j = (theta2_j mod 2^16) >> 1, in 0..32767: the carrier's phase modulo half a turn
 *   unwrap         d = (h_j - est_(j-1)) mod 2^16; est_j = h_j if d < 16384 or d >= 49152, else (h_j + 32768) mod 2^16
 *                  est_(-1) = init_phase (uint16, 1/65536 turn) for the first block after reset, else the state's
 *   derotation     of every pair of block j: adr = est_j >> 6, c = rom[(adr + 256) mod 1024], s = rom[adr]
 *                  I' = sat16((I * c + Q * s) >> 15)      Q' = sat16((Q * c - I * s) >> 15)
 *                  (both sums stay below 46341 * 32767 < 2^31)
 *   decision       bit = I' >= threshold (> with strict)
 * Limits.  Squaring removes the data and with it half a turn: est is the carrier's phase or that plus half a turn.  Which one
 * is fixed by init_phase (16384 makes bit 1 positive for a carrier phase-modulated as in the down-converter's example, -512
 * for bit 1) or left to the frame synchroniser's polarity search.  The estimate is constant over a block, so the carrier may
 * turn well below a quarter turn per block; a quarter turn or more per block breaks the unwrap.  BPSK only.
 * chunk_blocks (0: the default) only places the boundaries of the device's work: no output depends on it. */
typedef struct {
    uint32_t block_pairs;      /* L: a multiple of 8 in 8..1024; 0: 32 */
    uint32_t init_phase;       /* est_(-1) out of reset: 0..65535 in 1/65536 turn */
    int32_t  threshold;
    uint32_t strict;
    uint32_t chunk_blocks;     /* blocks one workgroup scans; 0: the default */
} bbb_carrier_cfg;

/* The sizes of a call, from sizes alone (host only, works without a GPU; every output may be NULL): *nblocks as above,
 * *nconsumed = min(nin, nblocks * L).  BBB_EINVAL for everything wrong with cfg, and for nin > 2^58. */
int bbb_carrier_plan(const bbb_carrier_cfg *cfg, uint64_t nin, int final, uint64_t *nblocks, uint64_t *nconsumed);
/* state_dev: uint64[2] on the device, read at the start and written at the end: [0] bit 63 is `started`, the low 16 bits are
 * est of the last block; [1] the pairs consumed since reset (added to).  A zeroed state is out of reset.  A record cut at
 * multiples of L and continued with these words, `final` on the last piece only, gives the outputs, stats and state of one
 * call, bit for bit.  Outputs, each may be NULL, at least one must be given: iq_dev, nconsumed pairs (I', Q') (4-byte aligned;
 * 16-byte aligned takes the wide stores); bits_packed_dev, LSB first in u64 words, all ceil(nblocks * L / 64) words are
 * written, the bits from nconsumed on are 0; soft_dev, nconsumed int16, I'; phase_dev, uint16[nblocks], est_j.
 * stats_dev (may be NULL): uint64[4], ADDED TO: blocks; blocks whose est changed sides, (est_j >> 15) != (est_(j-1) >> 15);
 * blocks whose sums are both 0; the int64 sum of wrap16(est_j - est_(j-1)), which divided by blocks * L * 65536 is the carrier
 * offset in turns per pair.  nin == 0 or nblocks == 0 only rewrites the state.  BBB_EINVAL before the device is touched:
 * everything wrong with cfg, nulls, no output, nin > 2^58, misaligned pointers, outputs that overlap the pairs read or each
 * other.  The call's scratch (4 bytes per block, 2 per chunk and 16 per workgroup of one pass) comes from the device's memory pool on hip_stream; there is
 * no host round trip inside the call.  Asynchronous; a device without gfx950 gives BBB_ENODEV. */
int bbb_carrier_run(const int16_t *in_dev, uint64_t nin, int final, const bbb_carrier_cfg *cfg, uint64_t *state_dev, int16_t *iq_dev,
                    uint64_t *bits_packed_dev, int16_t *soft_dev, uint16_t *phase_dev, uint64_t *stats_dev, int device,
                    void *hip_stream);
/* The definition as a plain serial loop over host memory (works without a GPU): state[2], iq / bits_packed / soft / phase /
 * stats as in bbb_carrier_run. */
int bbb_carrier_model_host(const int16_t *in, uint64_t nin, int final, const bbb_carrier_cfg *cfg, uint64_t *state, int16_t *iq,
                           uint64_t *bits_packed, int16_t *soft, uint16_t *phase, uint64_t *stats);

/* ---- convolutional codec: encoder, puncturing, Viterbi decoder over soft or hard decisions, exact ---------------------- */

/* Forward error correction for the receiver's decisions: a rate 1/n convolutional code of constraint length K, punctured or
 * not, encoded on the device and decoded by a Viterbi run per block.  All integers.
 *   K 3..7, NS = 2^(K-1) states, n 2..3 coded bits per step; gen[i] nonzero and < 2^K in the CONVENTIONAL notation: bit K-1
 *   of gen[i] weighs the current input bit, bit 0 the oldest, so (0171, 0133) and (7, 5) are written as in the books.
 *   state h   : K-1 bits, bit i = the input bit i + 1 steps back (the DFE's and the MLSE's convention)
 *   r         = (h << 1) | b                                   b the step's input bit
 *   c_i       = parity of the bits j of r for which bit K-1-j of gen[i] is set          coded bit i of the step, i < n
 *   h'        = ((h << 1) | b) & (NS - 1)                      step 0 starts from init_state (masked to K-1 bits)
 * Puncturing: period p is 1..16; coded bit i of ABSOLUTE step t is transmitted iff bit t mod p of keep[i] is set (keep[i] <
 * 2^p; every step keeps at least one bit, so the step count is a function of the value count).  Within a step the kept bits
 * go out in order of i; idx(t) is the number of transmitted bits in front of step t.  The usual patterns of (0171, 0133):
 * rate 2/3 p 2 keep {01b, 11b}; 3/4 p 3 {101b, 011b}; 5/6 p 5 {10101b, 01011b}; 7/8 p 7 {1010001b, 0101111b}.
 * The decoder: received value number idx(t) + (kept bits below i in step t) is r_i of step t, a punctured position and a
 * value in front of the history count as r_i = 0.
 *   gain      = sum_{i < n} r_i d(c_i)                         d(1) = +1, d(0) = -1, maximised over the paths
 * ACS: the predecessors of h' are h = (h' >> 1) | (c << (K-2)), c = 0, 1; the larger m[h] + gain survives, a tie goes to
 * c = 0.  Blocks on ABSOLUTE step numbers exactly as bbb_mlse_run's: block j is the steps [j B, (j + 1) B), decided from ONE
 * Viterbi run over [max(0, j B - W), min(Nend, (j + 1) B + D)).  A window that starts at step 0 gives init_state the metric 0
 * and every other state -2^30, any other window starts every state at 0.  The end state is the largest metric, the lowest
 * index on a tie; with terminated != 0 a window that ends at Nend of a final call ends in state 0 instead (the caller appended
 * K-1 zero bits; their steps are still emitted, dropping them is the caller's business).  The decision of step t is bit 0 of
 * the traced-back path's state behind step t.  B = block_steps, W = warmup_steps, D = lookahead_steps (0: 192, 64, 64) ARE
 * part of the definition; 1 <= B, 1 <= W <= 128, D <= 128, B + W + D <= 512.  final and the non-final rule are bbb_mlse_run's:
 * Nend = first_step + nsteps is known to a final call only, a call that is not final decides the steps below the largest
 * block boundary E with E + D <= first_step + nsteps; first_step may sit anywhere.  The decoder has no state on the device.
 * |gain| <= 3 * 32768 < 2^17 and a window is at most 512 steps: every allowed metric stays below 2^26, int32 is exact. */
#define BBB_CONV_SOFT16 0      /* received values: int16, positive means 1, 0 is an erasure */
#define BBB_CONV_HARD   1      /* received values: packed bits (LSB first in u64 words), a bit counts as +1 / -1 */
typedef struct {
    uint32_t K;                 /* 3..7 */
    uint32_t n;                 /* 2..3 */
    uint32_t gen[3];            /* entries beyond n are ignored */
    uint32_t init_state;        /* the input bits in front of step 0, bit i = step -1 - i */
    uint32_t period;            /* 1..16 */
    uint32_t keep[3];           /* bit t mod period of keep[i]: coded bit i of step t is transmitted */
    uint32_t terminated;        /* decoder only */
    uint32_t block_steps, warmup_steps, lookahead_steps;           /* decoder only; 0: the default */
} bbb_conv_cfg;

/* The sizes of a decoder call, from sizes alone (host only, works without a GPU; the three outputs may be NULL): *nsteps =
 * the largest T with idx(first_step + T) - idx(first_step) <= nin (the values of a step cut short are ignored), *ndecided
 * as above, *nbefore_wanted the history in received values with which the call's first window is not zero-filled:
 * idx(first_step) - idx(the window's first step).  BBB_EINVAL for everything wrong with cfg, nin > 2^60 and first_step +
 * nsteps > 2^58. */
int bbb_conv_plan(const bbb_conv_cfg *cfg, uint64_t nin, uint64_t first_step, int final, uint64_t *nsteps, uint64_t *ndecided,
                  uint64_t *nbefore_wanted);
/* The encoder: bits_dev holds the input bits of the steps [first_step, first_step + nsteps) packed LSB first in u64 words
 * (the layout of bbb_fir_slice).  state_dev: one uint32 on the device, the state h in front of first_step, read at the
 * start and written at the end, so a record encoded in pieces gives the bits of one call (set it to init_state in front of
 * step 0); NULL: the state is cfg->init_state and nothing is written back.  out_dev receives the idx(first_step + nsteps) -
 * idx(first_step) transmitted bits packed from its bit 0 on, the unused bits of the last word 0, words beyond the last
 * untouched; *nout (host, may be NULL) the count.  nsteps = 0 writes nothing.  Termination is the caller appending K-1 zero
 * bits.  BBB_EINVAL before the device is touched: everything wrong with cfg (the decoder's fields included), nulls,
 * misaligned pointers, buffers that overlap, first_step + nsteps > 2^58.  Asynchronous on hip_stream; a device without
 * gfx950 gives BBB_ENODEV. */
int bbb_conv_encode(const uint64_t *bits_dev, uint64_t nsteps, uint64_t first_step, const bbb_conv_cfg *cfg, uint32_t *state_dev,
                    uint64_t *out_dev, uint64_t *nout, int device, void *hip_stream);
/* The same as a plain serial loop over host memory (works without a GPU). */
int bbb_conv_encode_host(const uint64_t *bits, uint64_t nsteps, uint64_t first_step, const bbb_conv_cfg *cfg, uint32_t *state,
                         uint64_t *out, uint64_t *nout);
/* The decoder.  format: BBB_CONV_SOFT16 or BBB_CONV_HARD.  in_dev is the BASE of the received buffer (2-byte aligned int16
 * elements, or 8-byte aligned u64 words of bits); in_first the index (element or bit) of the call's first value, which is
 * received value idx(first_step); nin the values from there on; nbefore <= in_first values of history lie below in_first,
 * of which only what the first window reaches (nbefore_wanted) is read.  bits_packed_dev: the decision of step first_step
 * + k is bit k, the unused bits of the last word 0 (ceil(ndecided / 64) words, 8-byte aligned; words beyond them are not
 * touched).  stats_dev (may be NULL): uint64[2] on the device, ADDED TO: windows walked, steps decided.  *ndecided_out
 * (host, may be NULL) receives ndecided, which is bbb_conv_plan's.  BBB_EINVAL before the device is touched: everything
 * wrong with cfg, an unknown format, nulls, misaligned pointers, an output that overlaps the values read or the other
 * output, first_step + nsteps > 2^58, nin > 2^60, in_first > 2^62, nbefore > in_first.  ndecided = 0 writes nothing.
 * Asynchronous on hip_stream; a device without gfx950 gives BBB_ENODEV. */
int bbb_conv_decode(const void *in_dev, uint64_t in_first, uint64_t nin, uint64_t nbefore, uint64_t first_step, int final, int format,
                    const bbb_conv_cfg *cfg, uint64_t *bits_packed_dev, uint64_t *stats_dev, uint64_t *ndecided_out, int device,
                    void *hip_stream);
/* The definition as a plain serial loop over host memory (works without a GPU); arguments as bbb_conv_decode's. */
int bbb_conv_model_host(const void *in, uint64_t in_first, uint64_t nin, uint64_t nbefore, uint64_t first_step, int final, int format,
                        const bbb_conv_cfg *cfg, uint64_t *bits_packed, uint64_t *ndecided_out);

/* ---- the filtered link: eye, bathtub and BER sweep behind a receive filter (rx.py:24-26) -------------------------------- */

/* What bbb_tx_eye_run and bbb_tx_ber_sweep_run give for the raw sample, for the sample AFTER the receive filter, the
 * waveform and the filtered stream never reaching memory.  With x(n) = bbb_tx_fill_i16 of *base with settings[i]'s coeffs,
 * bit_en, noise_en and noise_var (x(n) = 0 for n < 0):
 *   acc(n) = sum_{i < ntaps} h[i] * x(n - i)     exact int32, the rules of bbb_fir_cfg
 *   z(n)   = sat16(acc(n) >> fir->shift)
 * and the filtered stream re-timed by `delay` (0..255, the filter's group delay): stream sample n is acc(n + delay) /
 * z(n + delay).  counters_dev[i][p] ([nset][8][2] uint64, ADDED TO) is the bathtub of that stream: phase p decides data bit
 * m from stream sample 8m + BBB_TX_BIT_SAMPLE0 + p as acc >= settings[i].threshold (> with strict), the threshold in units
 * of acc as in bbb_fir_slice; only bits m >= 0 whose stream sample lies in the range count.  hist_dev[i] ([nset][256][ncols]
 * uint64, ADDED TO; only when *eye was given at open) is bbb_eye_accumulate_i16 of the values z at their stream sample
 * numbers: eye->ncols, shift and col_origin are used, its threshold and strict are not (each setting carries its own).
 * run covers stream samples [first_sample, first_sample + nsamples); the filter's history in front of first_sample is the
 * true waveform, so the totals do not depend on how a range is cut into calls or chunks.  counters_dev may be NULL when a
 * histogram is filled.  So for taps {1}, shift 0, delay 0 the counters are bbb_tx_ber_sweep_run's and the histogram is
 * bbb_tx_eye_run's; in general a phase's counters are those of bbb_fir_slice at stride 8 on bbb_tx_fill_i16's output.
 * fir->decim must be 1 and fir->phase 0 (BBB_EINVAL otherwise); fir->out_bytes is ignored.  nset is 1..512; every setting is
 * checked as bbb_tx_ber_sweep_open checks it, and every argument before the device is touched.  The noise of a chunk
 * (chunk_samples, 0: 2^26) is generated once, with the filter's history and `delay` samples of overlap between chunks, the
 * data bits once; one launch per setting re-reads them from the cache.  Handles that bbb_tx_fill_i16 refuses with noise on
 * get the same BBB_EUNSUP from run when a setting has noise_en.  Asynchronous on the handle's stream; the handle's own stream
 * position is left as it was.  LIFETIME: as bbb_tx_ber_sweep -- close the object BEFORE bbb_lutopt_destroy of its handle. */
typedef struct bbb_link_sweep bbb_link_sweep;
int bbb_link_sweep_open(bbb_lutopt *h, const bbb_tx_cfg *base, const bbb_tx_setting *settings, int nset, const bbb_fir_cfg *fir,
                        uint32_t delay, const bbb_eye_cfg *eye /* NULL: no histograms */, uint64_t chunk_samples,
                        bbb_link_sweep **out);
int bbb_link_sweep_run(bbb_link_sweep *s, uint64_t first_sample, uint64_t nsamples,
                       uint64_t *counters_dev /* [nset][8][2], added to, may be NULL if hist_dev is not */,
                       uint64_t *hist_dev /* [nset][256][ncols], added to, NULL or eye was NULL: none */);
int bbb_link_sweep_close(bbb_link_sweep *s);

/* ---- GF(2) helpers (host only; the pieces of software/rnghunt this path leans on) ------------ */

/* Berlekamp-Massey (software/rnghunt/src/berlekamp_massey.rs:5-31): minimal polynomial of the bit
 * sequence bits[0..n) (one bit per byte).  coeffs_out[i] (needs n+1 bytes) = coefficient of x^i,
 * *degree = linear complexity.  E.g. the first 19 bits of PRBS9 give x^9 + x^5 + 1 (its test,
 * berlekamp_massey.rs:40-42). */
int bbb_gf2_berlekamp_massey(const uint8_t *bits, uint64_t n, uint8_t *coeffs_out, int64_t *degree);
/* BinaryMatrix::recur (software/rnghunt/src/binary_matrix.rs:68-76) on rnghunt's matrix storage
 * (column-major u64 words, first row in the MSbit, binary_matrix.rs:15-19): out_bits[s] = bit 0 of
 * A^(s+1) x. */
int bbb_gf2_recur(int nrows, int ncols, const uint64_t *col_words, const uint8_t *x_bits, int nsteps,
                  uint8_t *out_bits);

/* BinaryMatrix::dot (binary_matrix.rs:52-63), same storage: out_bits[r] = (A x)[r], nrows bytes. */
int bbb_gf2_dot(int nrows, int ncols, const uint64_t *col_words, const uint8_t *x_bits, uint8_t *out_bits);
/* BinaryPolynomial::is_primitive (software/rnghunt/src/binary_polynomial.rs:178-216).  coeffs[i] is
 * the coefficient of x^(ncoeffs-1-i), the order of BinaryPolynomial::from_coefficients (:48-53).
 * *result = 1 / 0.  The test needs the prime factors of 2^deg - 1: the degrees in
 * basebandboard_amd/data/mersenne_factors.txt are served, others give BBB_EUNSUP. */
int bbb_gf2_poly_is_primitive(const uint8_t *coeffs, int ncoeffs, int *result);
/* BinaryPolynomial::modexp (:135-163): x^e mod p, e = little-endian 64-bit words; out_coeffs has
 * ncoeffs bytes in the same order as coeffs. */
int bbb_gf2_poly_modexp(const uint8_t *coeffs, int ncoeffs, const uint64_t *exponent_words, int nwords,
                        uint8_t *out_coeffs);
/* The polynomial rnghunt's search examines for a recurrence (src/bin/rnghunt.rs:27-38): bit 0 of 2k
 * successive states from the all-ones vector, reversed, through Berlekamp-Massey.  coeffs_out needs
 * 2k+1 bytes (the reversed sequence of a singular matrix can have complexity above k); entries
 * 0..*degree are the coefficients, highest power first. */
int bbb_lutopt_charpoly(int k, const uint16_t *taps, const uint32_t *row_off, uint8_t *coeffs_out, int *degree);
/* Its acceptance test (rnghunt.rs:40-46): degree == k and primitive, i.e. period 2^k - 1. */
int bbb_lutopt_is_full_period(int k, const uint16_t *taps, const uint32_t *row_off, int *result);
/* Its output file (rnghunt.rs:51-53): k lines of k characters, line r character c = A[r][c]; read
 * back by bbb_lutopt_load_matrix_file and by the reference's util/pack.py, util/verify.py. */
int bbb_lutopt_save_matrix_file(const char *path, int k, const uint16_t *taps, const uint32_t *row_off);

/* ---- the recurrence search of software/rnghunt, on the GPU ----------------------------------- */

/* Candidate number `candidate` of `seed`: a random k x k matrix with 3 or 4 ones per row (weights
 * drawn from [3,4,4,4,4,4,4,4], rnghunt.rs:25) and balanced column weights
 * (BinaryMatrix::random, binary_matrix.rs:81-101), from a counter-based generator so that it is the
 * same matrix on every host and device (the reference's thread_rng is unseeded; see
 * csrc/search_rng.hpp for the construction).  taps_out needs 4k entries, row_off_out k+1. */
int bbb_lutopt_search_candidate(int k, uint64_t seed, uint64_t candidate, uint16_t *taps_out, uint32_t *row_off_out);
typedef struct {
    uint64_t tested;          /* candidates examined */
    uint64_t full_degree;     /* of those: characteristic polynomial of degree k (rnghunt.rs:40) */
    uint64_t order_divides;   /* of those: x^(2^k - 1) = 1 (first check of is_primitive) */
    uint64_t primitive;       /* of those: primitive = accepted */
    uint64_t kernel_ns;       /* duration of the search kernel (HIP events); the call adds the host re-check of a hit */
} bbb_search_stats;
/* Examine candidates first_candidate .. first_candidate + ncandidates - 1 on the GPU, one per
 * wavefront at a time: build the matrix, run 2k steps from the all-ones state, Berlekamp-Massey,
 * degree check, primitivity test (the loop body of rnghunt.rs:23-47).  *found_index receives the
 * SMALLEST accepted candidate number (UINT64_MAX if none), its taps go to taps_out / row_off_out (host,
 * may be NULL) after a re-check with the host arithmetic above.  k must be a multiple of 64 in
 * 64..512 or 16 or 32, with an entry in the factor table.  *stats is a host result. */
int bbb_lutopt_search(int k, uint64_t seed, uint64_t first_candidate, uint64_t ncandidates, uint64_t *found_index,
                      uint16_t *taps_out, uint32_t *row_off_out, bbb_search_stats *stats, int device, void *hip_stream);

/* ---- error statistics of a packed error stream: gaps, bursts, errored blocks ------------------ */

/* How the errors of a packed stream (bit t at word t/64, bit t%64: the layout of bbb_prbs_fill and of
 * bbb_prbs_detector_stream's err_packed_dev) are distributed.  The error positions are the t with err[t] & ~mask[t]; with
 * mask = the detector's reload stream these are the clocks bbb_detector_stats.errors counts.  Positions are absolute over the life of
 * an object: the first bit of the first call is position 0 and every call continues where the previous one ended.  With the
 * positions e_0 < e_1 < ...:
 *   bin(v) = v for v < 256, 256 + floor(log2 v) - 8 above: every histogram has BBB_ERRSTAT_NBINS entries, entry 0 stays 0.
 *   gaps:   g_i = e_i - e_(i-1), gap_hist[bin(g_i)]++, max_gap; the stretches before e_0 and behind the last error are no gaps.
 *   bursts: one starts at e_0 and at every e_i with g_i > guard (guard 0: every error is its own burst) and is closed when the
 *           next one starts: first f, last l, w errors give burst_len_hist[bin(l - f + 1)]++, burst_weight_hist[bin(w)]++,
 *           bursts++, burst_len_sum += l - f + 1 and the two maxima.  The burst still open at the end of the data is in none of
 *           these: it is open_first, open_last, open_weight (0: there is none); closing it is the caller's decision.
 *   blocks: errored_blocks[j] = number of distinct floor(e_i / block_bits[j]) (blocks aligned to position 0; 0: unused entry).
 * All counters and the carried state (the previous error, the open burst, the running position) live on the device:
 * accumulate and skip do not synchronise.  Pointers need 8-byte alignment.  nbits = 0 is a valid no-op; bits beyond nbits in
 * the last word are ignored.  A call whose nbits is not a multiple of 64 ends the record: every later accumulate or skip returns
 * BBB_EINVAL until reset.  Bad cfgs (BBB_EINVAL, checked before the device): nblock > 4, a used block_bits outside [1, 2^40). */
#define BBB_ERRSTAT_NBINS 312
typedef struct { uint32_t guard; uint32_t nblock; uint64_t block_bits[4]; } bbb_errstat_cfg;
typedef struct {
    uint64_t bits, errors, first_error, last_error, max_gap;
    uint64_t bursts, burst_len_sum, max_burst_len, max_burst_weight;
    uint64_t open_first, open_last, open_weight;
    uint64_t errored_blocks[4];
    uint64_t gap_hist[BBB_ERRSTAT_NBINS], burst_len_hist[BBB_ERRSTAT_NBINS], burst_weight_hist[BBB_ERRSTAT_NBINS];
} bbb_errstat_result;
typedef struct bbb_errstat bbb_errstat;
int bbb_errstat_open(const bbb_errstat_cfg *cfg, int device, void *hip_stream, bbb_errstat **out);
int bbb_errstat_accumulate(bbb_errstat *e, const uint64_t *err_packed_dev, const uint64_t *mask_packed_dev /* may be NULL */,
                           uint64_t nbits);
int bbb_errstat_skip(bbb_errstat *e, uint64_t nbits);            /* nbits error-free positions that are not read */
int bbb_errstat_read(bbb_errstat *e, bbb_errstat_result *out);   /* host result; synchronises the stream */
int bbb_errstat_reset(bbb_errstat *e);
/* Later calls run on hip_stream, ordered behind what is queued on the old one. */
int bbb_errstat_set_stream(bbb_errstat *e, void *hip_stream);
/* Host only: the bits one workgroup (tile) and one wavefront of the kernel cover, both multiples of 64. */
int bbb_errstat_geometry(uint64_t *tile_bits, uint64_t *wave_bits);
int bbb_errstat_close(bbb_errstat *e);

/* ---- Reed-Solomon codec over GF(2^8) with symbol interleaving --------------------------------- */

/* The outer code behind the Viterbi decoder (bbb_conv_decode), whose errors come in bursts.
 * Field: GF(2^8) defined by prim_poly (9 bits, bit 8 set, x of order 255: 0x11D and 0x187 are the usual ones); alpha = x.
 * Code:  nroots even, 2..32, t = nroots / 2; n = nroots + 1 .. 255 the codeword length (below 255: a shortened code, whose
 *        missing leading symbols are zero and never stored); k = n - nroots; fcr 0..254; prim 1..254 with gcd(prim, 255) = 1;
 *        g(x) = prod_{i < nroots} (x - alpha^(prim (fcr + i))).  Systematic: symbol 0 of a codeword is the coefficient of
 *        x^(n-1), the k data symbols come first, then the nroots parity symbols (the convention of the common software codecs).
 *        (255, 223) with 0x187, fcr 112, prim 11 is the CCSDS code in the conventional basis.
 * Interleaving: depth I = 1..8.  A coded frame is I n bytes, byte j is symbol j / I of codeword j % I: the I k data bytes
 *        unchanged, then I nroots parity bytes.  The encoder's input frame and the decoder's output frame are those I k data
 *        bytes.  Frame f starts at byte f I n (coded) or f I k (data); no alignment is assumed.
 * Bytes: byte j of a buffer is bits 8j .. 8j + 7 of the packed bit streams (LSB first in u64 words): the little-endian byte
 *        view of what bbb_conv_decode writes.
 * Decoder: bounded distance.  If a codeword of the (shortened) code lies within t symbols of the received word it is unique:
 *        its data symbols are the output, nerr the number of symbols that differ (0..t), "bits corrected" the popcount of the
 *        differences.  Otherwise the codeword FAILED: the received data symbols pass through unchanged and nerr = 255 (in
 *        terms of the error locator: a degree above t, fewer roots than the degree among the n stored positions, or a root
 *        in a padded position).  Beyond t errors the word found may be another codeword than the one sent.
 * Out of scope: erasures, soft-decision decoding, the CCSDS dual basis, convolutional interleavers.  (Frames that do not start
 *        at byte 0: bbb_framesync_run and bbb_frame_extract below.)
 *
 * nerr (may be NULL): one byte per codeword at index f I + c.  stats (may be NULL, 8-byte aligned) is uint64[BBB_RS_NSTATS],
 * ADDED TO: codewords, clean codewords, failed codewords, symbols corrected, bits corrected.  nframes = 0 writes nothing.
 * The device calls are asynchronous on hip_stream and keep no state.  BBB_EINVAL (with a detail, before the device is touched):
 * anything wrong with cfg (a prim_poly that is not primitive included; reserved must be 0), null pointers, a misaligned
 * stats_dev, an output that overlaps the input or another output, nframes I n > 2^40. */
#define BBB_RS_NSTATS 5
#define BBB_RS_FAILED 255
typedef struct {
    uint32_t prim_poly, fcr, prim, nroots, n, depth;
    uint32_t reserved[2];
} bbb_rs_cfg;
int bbb_rs_encode(const uint8_t *data_dev, uint64_t nframes, const bbb_rs_cfg *cfg, uint8_t *out_dev, int device, void *hip_stream);
/* The same as a serial loop over host memory; works without a GPU. */
int bbb_rs_encode_host(const uint8_t *data, uint64_t nframes, const bbb_rs_cfg *cfg, uint8_t *out);
int bbb_rs_decode(const uint8_t *in_dev, uint64_t nframes, const bbb_rs_cfg *cfg, uint8_t *data_dev, uint8_t *nerr_dev /* may be NULL */,
                  uint64_t *stats_dev /* may be NULL */, int device, void *hip_stream);
/* The decoder's definition as an independent serial loop over host memory; works without a GPU. */
int bbb_rs_model_host(const uint8_t *in, uint64_t nframes, const bbb_rs_cfg *cfg, uint8_t *data, uint8_t *nerr /* may be NULL */,
                      uint64_t *stats /* may be NULL */);

/* ---- LDPC codec: quasi-cyclic codes, layered normalised min-sum decoder, triangular encoder ---- */

/* An iteratively decoded block code for the receiver's soft or hard decisions.  All integers.
 * Code:  a base matrix base[j][c], j < J block rows, c < K block columns of Z x Z circulants (row-major J x K in cfg->base).
 *        Entry -1 is the zero block, entry s in 0..Z-1 the identity shifted by s: check j Z + r involves variable
 *        c Z + (r + s) mod Z.  n = K Z coded bits, m = J Z checks, k = (K - J) Z data bits; systematic, data first.
 *        Bounds (part of the ABI): Z 2..512, J 1..32, J < K <= 64, n <= 16384, m <= 8192, every block row holds 2..32 entries
 *        >= 0, every block column at least one, entries lie in -1..Z-1.  Cycles are not checked.
 * Decoder: received values as bbb_conv_decode's: BBB_CONV_SOFT16 (int16, positive means 1, 0 an erasure) or BBB_CONV_HARD
 *        (packed bits, a bit counts as +hard_mag / -hard_mag).  Per codeword, with r[v] its n values:
 *          P[v] = clamp(r[v], +-32767), R[c][e] = 0 for every check c and every edge e of it; hard(v) = P[v] > 0.
 *          If every check of hard is satisfied the codeword is done with iters = 0.  Otherwise for it = 0 .. max_iter - 1:
 *            for j = 0 .. J - 1 in this order, for every row r < Z of layer j (check c = j Z + r; its edges e run over the
 *            entries >= 0 of block row j by ascending column, v_e the variable of edge e):
 *              Q_e = clamp(P[v_e] - R[c][e], +-32767), b_e = Q_e > 0, S = XOR of the b_e
 *              i1 = the lowest e with the smallest |Q_e|, m1 that value, m2 the smallest |Q_e| over e != i1
 *              a_e = ((e == i1 ? m2 : m1) * norm) >> 4
 *              R[c][e] = (S ^ b_e) ? +a_e : -a_e,  P[v_e] = clamp(Q_e + R[c][e], +-32767)
 *            after layer J - 1: if every check of hard is satisfied, stop with iters = it + 1.
 *          After max_iter iterations without that the codeword has FAILED: iters = 255 (BBB_LDPC_FAILED).
 *          The output is hard(v) for v < k of the final P in every case.
 *        A block column has at most one circulant in a block row, so the checks of a layer touch disjoint variables: their order
 *        within the layer does not matter, and the device runs them at once.  Storing R as (m1 norm >> 4, m2 norm >> 4, i1 and
 *        the bits S ^ b_e) is equivalent, and is what the device keeps.  max_iter 1..64; norm 1..16, 0 means 12; hard_mag
 *        1..32767, 0 means 32.  |Q_e + R| < 2^17: int32 is exact throughout.
 * Encoder: for codes whose parity part is block upper triangular: base[j][K-J+i] = -1 for i < j and >= 0 for i = j.  x[0..k)
 *        is the data; for j = J - 1 down to 0, for r < Z: t_r = the XOR, over the entries of row j other than (j, K-J+j), of
 *        x[c Z + (r + s) mod Z]; then x[(K-J+j) Z + (r + s_jj) mod Z] = t_r.  Other base matrices decode but do not encode
 *        (BBB_EINVAL, "parity part not triangular").  The triangular array code array(p, J, K) needs no table: p an odd prime,
 *        Z = p, J < K <= p, base[j][c] = j (c + J - j) mod p for c < K - J, parity column i: j (i - j) mod p for i >= j, else -1.
 * Layouts: codeword w's values are elements in_first + w n ... of in_dev (bits for HARD), in_dev the BASE of the buffer,
 *        2-byte aligned for SOFT16 and 8-byte aligned for HARD.  Decoded data are packed contiguously: codeword w's bit i is bit
 *        w k + i of bits_packed_dev (8-byte aligned, LSB first in u64 words), the unused bits of the last word 0, words beyond it
 *        untouched; nothing depends on the buffer's old contents.  The encoder reads data in that layout and writes codeword
 *        w's bit i to bit w n + i of out_dev, packed the same way.
 * Outputs: iters_dev (may be NULL): one byte per codeword.  stats_dev (may be NULL, 8-byte aligned): uint64[BBB_LDPC_NSTATS],
 *        ADDED TO: codewords, clean (iters 0), failed, iterations summed over the converged codewords, bits corrected (the
 *        popcount over all n bits of (clamped r > 0) ^ hard, over the converged codewords).
 * Codewords are independent and there is no device state: any cutting of a record at codeword boundaries gives the outputs
 * of one call.  ncodewords = 0 writes nothing.  The device calls are asynchronous on hip_stream.  BBB_EINVAL (with a detail,
 * before the device is touched): every bound above, reserved != 0, an unknown format, null or misaligned pointers, any two
 * buffers that overlap, ncodewords n > 2^40, in_first > 2^62.  A device without gfx950 gives BBB_ENODEV.
 * Out of scope: puncturing, shortening, dual-diagonal and accumulator encoders, soft outputs, flooding schedules. */
#define BBB_LDPC_NSTATS 5
#define BBB_LDPC_FAILED 255
#define BBB_LDPC_MAX_J 32
#define BBB_LDPC_MAX_K 64
typedef struct {
    uint32_t Z, J, K;
    uint32_t max_iter, norm, hard_mag;
    uint32_t reserved[2];
    int16_t  base[BBB_LDPC_MAX_J * BBB_LDPC_MAX_K];   /* row-major J x K: base[j * K + c]; entries beyond J K are ignored */
} bbb_ldpc_cfg;
int bbb_ldpc_decode(const void *in_dev, uint64_t in_first, uint64_t ncodewords, int format, const bbb_ldpc_cfg *cfg,
                    uint64_t *bits_packed_dev, uint8_t *iters_dev /* may be NULL */, uint64_t *stats_dev /* may be NULL */, int device,
                    void *hip_stream);
int bbb_ldpc_encode(const uint64_t *bits_dev, uint64_t ncodewords, const bbb_ldpc_cfg *cfg, uint64_t *out_dev, int device,
                    void *hip_stream);
/* The decoder's definition as a plain serial loop over host memory with R kept per edge; works without a GPU. */
int bbb_ldpc_model_host(const void *in, uint64_t in_first, uint64_t ncodewords, int format, const bbb_ldpc_cfg *cfg,
                        uint64_t *bits_packed, uint8_t *iters /* may be NULL */, uint64_t *stats /* may be NULL */);
/* The encoder as a serial loop over host memory; works without a GPU. */
int bbb_ldpc_encode_host(const uint64_t *bits, uint64_t ncodewords, const bbb_ldpc_cfg *cfg, uint64_t *out);

/* ---- Frame synchroniser: marker search, lock, derandomiser ------------------------------------ */

/* Finds the frames of a packed bit stream that starts anywhere: in front of bbb_rs_decode, behind bbb_conv_decode.
 * Bit order: stream bit j is bit j % 64 of word j / 64; byte j of a buffer is stream bits 8j .. 8j + 7, bit 8j the least
 *        significant.  Positions are ABSOLUTE: bit 0 of a call's data is position first_bit, N = first_bit + nbits its end.
 * Config: marker: bit i is compared with stream bit p + i; marker_bits M 8..64 (bits of marker above M must be 0); frame_bits F,
 *        marker included, M + 8 <= F <= 2^20; tol_search <= tol_lock <= M / 4; verify v 0..7; flywheel w 0..7; both_polarities
 *        0 or 1; rand_poly 0 (no randomiser) or 9 bits with the x^8 and x^0 terms set; rand_seed 1..255 (looked at only with a
 *        rand_poly); reserved 0.
 * Distance: dist(p, pol) = the number of i < M with bit[p + i] != marker_i ^ pol; a position whose marker does not lie wholly
 *        inside the data (p + M > N) has distance M + 1.  pol is 0, or also 1 with both_polarities.  As tol_lock <= M / 4 a
 *        position is within tolerance in one polarity at most.
 * The machine is serial and causal; this is the definition.
 *   SEARCH at s: the smallest p >= s and a pol with dist(p, pol) <= tol_search (a CANDIDATE) and dist(p + j F, pol) <=
 *        tol_lock for j = 1..v: acquisitions += 1, go to LOCK at e = p with that polarity and 0 misses.  Every candidate
 *        passed over because a confirmation failed: rejected += 1.
 *   LOCK at e: a step is taken when e + F <= N.  dist(e, pol) <= tol_lock: misses = 0, the frame at e is emitted.  Otherwise
 *        misses += 1; if misses > w the lock is lost: nothing is emitted, losses += 1, misses = 0, SEARCH at s = e; else the
 *        frame is emitted as flywheeled.  After an emitted frame e += F.
 *   A call that is not final stops at the first point it cannot decide yet and leaves its state there: a position p in SEARCH
 *        needs p + M <= N, a candidate p + v F + M <= N, a LOCK step e + F <= N.  So it never needs bits older than
 *        N - (max(v, 1) F + M): a stream can hold back that many bits, rounded up to words (bbb_framesync_plan).
 *   A final call: what lies beyond N is no hit (a candidate whose confirmation does not lie inside the data is rejected), a
 *        frame that does not end inside the data is not emitted; SEARCH ends at the first p >= s with p + M > N.
 *   Cutting invariance: any cutting of a record into non-final calls plus one final call gives the frames, counters and state
 *        of one final call.  Each call's data must begin at or before the state's position.
 * State: uint64[BBB_FRAMESYNC_NSTATE] on the device, all zero = SEARCH at 0.  Word 0 packs: bits 0..7 mode (0 SEARCH, 1 LOCK; a
 *        state with another mode, or with bits set that are not named here, was not written by these calls: undefined),
 *        bit 8 polarity, bit 9 "the next frame emitted is the first of its acquisition", bits 16..23 misses, bit 24 overflow
 *        (more frames than max_frames in some call), bit 25 ERROR (the data began behind the state's position: the call set
 *        this bit and wrote nothing else; sticky), bits 32..63 the frames the LAST call emitted (written or not).  Word 1: the
 *        position (s or e).  Words 2..7, added to: frames, flywheeled, acquisitions, losses, rejected, marker_bit_errors (the
 *        sum of the distances of the emitted frames that were hits).
 * Records: a call writes its frames from index 0, in order: pos[i] the absolute position of the marker's first bit; meta[i]
 *        bits 0..6 the distance in the episode's polarity, bit 8 the polarity, bit 9 flywheeled, bit 10 first frame of an
 *        acquisition.  Beyond max_frames frames are counted but not written and the overflow bit is set.
 * Randomiser: the register s starts at rand_seed at every frame; a step gives the bit s & 1 and then s = s >> 1 | parity(s &
 *        rand_poly & 0xFF) << 7.  The bits are packed into table bytes most significant first, so the table equals the
 *        standards' byte tables: x^8 + x^7 + x^5 + x^3 + 1 (0x1A9) from 0xFF gives FF 48 0E C0 9A 0D 70 BC ..., period 255.
 *        Table byte j % period is XORed onto payload byte j (payload byte j = frame bits M + 8j .. M + 8j + 7).
 * CCSDS preset: the buffer bytes 1A CF FC 1D, that is marker = 0x1DFCCF1A, M = 32, the randomiser above, F = 32 + 8 depth 255.
 *        This is CCSDS at the BYTE level: the order of the bits within a byte on the channel is this project's (least
 *        significant first), not the standard's.
 * Out of scope: bit-slip windows in lock, node synchronisation of the inner code (which received bit is the first of a step),
 *        soft-decision correlation, convolutional interleavers, markers longer than 64 bits.
 *
 * bbb_framesync_plan (host only): the scratch of a run over nbits, the hold-back in bits (a multiple of 64) and the bits one
 * workgroup of the search pass covers (a multiple of 64), so that tests can aim at its boundaries.
 * bbb_framesync_run: asynchronous on hip_stream, no host round trip.  in_packed_dev: ceil(nbits / 64) words, 8-byte aligned;
 * state_dev 8-byte, pos_dev 8-byte, meta_dev 2-byte, scratch_dev 8-byte aligned, scratch of plan's size.
 * bbb_frame_extract: the payloads of the first min(frames of the last call, max_frames) records, frame i at out[i (F - M) / 8 ...]:
 * complemented where the record's polarity bit is set, then derandomised.  The count is read from state_dev on the device.
 * Needs (F - M) % 8 == 0 and out_dev 8-byte aligned with room for max_frames payloads; a record that does not lie inside the
 * data gives a payload of zeros.
 * bbb_frame_attach: frame i (marker, then the randomised payload i) at bit i F of out_packed_dev, ceil(nframes F / 64) words
 * (the bits behind the last frame are 0); payload i is the (F - M) / 8 bytes at payload_dev + i (F - M) / 8.
 * The *_host forms are the same as plain serial loops over host memory (state, records and all); they share no code with the
 * kernels and work without a GPU.
 * BBB_EINVAL (with a detail, before the device is touched): everything wrong with cfg, null or misaligned pointers, any two
 * buffers of a call that overlap (outputs with inputs and with each other, and, stricter than needed, two inputs), nbits > 2^35, first_bit + nbits > 2^48, nframes F > 2^40. */
#define BBB_FRAMESYNC_NSTATE 8
#define BBB_FRAMESYNC_ERROR (1ull << 25)
#define BBB_FRAMESYNC_OVERFLOW (1ull << 24)
typedef struct {
    uint64_t marker;
    uint32_t marker_bits, frame_bits, tol_search, tol_lock, verify, flywheel, both_polarities, rand_poly, rand_seed;
    uint32_t reserved[3];
} bbb_framesync_cfg;
typedef struct {
    uint64_t scratch_bytes, holdback_bits, tile_bits;
} bbb_framesync_plan_out;
int bbb_framesync_plan(uint64_t nbits, const bbb_framesync_cfg *cfg, bbb_framesync_plan_out *out);
int bbb_framesync_run(const uint64_t *in_packed_dev, uint64_t nbits, uint64_t first_bit, int final, const bbb_framesync_cfg *cfg,
                      uint64_t *state_dev, uint64_t *pos_dev, uint16_t *meta_dev, uint64_t max_frames, void *scratch_dev, int device,
                      void *hip_stream);
int bbb_frame_extract(const uint64_t *in_packed_dev, uint64_t nbits, uint64_t first_bit, const uint64_t *pos_dev, const uint16_t *meta_dev,
                      const uint64_t *state_dev, uint64_t max_frames, const bbb_framesync_cfg *cfg, uint8_t *out_dev, int device,
                      void *hip_stream);
int bbb_frame_attach(const uint8_t *payload_dev, uint64_t nframes, const bbb_framesync_cfg *cfg, uint64_t *out_packed_dev, int device,
                     void *hip_stream);
int bbb_framesync_model_host(const uint64_t *in_packed, uint64_t nbits, uint64_t first_bit, int final, const bbb_framesync_cfg *cfg,
                             uint64_t *state, uint64_t *pos, uint16_t *meta, uint64_t max_frames);
int bbb_frame_extract_host(const uint64_t *in_packed, uint64_t nbits, uint64_t first_bit, const uint64_t *pos, const uint16_t *meta,
                           const uint64_t *state, uint64_t max_frames, const bbb_framesync_cfg *cfg, uint8_t *out);
int bbb_frame_attach_host(const uint8_t *payload, uint64_t nframes, const bbb_framesync_cfg *cfg, uint64_t *out_packed);

#ifdef __cplusplus
}
#endif
#endif /* BBB_H */
