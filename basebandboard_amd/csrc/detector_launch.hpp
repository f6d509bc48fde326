// detector_launch.hpp -- what detector_api.hip hands to detector_kernels.hip: the launch structure of one
// bbb_prbs_detector_stream call and one launcher per stage the scheduler queues.
#pragma once
#include "bbb_common.hpp"

namespace bbb {

struct DetState;                                  // detector_kernels.hip: a chunk's machine state and its four counters
struct DetCount;
constexpr size_t kDetStateBytes = 16, kDetCountBytes = 32;
constexpr int kDetFusedMaxChunkWords = 1024;      // the longest chunk det_fused_kernel's flag words in LDS are sized for
bool det_k_ok(int k);                             // det_tap_of(k) != 0: a PRBS length the detector is built for
bool det_sparse_ok(int k);                        // DetLag<K>::OK: the word recurrence needs at most three history words

struct DetLaunch {                                // one call; every launcher reads the fields its kernel takes
    const uint64_t *src;
    uint64_t nbits, nwords, chunk_words, warm_words, nchunks;
    DetState *spec, *endst;                       // [nchunks] each: the speculative start and the end of every chunk
    DetCount *counts;                             // [nchunks]
    uint64_t *flags;                              // the two-kernel form's clean-word flags, four words per 256 words of src
    uint64_t *err, *reload;                       // nwords each, or nullptr
    int tiles_ok;                                 // the dense pass may load whole 128-byte rows
};

// The launchers queue on st with the grid they are given and check nothing: the call's one hipGetLastError is the scheduler's.
enum DetForm { kDetFused, kDetTwoKernels, kDetDenseOut, kDetDenseTotals };
// the speculative run of every chunk; cgrid: the classify kernel's blocks (kDetTwoKernels only)
int det_first_pass_launch(int k, DetForm form, const DetLaunch &a, unsigned grid, unsigned cgrid, hipStream_t st);
// verify the chain and sum the counters: totals[0..3], the inconsistent chunks in list[0 .. *nlist); returns at once when
// skip_if_zero is given and points at zero
int det_reduce_launch(const DetLaunch &a, unsigned rgrid, uint64_t *totals, unsigned *list, unsigned *nlist, const unsigned *skip_if_zero,
                      hipStream_t st);
// the listed chunks again from their predecessors' ends: nlist of them, or *nlist_dev if that is given and smaller
int det_rerun_launch(int k, const DetLaunch &a, unsigned grid, const unsigned *list, unsigned nlist, const unsigned *nlist_dev, hipStream_t st);
// one lane from chunk c0 to where the chain is consistent again
int det_serial_launch(int k, const DetLaunch &a, uint64_t c0, hipStream_t st);

// detector_api.hip: the geometry of a call, from its arguments and the device's CU count alone (ncu is looked at when
// chunk_bits == 0 only).  BBB_EINVAL with a detail for a chunk_bits that is no multiple of 64 and for too many chunks.
struct DetPlan {
    uint64_t nwords, chunk_words, warm_words, nchunks;
    int tiles_ok;
    bool sparse, fused;                           // the sparse pass; as one kernel (else classify + sparse)
    unsigned grid, rgrid, cgrid;
    size_t o_spec, o_end, o_cnt, o_list, o_tail, o_flags, total;     // the workspace: spec | endst | counts | lists | tails | flags
};
int det_plan(int k, const void *src, uint64_t nbits, uint64_t chunk_bits, uint64_t warm_bits, int ncu, DetPlan *p);

}  // namespace bbb
