// timing_launch.hpp -- what timing_api.hip hands to timing_kernels.hip: the launch structure of one bbb_timing_run.
#pragma once
#include "bbb_common.hpp"
#include "timing_common.hpp"

namespace bbb {

// timing_kernels.hip: the symbol timing recovery (include/bbb.h, bbb_timing_run)
struct TimingLaunch {                             // one call: in, nbefore, in_vec, ngroups, taps as FirLaunch; nin is g.nin
    const int16_t *in;
    uint32_t nbefore, ngroups, shift;
    int in_vec;
    TimingGeom g;
    uint32_t split;                               // timing_split(P, LP)
    int32_t threshold, strict;
    uint32_t init_phase;                          // < P, or kTimingAcquire
    uint64_t *state;                              // [2], read by the chunk and chain kernels, written by the chain
    uint64_t *bits;                               // ceil(max_bits / 64) zeroed words
    void *soft;                                   // max_bits int16 (soft_bytes 2) or int32 (4), or nullptr
    uint32_t soft_bytes;
    uint8_t *phase;                               // [nblocks], or nullptr
    uint64_t *stats;                              // [4] added to, or nullptr
    uint64_t *nbits;                              // one word, written
    // the call's scratch
    uint64_t *hdr;                                // [0]: the call's block 0 is a first block after reset; [1]: its arg-max
    uint64_t *boff;                               // [nblocks] the output bit of a block's first instant
    uint64_t *coff;                               // [nchunks] the same of a chunk
    uint32_t *cbits;                              // [nchunks][P] the bits a chunk emits, entered in phase p
    uint16_t *binfo;                              // [nblocks] timing_info
    uint8_t *mv;                                  // [nblocks][P] a block's map: the move + 1
    uint8_t *cmap;                                // [nchunks][P] a chunk's map
    uint8_t *cstart;                              // [nchunks] the phase a chunk is entered in
    uint32_t taps[BBB_FIR_MAX_TAPS / 2];
};

// the scratch of a call in uint64 words, and where its arrays lie in it
struct TimingScratch {
    size_t hdr, boff, coff, cbits, binfo, mv, cmap, cstart, words;
};
inline TimingScratch timing_scratch(uint64_t nblocks, uint64_t nchunks, uint32_t P) {
    TimingScratch s;
    size_t w = 0;
    auto take = [&](uint64_t bytes) {
        const size_t at = w;
        w += (size_t)((bytes + 7) / 8);
        return at;
    };
    s.hdr = take(16);
    s.boff = take(8 * nblocks);
    s.coff = take(8 * nchunks);
    s.cbits = take(4 * nchunks * P);
    s.binfo = take(2 * nblocks);
    s.mv = take(nblocks * P);
    s.cmap = take(nchunks * P);
    s.cstart = take(nchunks);
    s.words = w;
    return s;
}

// the metric, chunk, chain, walk and gather kernels of one call, in that order on st
int timing_launch(const TimingLaunch &a, int cus, hipStream_t st);

}  // namespace bbb
