// conv_launch.hpp -- what conv_api.hip hands to conv_kernels.hip: the launch structures of bbb_conv_decode and bbb_conv_encode.
#pragma once
#include "bbb_common.hpp"
#include "conv_common.hpp"

namespace bbb {

// conv_kernels.hip: the Viterbi decoder (include/bbb.h, bbb_conv_decode)
struct ConvLaunch {
    const void *in;                               // the buffer's base: int16 elements or u64 words of bits
    int hard;
    uint64_t in_first;                            // the element / bit of received value idx(first)
    int64_t rel_lo, rel_hi;                       // the values that exist, counted from in_first: -history .. idx(end) - idx(first)
    uint64_t idx_first;                           // idx(first)
    uint32_t K, n;
    uint32_t gen[kConvMaxN];
    uint32_t init_state;                          // masked to K - 1 bits
    int forced_end;                               // terminated and final: a window that ends at the call's end ends in state 0
    ConvPunct punct;
    MlseGeom geom;
    uint64_t first, nsteps, ndecided;             // the call's steps [first, first + nsteps), of which ndecided >= 1 are emitted
    uint64_t j0, nblocks;                         // the blocks that hold the emitted steps: j0 .. j0 + nblocks - 1
    uint64_t *bits;                               // ceil(ndecided / 64) zeroed words
    uint64_t *stats;                              // [2] added to, or nullptr
};

// the one kernel of a decoder call on st
int conv_decode_launch(const ConvLaunch &a, int cus, hipStream_t st);

// bbb_conv_encode
struct ConvEncodeLaunch {
    const uint64_t *bits;                         // the input bits of the steps [first, first + nsteps)
    uint64_t first, nsteps, idx_first, nout;      // nout = idx(first + nsteps) - idx(first) >= 1
    uint32_t K, n;
    uint32_t gen[kConvMaxN];
    uint32_t init_state;                          // the state when `state` is null
    uint32_t *state;                              // read by the encode kernel, written by the kernel behind it; may be null
    ConvPunct punct;
    uint64_t *out;                                // ceil(nout / 64) words, every one written whole
};

// the encode kernel and, when there is a state word, the one thread that moves it on
int conv_encode_launch(const ConvEncodeLaunch &a, hipStream_t st);

}  // namespace bbb
