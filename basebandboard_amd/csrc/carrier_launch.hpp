// carrier_launch.hpp -- what carrier_api.hip hands to carrier_kernels.hip: the launch structure of one bbb_carrier_run.
#pragma once
#include "bbb_common.hpp"
#include "carrier_common.hpp"

namespace bbb {

// carrier_kernels.hip: the carrier recovery (include/bbb.h, bbb_carrier_run)
struct CarrierLaunch {
    const int16_t *in;                            // g.nin pairs (I, Q), 4-byte aligned
    int in_vec;                                   // in is 16-byte aligned
    CarrierGeom g;
    uint32_t init_phase;
    int32_t threshold, strict;
    uint64_t *state;                              // [2], read by the flag and chain kernels, written by the chain
    int16_t *iq;                                  // g.nin pairs, or nullptr
    uint64_t *bits;                               // carrier_bit_words words, or nullptr
    int16_t *soft;                                // g.nin values, or nullptr
    uint16_t *phase;                              // [nblocks], or nullptr
    uint64_t *stats;                              // [4] added to, or nullptr
    int iq_vec, soft_vec;                         // iq, soft are 16-byte aligned
    // the call's scratch
    uint16_t *h;                                  // [nblocks] h_j
    uint16_t *e;                                  // [nblocks] h_j | 32768 * (XOR of f over the chunk's blocks up to j): est_j but for the chunk's start bit
    uint8_t *cpar;                                // [nchunks] the XOR of f over a chunk
    uint8_t *cstart;                              // [nchunks] b of the block in front of a chunk
    uint64_t *wsum;                               // [nflag][2] what a workgroup of the flag kernel counted: blocks with f = 1, the sum of the steps
    uint32_t nflag;                               // the workgroups of the flag and est kernels: min(nchunks, the cap)
};
// bbb_nco_rom: travels with the rotate kernel's launch as DdcLaunch's does, so the call has no device state and can be captured
struct CarrierRom {
    alignas(16) int16_t v[1024];
};

// the scratch of a call in uint64 words, and where its arrays lie in it
struct CarrierScratch {
    size_t h, e, cpar, cstart, wsum, words;
};
inline CarrierScratch carrier_scratch(uint64_t nblocks, uint64_t nchunks, uint32_t nflag) {
    CarrierScratch s;
    size_t w = 0;
    auto take = [&](uint64_t bytes) {
        const size_t at = w;
        w += (size_t)((bytes + 7) / 8);
        return at;
    };
    s.h = take(2 * nblocks);
    s.e = take(2 * nblocks);
    s.cpar = take(nchunks);
    s.cstart = take(nchunks);
    s.wsum = take(16 * (uint64_t)nflag);
    s.words = w > 0 ? w : 1;
    return s;
}

// the sum, flag, chain and rotate kernels of one call, in that order on st
int carrier_launch(const CarrierLaunch &a, const CarrierRom &rom, int cus, hipStream_t st);

}  // namespace bbb
