// dfe_launch.hpp -- what dfe_api.hip hands to dfe_kernels.hip: the launch structure of one bbb_dfe_run.
#pragma once
#include "bbb_common.hpp"
#include "dfe_common.hpp"

namespace bbb {

// dfe_kernels.hip: the decision-feedback equalizer (include/bbb.h, bbb_dfe_run)
struct DfeLaunch {                                // one call: in .. in_vec, taps as FirLaunch
    const int16_t *in;
    uint64_t nin, nsym;
    uint32_t nbefore, ngroups, shift, decim, phase;
    int in_vec;
    uint32_t nfb;
    DfeRule rule;
    uint32_t region, warmup;                      // symbols of a region and of its warm-up, both >= 1
    uint64_t nreg;                                // ceil(nsym / region) <= kDfeMaxRegions
    uint32_t *state;                              // the call's state word, read by the region and chain kernels, written by the chain
    uint64_t *bits;                               // ceil(nsym / 64) zeroed words
    void *soft;                                   // nsym int16 (soft_bytes 2) or int32 (4), or nullptr
    uint32_t soft_bytes;
    uint64_t *rec;                                // [nreg][2]: a region's map and dfe_info
    uint64_t *flagged;                            // [nreg] dfe_flag entries; flagged[nreg] is their count
    uint64_t *stats;                              // [4] added to, or nullptr
    uint32_t taps[BBB_FIR_MAX_TAPS / 2];
};
inline size_t dfe_scratch_words(uint64_t nreg) { return (size_t)(3 * nreg + 1); }
// the region, chain and repair kernels of one call, in that order on st
int dfe_launch(const DfeLaunch &a, int cus, hipStream_t st);

}  // namespace bbb
