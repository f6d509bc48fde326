// mlse_launch.hpp -- what mlse_api.hip hands to mlse_kernels.hip: the launch structure of one bbb_mlse_run.
#pragma once
#include "bbb_common.hpp"
#include "mlse_common.hpp"

namespace bbb {

// mlse_kernels.hip: the Viterbi sequence detector (include/bbb.h, bbb_mlse_run)
struct MlseLaunch {                               // one call: in .. in_vec, taps as FirLaunch
    const int16_t *in;
    uint64_t nin;
    uint32_t nbefore;                             // history the kernel may read: clamped to what the first window reaches
    uint32_t ngroups, shift, decim, phase;
    int in_vec;
    uint32_t mem;                                 // 1..4
    int32_t g[kMlseMaxMem + 1];                   // 0 from mem + 1 on
    uint32_t init_state;                          // masked to mem bits
    MlseGeom geom;
    uint64_t first, nsym, ndecided;               // the call's symbols [first, first + nsym), of which ndecided >= 1 are emitted
    uint64_t j0, nblocks;                         // the blocks that hold the emitted symbols: j0 .. j0 + nblocks - 1
    uint64_t *bits;                               // ceil(ndecided / 64) zeroed words
    uint64_t *stats;                              // [2] added to, or nullptr
    uint32_t taps[BBB_FIR_MAX_TAPS / 2];
};

// the one kernel of a call on st
int mlse_launch(const MlseLaunch &a, int cus, hipStream_t st);

}  // namespace bbb
