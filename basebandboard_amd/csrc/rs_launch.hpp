// rs_launch.hpp -- what rs_api.hip hands to rs_kernels.hip: the launch structure of bbb_rs_decode and bbb_rs_encode.
#pragma once
#include "bbb_common.hpp"
#include "rs_common.hpp"

namespace bbb {

constexpr uint32_t kRsFramesPerGroup = 4;          // coded frames a workgroup stages at once: 4 * depth codewords for its 4 waves

// The field's tables travel with the launch, as the down-converter's ROM does: the codec has no device state.
struct RsLaunch {
    RsField field;
    RsCode code;
    const uint8_t *in;                            // decode: nframes coded frames; encode: nframes data frames
    uint8_t *out;                                 // decode: nframes data frames; encode: nframes coded frames
    uint8_t *nerr;                                // decode: nframes * depth bytes, or nullptr
    uint64_t *stats;                              // decode: [BBB_RS_NSTATS] added to, or nullptr
    uint64_t nframes;                             // >= 1
};

int rs_decode_launch(const RsLaunch &a, int cus, hipStream_t st);
int rs_encode_launch(const RsLaunch &a, hipStream_t st);

}  // namespace bbb
