// ldpc_launch.hpp -- what ldpc_api.hip hands to ldpc_kernels.hip: the launch structure of bbb_ldpc_decode and bbb_ldpc_encode.
#pragma once
#include "bbb_common.hpp"
#include "ldpc_common.hpp"

namespace bbb {

// The code's edge list travels with the launch, as the Reed-Solomon tables do: the codec has no device state.
struct LdpcLaunch {
    LdpcCode code;
    const void *in;                               // decode: the BASE of the received values; encode: the packed data bits
    uint64_t in_first;                            // decode: element (SOFT16) or bit (HARD) of codeword 0's first value
    uint64_t *out;                                // decode: the packed data bits; encode: the packed coded bits; zeroed by the launch
    uint8_t *iters;                               // decode: a byte per codeword, or nullptr
    uint64_t *stats;                              // decode: [BBB_LDPC_NSTATS] added to, or nullptr
    uint64_t ncodewords;                          // >= 1
    int format;                                   // decode: BBB_CONV_SOFT16 or BBB_CONV_HARD
};
static_assert(sizeof(LdpcLaunch) <= 3584, "the launch structure must stay inside the kernel-argument segment");

int ldpc_decode_launch(const LdpcLaunch &a, int cus, hipStream_t st);
int ldpc_encode_launch(const LdpcLaunch &a, int cus, hipStream_t st);

}  // namespace bbb
