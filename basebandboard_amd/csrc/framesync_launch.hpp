// framesync_launch.hpp -- what framesync_api.hip hands to framesync_kernels.hip: the launch structure of bbb_framesync_run,
// bbb_frame_extract and bbb_frame_attach.
#pragma once
#include "bbb_common.hpp"
#include "framesync_common.hpp"

namespace bbb {

// the scratch of a run over nbits: the tile flags (a bit per tile of the search pass), then the candidate plane (a bit per position)
FS_HD uint64_t fs_words(uint64_t nbits) { return (nbits + 63) / 64; }
FS_HD uint64_t fs_tiles(uint64_t nbits) { return (fs_words(nbits) + kFsTileWords - 1) / kFsTileWords; }
FS_HD uint64_t fs_flag_words(uint64_t nbits) { return (fs_tiles(nbits) + 63) / 64; }

// The randomiser's table travels with the launch, as the Reed-Solomon tables do: no device state but the caller's.
struct FsLaunch {
    FsCfg c;
    FsRand rnd;
    const uint64_t *in;                            // the data: fs_words(nbits) words
    uint64_t nbits, first_bit;
    int final;
    uint64_t *state;
    uint64_t *pos;
    uint16_t *meta;
    uint64_t max_frames;
    uint64_t *flags, *plane;                       // run: the scratch
    const uint8_t *payload;                        // attach
    uint8_t *out_bytes;                            // extract
    uint64_t *out_words;                           // attach
    uint64_t nframes;                              // attach
};

int fs_run_launch(const FsLaunch &a, int cus, hipStream_t st);
int fs_extract_launch(const FsLaunch &a, int cus, hipStream_t st);
int fs_attach_launch(const FsLaunch &a, int cus, hipStream_t st);

}  // namespace bbb
