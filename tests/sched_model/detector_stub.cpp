// The COARSE stand-in for basebandboard_amd/csrc/detector_api.hip, for the drivers that link bbb_api.hip and model.cpp and are
// not about the detector: one operation for everything the call queues, then its synchronisation.  (detector_driver.cpp
// links the real scheduler instead and stubs the launchers of detector_launch.hpp.)
#include "model.hpp"

#include "../../basebandboard_amd/csrc/bbb_common.hpp"

using namespace model;

namespace bbb {

int prbs_detector_stream_launch(int, const uint64_t *src, uint64_t, uint64_t *err, uint64_t *reload, bbb_detector_stats *stats, uint64_t, uint64_t,
                                hipStream_t st) {
    if (refused()) return BBB_EHIP;
    op(st, "detector stream (chunk pass ... read-back)", {src}, {err, reload});
    if (stats) *stats = bbb_detector_stats{};
    hipStreamSynchronize(st);
    return BBB_OK;
}

}  // namespace bbb
