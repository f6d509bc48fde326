// ddc_api.hip -- the extern "C" entry points of the digital down-converter (include/bbb.h, bbb_ddc_*).  Host logic only: the
// argument checks, the launch structure (taps packed by fir_api.hip's rule, the oscillator's ROM) and the host CORDIC.
#include "bbb_common.hpp"
#include "ddc_common.hpp"

#include <algorithm>
#include <string>

using namespace bbb;

namespace {

constexpr uint64_t kDdcSampleLimit = 1ull << 58;

bool overlap(const void *a, uint64_t abytes, const void *b, uint64_t bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bbytes && b0 < a0 + abytes;
}

}  // namespace

extern "C" {

int bbb_ddc_polar_host(int16_t i, int16_t q, uint16_t *mag, int16_t *phase) {
    if (!mag || !phase) return fail(BBB_EINVAL, "null mag or phase");
    uint32_t m;
    int p;
    ddc_polar(i, q, m, p);
    *mag = (uint16_t)m;
    *phase = (int16_t)p;
    return BBB_OK;
}

int bbb_ddc_run(const int16_t *in_dev, uint64_t nin, uint32_t nbefore, uint64_t first_sample, const bbb_ddc_cfg *ddc,
                const bbb_fir_cfg *fir, void *out_dev, uint64_t *nout_out, int device, void *hip_stream) {
    if (!ddc) return fail(BBB_EINVAL, "null ddc cfg");
    if (ddc->fcw >= (1u << 24)) return fail(BBB_EINVAL, "fcw must be < 2^24 (got " + std::to_string(ddc->fcw) + ")");
    if (ddc->pa0 >= (1u << 24)) return fail(BBB_EINVAL, "pa0 must be < 2^24 (got " + std::to_string(ddc->pa0) + ")");
    if (ddc->mode > BBB_DDC_POLAR) return fail(BBB_EINVAL, "mode must be BBB_DDC_IQ16, IQ32 or POLAR (got " + std::to_string(ddc->mode) + ")");
    int rc = fir_cfg_check(fir, true);                  // out_bytes is not looked at; the shift is, here
    if (rc) return rc;
    if (fir->shift > 31) return fail(BBB_EINVAL, "shift must be 0..31 (got " + std::to_string(fir->shift) + ")");
    if (first_sample > kDdcSampleLimit || nin > kDdcSampleLimit - first_sample) return fail(BBB_EINVAL, "first_sample + nin must be <= 2^58");
    if (nin && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    const uint64_t nout = fir->phase < nin ? (nin - fir->phase + fir->decim - 1) / fir->decim : 0;
    if (nout && !out_dev) return fail(BBB_EINVAL, "null out_dev");
    const unsigned pair = ddc->mode == BBB_DDC_IQ32 ? 8 : 4;           // bytes of one output element
    if (((uintptr_t)in_dev & 1) || ((uintptr_t)out_dev & (pair - 1))) return fail(BBB_EINVAL, "misaligned device pointer");
    const uint32_t before = std::min<uint32_t>(nbefore, fir->ntaps - 1);
    if (nout && overlap(in_dev - before, (nin + before) * 2, out_dev, nout * pair)) return fail(BBB_EINVAL, "out_dev overlaps the samples");
    if (nout_out) *nout_out = nout;
    if (nout == 0) return BBB_OK;
    if ((rc = use_device(device))) return rc;
    int cus = 0;
    BBB_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    DdcLaunch a{};
    a.in = in_dev;
    a.out = out_dev;
    a.nin = nin;
    a.nout = nout;
    a.nbefore = before;
    a.ngroups = fir_pack_taps(fir, a.taps);
    a.shift = fir->shift;
    a.decim = fir->decim;
    a.phase = fir->phase;
    a.first = (uint32_t)first_sample;
    a.fcw = ddc->fcw;
    a.pa0 = ddc->pa0;
    a.in_vec = !((uintptr_t)in_dev & 15);
    a.out_vec = !((uintptr_t)out_dev & 15);
    bbb_nco_rom(a.rom);
    return ddc_launch(a, (int)ddc->mode, cus, (hipStream_t)hip_stream);
}

}  // extern "C"
