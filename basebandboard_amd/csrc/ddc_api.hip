// ddc_api.hip -- the extern "C" entry points of the digital down-converter (include/bbb.h, bbb_ddc_*).  Host logic only: the
// argument checks, the launch structure (taps packed by fir_api.hip's rule, the oscillator's ROM) and the host CORDIC.
#include "capture.hpp"
#include "ddc_common.hpp"

#include <algorithm>
#include <string>

using namespace bbb;

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
    if (first_sample > kFirSampleLimit || nin > kFirSampleLimit - first_sample) return fail(BBB_EINVAL, "first_sample + nin must be <= 2^58");
    if (nin && !in_dev) return fail(BBB_EINVAL, "null in_dev");
    const uint64_t nout = fir_nout(fir, nin);
    if (nout && !out_dev) return fail(BBB_EINVAL, "null out_dev");
    const unsigned pair = ddc->mode == BBB_DDC_IQ32 ? 8 : 4;           // bytes of one output element
    if (((uintptr_t)in_dev & 1) || ((uintptr_t)out_dev & (pair - 1))) return fail(BBB_EINVAL, "misaligned device pointer");
    uint32_t before;
    if ((rc = fir_history(in_dev, nin, nbefore, fir->ntaps, out_dev, nout * pair, "out_dev", &before))) return rc;
    if (nout_out) *nout_out = nout;
    if (nout == 0) return BBB_OK;
    int cus = 0;
    if ((rc = use_device(device)) || (rc = device_cus(device, &cus))) return rc;
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
