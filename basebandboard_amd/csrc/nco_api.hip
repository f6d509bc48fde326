// nco_api.hip -- the extern "C" entry points of the numerically controlled oscillator (include/bbb.h, bbb_nco_*).  Host logic
// only: argument checks, the ROM, the object's device state (two slots, alternated by the launches) and the chunk loop.
#include "capture.hpp"

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>

using namespace bbb;

namespace {

constexpr uint64_t kChunkConst = 1ull << 30;   // samples per launch with constant fm (launch indices stay below 2^31)
constexpr uint64_t kChunkFm = 1ull << 24;      // with an fm buffer: 64 MiB of fm, re-read by the third pass from the Infinity Cache

int cfg_check(const bbb_nco_cfg *c) {
    if (!c) return fail(BBB_EINVAL, "null cfg");
    if (c->fcw >= (1u << 24)) return fail(BBB_EINVAL, "fcw must be < 2^24 (got " + std::to_string(c->fcw) + ")");
    if (c->am >= (1u << 16)) return fail(BBB_EINVAL, "am must be < 2^16 (got " + std::to_string(c->am) + ")");
    if (c->fm < -(1 << 23) || c->fm >= (1 << 23)) return fail(BBB_EINVAL, "fm must be in [-2^23, 2^23) (got " + std::to_string(c->fm) + ")");
    if (c->pm < -512 || c->pm >= 512) return fail(BBB_EINVAL, "pm must be in [-512, 512) (got " + std::to_string(c->pm) + ")");
    return BBB_OK;
}

int state_check(const bbb_nco_state *s) {
    if (!s) return fail(BBB_EINVAL, "null state");
    if (s->pa >= (1u << 24)) return fail(BBB_EINVAL, "pa must be < 2^24");
    if (s->q < -32768 || s->q > 32767 || s->w < -32768 || s->w > 32767) return fail(BBB_EINVAL, "q and w must be int16 values");
    return BBB_OK;
}

}  // namespace

struct bbb_nco {
    bbb_nco_cfg cfg{};
    int grid = 0;
    int cur = 0;                     // the slot of state holding the registers after the last queued launch
    DevBuf<uint32_t> tiles;          // the fm scan's tile sums / offsets of one chunk
    DevBuf<bbb_nco_state> state;     // 2 slots
    DevBuf<int16_t> rom;             // 1024 entries
    StreamObj on;                    // last: selects the device for the frees (rom, state, tiles)
};

extern "C" {

int bbb_nco_rom(int16_t rom[1024]) {
    if (!rom) return fail(BBB_EINVAL, "null rom");
    // np.linspace(0, 2 pi, 1024): t_i = i * (2 pi / 1023), the last point exactly 2 pi; np.round is half-to-even, as
    // nearbyint in the default rounding mode.  No entry lies within 0.001 of a half-integer, so the libm sin rounds alike.
    const double step = 2.0 * M_PI / 1023.0;
    for (int i = 0; i < 1024; ++i) {
        const double t = i == 1023 ? 2.0 * M_PI : i * step;
        rom[i] = (int16_t)std::nearbyint(std::sin(t) * 32767.0);
    }
    return BBB_OK;
}

int bbb_nco_open(const bbb_nco_cfg *cfg, int device, void *hip_stream, bbb_nco **out) {
    if (!out) return fail(BBB_EINVAL, "null out");
    int rc = cfg_check(cfg);
    if (rc) return rc;
    if ((rc = use_device(device))) return rc;
    auto o = std::make_unique<bbb_nco>();
    o->on.device = device;
    o->on.st = (hipStream_t)hip_stream;
    o->cfg = *cfg;
    int cus = 0;
    if ((rc = device_cus(device, &cus))) return rc;
    o->grid = std::max(1, cus) * 4;        // 4 workgroups of 512 threads fit a CU beside the 32 KiB of ROM replicas each
    int16_t rom[1024];
    bbb_nco_rom(rom);
    if ((rc = o->rom.grow(1024)) || (rc = o->state.grow(2)) || (rc = o->tiles.grow(nco_tiles(kChunkFm)))) return rc;
    BBB_HIP(hipMemcpyAsync(o->rom, rom, sizeof rom, hipMemcpyHostToDevice, o->on.st));
    BBB_HIP(hipMemsetAsync(o->state, 0, 2 * sizeof(bbb_nco_state), o->on.st));
    BBB_HIP(hipStreamSynchronize(o->on.st));  // `rom` is a host stack array
    *out = o.release();
    return BBB_OK;
}

int bbb_nco_set_cfg(bbb_nco *o, const bbb_nco_cfg *cfg) {
    if (!o) return fail(BBB_EINVAL, "null nco object");
    int rc = cfg_check(cfg);
    if (rc) return rc;
    o->cfg = *cfg;                         // launches take the constants by value: queued runs keep theirs
    return BBB_OK;
}

int bbb_nco_set_stream(bbb_nco *o, void *hip_stream) {
    if (!o) return fail(BBB_EINVAL, "null nco object");
    return o->on.rebind((hipStream_t)hip_stream);
}

int bbb_nco_run(bbb_nco *o, const int32_t *fm_dev, const uint16_t *am_dev, const int16_t *pm_dev, uint64_t nsamples,
                int16_t *x_dev) {
    if (!o) return fail(BBB_EINVAL, "null nco object");
    if (nsamples == 0) return BBB_OK;
    if (!x_dev) return fail(BBB_EINVAL, "null x_dev");
    if (((uintptr_t)x_dev & 1) || ((uintptr_t)fm_dev & 3) || ((uintptr_t)am_dev & 1) || ((uintptr_t)pm_dev & 1))
        return fail(BBB_EINVAL, "misaligned device pointer");
    BBB_HIP(hipSetDevice(o->on.device));
    NcoLaunch a{};
    a.fcw = o->cfg.fcw;
    a.am_c = o->cfg.am;
    a.fm_c = o->cfg.fm;
    a.pm_c = o->cfg.pm;
    a.vec = !(((uintptr_t)x_dev | (uintptr_t)fm_dev | (uintptr_t)am_dev | (uintptr_t)pm_dev) & 15);
    a.rom = o->rom;
    a.tiles = o->tiles;
    const uint64_t chunk = fm_dev ? kChunkFm : kChunkConst;     // multiples of 8: a chunk keeps the buffers' alignment
    for (uint64_t off = 0; off < nsamples; off += chunk) {
        a.n = std::min(chunk, nsamples - off);
        a.fm = fm_dev ? fm_dev + off : nullptr;
        a.am = am_dev ? am_dev + off : nullptr;
        a.pm = pm_dev ? pm_dev + off : nullptr;
        a.x = x_dev + off;
        a.in = o->state + o->cur;
        a.out = o->state + (o->cur ^ 1);
        int rc = nco_launch(a, o->grid, o->on.st);
        if (rc) return rc;
        o->cur ^= 1;
    }
    return BBB_OK;
}

int bbb_nco_get_state(bbb_nco *o, bbb_nco_state *st) {
    if (!o) return fail(BBB_EINVAL, "null nco object");
    if (!st) return fail(BBB_EINVAL, "null state");
    BBB_HIP(hipSetDevice(o->on.device));
    bbb_nco_state s;
    BBB_HIP(hipMemcpyAsync(&s, o->state + o->cur, sizeof s, hipMemcpyDeviceToHost, o->on.st));
    BBB_HIP(hipStreamSynchronize(o->on.st));
    *st = s;
    return BBB_OK;
}

int bbb_nco_set_state(bbb_nco *o, const bbb_nco_state *st) {
    if (!o) return fail(BBB_EINVAL, "null nco object");
    int rc = state_check(st);
    if (rc) return rc;
    BBB_HIP(hipSetDevice(o->on.device));
    return nco_put_state(*st, o->state + o->cur, o->on.st);
}

int bbb_nco_close(bbb_nco *o) {
    if (!o) return fail(BBB_EINVAL, "null nco object");
    o->on.drain();
    delete o;
    return BBB_OK;
}

}  // extern "C"
