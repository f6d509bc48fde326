// ddc_common.hpp -- the per-sample arithmetic of the digital down-converter (include/bbb.h, bbb_ddc_*), for the device and
// for the host: bbb_ddc_polar_host and tests/ddc_host.cpp run the same code on the CPU.
//
//   j(n)  = (first_sample + n) mod 2^24      pa(n) = (pa0 + j(n) * fcw) mod 2^24      adr(n) = pa(n) >> 14
//   c(n)  = rom[(adr(n) + 256) mod 1024]     s(n)  = rom[adr(n)]
//   mi(n) = (x(n) * c(n)) >> 15              mq(n) = (x(n) * -s(n)) >> 15
// |rom| <= 32767 and x >= -32768, so both products lie within 32768 * 32767 and mi, mq within [-32767, 32767].
// The polar form of an (I, Q) pair is a 16-step CORDIC on the pair scaled by 2^14 (ddc_polar below).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DDC_HD __host__ __device__ __forceinline__
#else
#define DDC_HD inline
#endif

namespace bbb {

constexpr uint32_t kDdcMask24 = 0xFFFFFFu;

// adr of the sample whose absolute number is j (only its low 24 bits count; uint32 arithmetic is exact modulo 2^24)
DDC_HD uint32_t ddc_adr(uint32_t pa0, uint32_t fcw, uint32_t j) { return ((pa0 + j * fcw) & kDdcMask24) >> 14; }

// (mi, mq) of one sample from the ROM entries c = rom[(adr + 256) mod 1024], s = rom[adr]
DDC_HD void ddc_mix(int x, int c, int s, int &mi, int &mq) {
    mi = (x * c) >> 15;
    mq = (x * -s) >> 15;
}

// round(atan(2^-k) / (2 pi) * 2^32)
DDC_HD uint32_t ddc_cordic_angle(int k) {
    constexpr uint32_t A[16] = {536870912u, 316933406u, 167458907u, 85004756u, 42667331u, 21354465u, 10679838u, 5340245u,
                                2670163u,   1335087u,   667544u,    333772u,   166886u,   83443u,    41722u,    20861u};
    return A[k];
}

constexpr int kDdcCordicSteps = 16;
constexpr int kDdcCordicGain = 39797;          // round(2^16 / prod sqrt(1 + 4^-k)): mag = X * gain >> 30 undoes the 2^14 and the gain

// The CORDIC on accumulators of type T: int32_t is the definition (|X|, |Y| stay below 2^31: tests/ddc_host.cpp walks the
// pairs with T = int64_t beside it).  (0, 0) gives (0, 0).  *xmax, when given, receives max(|X|, |Y|) over the steps.
template <typename T>
DDC_HD void ddc_polar_t(int i, int q, uint32_t &mag, int &phase, T *xmax = nullptr) {
    if (i == 0 && q == 0) {
        mag = 0;
        phase = 0;
        if (xmax) *xmax = 0;
        return;
    }
    const bool neg = i < 0;
    T X = (T)(neg ? -i : i) * 16384, Y = (T)(neg ? -q : q) * 16384, top = X > (Y < 0 ? -Y : Y) ? X : (Y < 0 ? -Y : Y);
    uint32_t Z = neg ? 0x80000000u : 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < kDdcCordicSteps; ++k) {
        const bool d = Y >= 0;
        const T xs = X >> k, ys = Y >> k;
        X = d ? X + ys : X - ys;
        Y = d ? Y - xs : Y + xs;
        Z = d ? Z + ddc_cordic_angle(k) : Z - ddc_cordic_angle(k);
        const T ay = Y < 0 ? -Y : Y, ax = X < 0 ? -X : X;
        top = ax > top ? ax : top;
        top = ay > top ? ay : top;
    }
    mag = (uint32_t)(((long long)X * kDdcCordicGain + (1ll << 29)) >> 30);
    phase = (int)(int16_t)(uint16_t)((Z + 0x8000u) >> 16);
    if (xmax) *xmax = top;
}

// (mag: uint16, phase: int16 in 1/65536 turn) of an int16 pair
DDC_HD void ddc_polar(int i, int q, uint32_t &mag, int &phase) { ddc_polar_t<int32_t>(i, q, mag, phase); }

}  // namespace bbb
