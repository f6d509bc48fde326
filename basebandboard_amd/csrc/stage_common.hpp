// stage_common.hpp -- the staged count-plane stream of the k = 256 sample kernel: THE definition of its layout,
// for the kernel that writes it (awgn256_planes_kernel), the kernels that read it (unplane_kernel: the byte mover and the shaping
// mover; hist_planes_kernel: the histogram mover), the launch functions that cut it into units and the host scheduler that
// sizes a staging slot (bbb_api.hip, which is also compiled as plain C++ for the scheduler model: device parts behind __HIPCC__).
//
// Layout: u32x4 stage[wave][step][half][lane].  A wave of the sample kernel owns 2048 consecutive generators (generator
// 2048 w + 64 j + l is bit j of lane l of wave w) and runs all L steps of their segments; at every step a lane stores its 8
// count planes as two 16-byte vectors, half 0 = planes 0..3, half 1 = planes 4..7 (plane 7 already complemented: the int8
// two's complement form).  One (step, half) row of a wave is 64 lanes x 16 B = 1 KiB.
//
// A reader's UNIT of work = (source wave w, 8 of its lanes q8 * 8 .. + 8, 128 steps 128 rg .. + 128): 32 KiB of planes, the
// 128 samples of 256 generators.  Units are numbered (w * 8 + q8) * ngroups + rg and a block takes CONSECUTIVE ones (why:
// awgn_kernels.hip, unplane_kernel).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace bbb {

constexpr unsigned kStageLaneBytes = 16;                                  // one lane's half: four planes
constexpr unsigned kStageHalfBytes = 64 * kStageLaneBytes;                // 1 KiB: a (step, half) row of a wave
constexpr unsigned kStageStepBytes = 2 * kStageHalfBytes;                 // 2 KiB per step and wave
constexpr unsigned kStageHalfVecs = kStageHalfBytes / 16, kStageStepVecs = kStageStepBytes / 16;      // the same in u32x4
constexpr unsigned kStageWaveGens = 64 * 32;                              // generators per wave
constexpr unsigned kStageUnitLanes = 8, kStageUnitSteps = 128;
constexpr unsigned kStageUnitBytes = kStageUnitLanes * kStageUnitSteps * 2 * kStageLaneBytes;        // 32 KiB

// 32-bit words of a staging slot: nlanes / 64 waves x L steps
inline size_t stage_words(unsigned nlanes, uint64_t L) { return (size_t)(nlanes / 64) * (size_t)L * (kStageStepBytes / 4); }

struct StageGeom {                   // host computed (stage_geom), a kernel argument of every reader
    unsigned w_lo, ngroups, nunits;  // first source wave of the window; ceil(L / 128); units = waves x 8 x ngroups
    unsigned per_block;              // a block takes the units [per_block * blockIdx.x, + per_block) of the order (w, q8, rg)
};

// The units of the stream window [win_lo, win_lo + n) of a staged kernel (L, nlanes), over at most blocks_wanted blocks: only
// the source waves whose generators touch the window -- generator g owns [g L, (g + 1) L), wave w the generators
// [2048 w, 2048 (w + 1)).  Returns the number of blocks; 0: no unit, or 2^32 and more (out of one launch's reach)
inline unsigned stage_geom(uint64_t win_lo, uint64_t n, unsigned L, unsigned nlanes, uint64_t blocks_wanted, StageGeom *ge) {
    const uint64_t seg = (uint64_t)L * kStageWaveGens;
    const uint64_t w_lo = win_lo / seg;
    const uint64_t w_hi = std::min<uint64_t>((win_lo + n + seg - 1) / seg, nlanes / 64);
    ge->w_lo = (unsigned)w_lo;
    ge->ngroups = (L + kStageUnitSteps - 1) / kStageUnitSteps;
    const uint64_t nunits = w_hi > w_lo ? (w_hi - w_lo) * ge->ngroups * (64 / kStageUnitLanes) : 0;
    if (nunits == 0 || nunits >> 32) return 0;
    ge->nunits = (unsigned)nunits;
    const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>(blocks_wanted, nunits));
    ge->per_block = (unsigned)((nunits + want - 1) / want);
    return (unsigned)((nunits + ge->per_block - 1) / ge->per_block);
}

#ifdef __HIPCC__

typedef uint32_t stage_u32x4 __attribute__((ext_vector_type(4)));

// the writer: lane `lane` of wave `wave` stores half h of step t at stage_row(..)[t * kStageStepVecs + h * kStageHalfVecs]
__device__ __forceinline__ stage_u32x4 *stage_row(stage_u32x4 *stage, unsigned long long wave, unsigned L, unsigned lane) {
    return stage + (wave * L) * kStageStepVecs + lane;
}

// a unit's place; w counts from ge.w_lo
struct StagePos { unsigned q8, rg, w; };

__device__ __forceinline__ void stage_advance(StagePos &p, const StageGeom &ge) {
    if (++p.rg == ge.ngroups) {
        p.rg = 0;
        if (++p.q8 == 64 / kStageUnitLanes) { p.q8 = 0; p.w++; }
    }
}

// the units of block `block`: the number of them, and the place of the first
__device__ __forceinline__ unsigned stage_block_units(const StageGeom &ge, unsigned block, StagePos *first) {
    const unsigned u0 = block * ge.per_block;
    first->rg = u0 % ge.ngroups;
    first->q8 = (u0 / ge.ngroups) & 7;
    first->w = (u0 / ge.ngroups) >> 3;
    return u0 >= ge.nunits ? 0u : (ge.nunits - u0 < ge.per_block ? ge.nunits - u0 : ge.per_block);
}

// where a unit starts in the staging slot: lane q8 * 8 of half 0 of step step0 of source wave wabs
__device__ __forceinline__ const char *stage_unit_src(const void *stage, unsigned long long wabs, unsigned L, unsigned step0, unsigned q8) {
    return reinterpret_cast<const char *>(stage) + ((wabs * L + step0) * kStageStepVecs + q8 * kStageUnitLanes) * 16;
}

// The 8 LDS-DMA instructions of wave wv (of a block's four) for the unit at p -- exactly eight vector-memory instructions, which
// the readers' counted vmcnt waits rely on -- into the 32 KiB raw image at `raw`, laid out for stage_unpack:
// raw[c = 2 s + half][quad-step qs][lane8][16 B] (the DMA's destination is lane-linear, its per-lane SOURCE address is free).
// A lane fetches 16 bytes of one (step, half) row (8 lanes = one full 128-byte line); the 1 KiB block b = wv * 8 + k holds
// c = b >> 2 = 2 wv + (k >> 2) (step-in-quad s = wv, half = k >> 2) of quad-steps (k & 3) * 8 .. + 8
__device__ __forceinline__ void stage_dma_unit(const void *stage, const StageGeom &ge, const StagePos &p, unsigned L, uint32_t *raw, unsigned wv,
                                               unsigned lane) {
    typedef __attribute__((address_space(3))) void *lds_void_ptr;
    const unsigned step0 = p.rg * kStageUnitSteps;
    const char *const sb = stage_unit_src(stage, (unsigned long long)ge.w_lo + p.w, L, step0, p.q8);
    uint32_t *const rawb = raw + wv * 8 * 256;
    if (step0 + kStageUnitSteps <= L) {
        // a lane's 16 bytes of its row; rows 4 steps (8 KiB) apart
        const char *const pl = sb + wv * kStageStepBytes + (lane & 7) * 16 + (lane >> 3) * (4 * kStageStepBytes);
#pragma unroll
        for (unsigned k = 0; k < 8; k++)
            __builtin_amdgcn_global_load_lds((const void *)(pl + ((k & 3) * 32 * kStageStepBytes + (k >> 2) * kStageHalfBytes)),
                                             (lds_void_ptr)(uintptr_t)(rawb + k * 256), 16, 0, 0);
    } else {
        // a segment's last unit may be short: the readers never use the missing steps, the DMA re-reads the last one
        const unsigned last = L - 1 - step0;
#pragma unroll
        for (unsigned k = 0; k < 8; k++) {
            unsigned st = 4 * ((k & 3) * 8 + (lane >> 3)) + wv;
            st = st < last ? st : last;
            __builtin_amdgcn_global_load_lds((const void *)(sb + (size_t)st * kStageStepBytes + (k >> 2) * kStageHalfBytes + (lane & 7) * 16),
                                             (lds_void_ptr)(uintptr_t)(rawb + k * 256), 16, 0, 0);
        }
    }
}

// thread tid of the block's 256 = (quad-step qs = tid >> 3, lane of eight l8 = tid & 7): Z[s][i] = count plane i of step
// 4 qs + s of lane q8 * 8 + l8 (32 generators), 8 x ds_read_b128 (a wave reads 1 KiB contiguous).  COMPLEMENT7: plane 7 as that
// of the unsigned count u = g + 128 instead of the staged int8's
template <bool COMPLEMENT7>
__device__ __forceinline__ void stage_unpack(const uint32_t *raw_image, unsigned tid, uint32_t (&Z)[4][8]) {
    const uint32_t *raw = raw_image + ((tid >> 3) * 8 + (tid & 7)) * 4;
#pragma unroll
    for (unsigned s = 0; s < 4; s++) {
        const stage_u32x4 lo = *reinterpret_cast<const stage_u32x4 *>(raw + (2 * s) * 1024);
        const stage_u32x4 hi = *reinterpret_cast<const stage_u32x4 *>(raw + (2 * s + 1) * 1024);
        Z[s][0] = lo[0]; Z[s][1] = lo[1]; Z[s][2] = lo[2]; Z[s][3] = lo[3];
        Z[s][4] = hi[0]; Z[s][5] = hi[1]; Z[s][6] = hi[2]; Z[s][7] = COMPLEMENT7 ? ~hi[3] : hi[3];
    }
}

#endif  // __HIPCC__

}  // namespace bbb
