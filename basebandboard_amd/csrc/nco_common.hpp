// nco_common.hpp -- the oscillator's ROM in LDS, shared by the NCO (nco_kernels.hip) and the down-converter's local
// oscillator (ddc_kernels.hip).
//
// kNcoReps replicas of the 1024 int16 entries, replica r at dword r * 513.  Lane l reads replica l % 16, so that lanes whose
// entries fall on one bank of one replica land on different banks: bank = (r + entry / 2) mod 32.  Without replicas, the
// lanes of a ds_read group (32 lanes), each owning 8 consecutive samples, address entries 8 * inc / 2^14 apart, all on one
// bank at fcw = 2^16 .. 2^17 (16-way); with them no fcw costs more than 2 cycles per group.
#pragma once

#include "bbb_common.hpp"

namespace bbb {

constexpr int kNcoRepWords = 513;
constexpr int kNcoLdsWords = kNcoReps * kNcoRepWords;

// copies the ROM (1024 entries anywhere a thread can read: global memory or the kernel's arguments) into the replicas,
// waits for the workgroup, and returns this thread's replica
__device__ inline const int16_t *nco_rom_to_lds(const int16_t *rom, uint32_t *lds) {
    const uint32_t *r32 = reinterpret_cast<const uint32_t *>(rom);
    for (int i = threadIdx.x; i < kNcoReps * 512; i += blockDim.x) lds[(i >> 9) * kNcoRepWords + (i & 511)] = r32[i & 511];
    __syncthreads();
    return reinterpret_cast<const int16_t *>(lds + (threadIdx.x % kNcoReps) * kNcoRepWords);
}

}  // namespace bbb
