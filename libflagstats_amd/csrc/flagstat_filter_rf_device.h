// flagstat_filter_rf_device.h -- internal, device code only: the residue of samtools' view predicate on FLAG, --rf include_any and
// -G exclude_all, as the counting kernels apply it, shared by flagstat_filter_rf.hip (uint16 arrays) and
// flagstat_wide_filter_rf.hip (4-byte and 8-byte elements).  The residue of a launch in byte-replicated form and the test of 4
// flags on their byte planes: pass4 (flagstat_filter_device.h) with up to two more tests ANDed into the pass word.  The
// derivation of the two tests is written out at the top of flagstat_filter_rf.hip.
#ifndef FLAGSTAT_FILTER_RF_DEVICE_H_
#define FLAGSTAT_FILTER_RF_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flagstat_filter_device.h"

namespace fsk {

// the residue of a launch, byte-replicated: wave-uniform
struct FilterRfArgs {
    uint32_t aL, aH;           // include_any, low and high byte plane
    uint32_t gL, gH;           // exclude_all
};

__device__ __forceinline__ FilterRfArgs filter_rf_args_of(uint32_t include_any, uint32_t exclude_all)
{
    FilterRfArgs r;
    r.aL = (include_any & 0xFFu) * 0x01010101u;
    r.aH = ((include_any >> 8) & 0xFFu) * 0x01010101u;
    r.gL = (exclude_all & 0xFFu) * 0x01010101u;
    r.gH = ((exclude_all >> 8) & 0xFFu) * 0x01010101u;
    return r;
}

// v_bitop3_b32 truth tables of the two tests (a = 0xF0, b = 0xCC, c = 0xAA, as in flagstat_filter_device.h)
constexpr uint32_t kTtAndOr = (0xF0 & 0xCC) | 0xAA;                           // (a & b) | c
constexpr uint32_t kTtNotAndOr = ((~0xF0 & 0xCC) | 0xAA) & 0xFF;              // (~a & b) | c

// p with the bytes cleared whose byte of x is 0; p holds nothing but bit 7 of its bytes
__device__ __forceinline__ uint32_t and_nonzero_bytes(uint32_t p, uint32_t x)
{
    const uint32_t s = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return __builtin_amdgcn_bitop3_b32(s, x, p, kTtOrAnd);
}

// pass4 (flagstat_filter_device.h) under the residue: 0x80 per flag of the planes L, H that passes all of it
template <bool MAPQ, bool ANY, bool ALL>
__device__ __forceinline__ uint32_t pass4_rf(const FilterArgs& f, const FilterRfArgs& r, uint32_t L, uint32_t H, uint32_t w)
{
    uint32_t p = pass4<MAPQ>(f, L, H, w);
    if constexpr (ANY) p = and_nonzero_bytes(p, __builtin_amdgcn_bitop3_b32(H, r.aH, L & r.aL, kTtAndOr));
    if constexpr (ALL) p = and_nonzero_bytes(p, __builtin_amdgcn_bitop3_b32(H, r.gH, ~L & r.gL, kTtNotAndOr));
    return p;
}

}  // namespace fsk

#endif
