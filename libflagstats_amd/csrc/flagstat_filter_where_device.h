// flagstat_filter_where_device.h -- internal, device code only: how a selection joins the filter's pass word in registers, shared by
// flagstat_filter_where.hip (one row for the whole array) and flagstat_segments_filter_where.hip (one row per segment).  pass4
// (flagstat_filter_device.h) leaves 0x80 per passing flag of 4; these two clear it where the flag is not selected.  The derivation
// and the instruction counts are written out at the top of flagstat_filter_where.hip.
#ifndef FLAGSTAT_FILTER_WHERE_DEVICE_H_
#define FLAGSTAT_FILTER_WHERE_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flagstat_filter_device.h"

namespace fsk {

// 0x80 per flag of 4 that passes (p: 0x80 per passing flag, nothing else) and whose selection bit is set; b: the 4 bits.  The
// compiler folds the shift into the multiplier (one v_mul_lo_u32 by 0x10204080).  Shifting p instead, which keeps the multiply a
// v_mul_u32_u24, measured 1.6-2.0 % slower without MAPQ and the same with it (profiles/r20/filter_where_ab.log)
__device__ __forceinline__ uint32_t counted_bits(uint32_t p, uint32_t b)
{
    return p & (__umul24(b, 0x204081u) << 7);
}

// 0x80 per flag of 4 that passes and whose selection byte in x is not zero
__device__ __forceinline__ uint32_t counted_bytes(uint32_t p, uint32_t x)
{
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;   // no carry leaves a byte
    return __builtin_amdgcn_bitop3_b32(t, x, p, kTtOrAnd);
}

}  // namespace fsk

#endif
