// flagstat_segments_wide_device.h -- internal, device code only: the per-piece count both segmented kernels over 4-byte and 8-byte
// elements run outside their chain regime (flagstat_segments_wide.hip, flagstat_segments_wide_filter.hip).
#ifndef FLAGSTAT_SEGMENTS_WIDE_DEVICE_H_
#define FLAGSTAT_SEGMENTS_WIDE_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flagstat_count_core.h"
#include "flagstat_segments_shared.h"
#include "flagstat_wide_device.h"

namespace fsk {

// The piece [b, e) of the unit starting at grid position w0 (its 8 rows in v[]) into the lane counters and the lane's mask
// accumulators; only dwords of elements inside the piece reach either (mask_vec_wide).  A count_planes call takes the byte planes
// of 8 elements of the lane, group g of the unit:
//   W = 4: rows 2 g and 2 g + 1; (L0, H0) are the 4 elements of the lane's vector in row 2 g, (L1, H1) those in row 2 g + 1
//   W = 8: rows 4 g .. 4 g + 3;  (L0, H0) are the 2 elements of row 4 g, then the 2 of row 4 g + 1; (L1, H1) rows 4 g + 2, 4 g + 3
// and `planes(g, L0, H0, L1, H1)` may change them in front of the count (the filter zeroes the flags that fail).  Rows outside
// the piece are not read out: their bytes of the planes are 0.
template <int W, typename Planes>
__device__ __forceinline__ void count_piece_wide_with(uint32_t (&acc)[kInternal], uint32_t& or_even, uint32_t& or_odd,
                                                      const uint4 (&v)[kUnroll], uint64_t w0, uint64_t b, uint64_t e, uint32_t lane,
                                                      Planes&& planes)
{
    constexpr int RPG = W / 2;                     // rows per count_planes call (8 flags): 2 at W = 4, 4 at W = 8
    constexpr uint64_t RE = 1024 / W;              // elements per row
    constexpr uint32_t EPV = 16 / W;
    constexpr uint32_t sel = 0x05010400u;          // narrow_out's: two flag-carrying dwords a, b -> P = [a.b0, b.b0, a.b1, b.b1]
#pragma unroll
    for (int g = 0; g < kUnroll / RPG; ++g) {
        const uint64_t g0 = w0 + static_cast<uint64_t>(g) * (RPG * RE);
        if (g0 + RPG * RE <= b || g0 >= e) continue;  // wave-uniform
        uint32_t P[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < RPG; ++i) {
            const uint64_t r0 = g0 + static_cast<uint64_t>(i) * RE;
            if (r0 + RE <= b || r0 >= e) continue;  // wave-uniform: a row outside the piece counts as zeros
            uint4 x = v[g * RPG + i];
            if (r0 < b || r0 + RE > e) x = mask_vec_wide<W>(x, r0 + EPV * lane, b, e);
            if constexpr (W == 4) {
                or_even |= x.x | x.y | x.z | x.w;
                P[2 * i] = perm(x.y, x.x, sel);
                P[2 * i + 1] = perm(x.w, x.z, sel);
            } else {
                or_even |= x.x | x.z;
                or_odd |= x.y | x.w;
                P[i] = perm(x.z, x.x, sel);
            }
        }
        uint32_t L0 = perm(P[1], P[0], 0x05040100u), H0 = perm(P[1], P[0], 0x07060302u);
        uint32_t L1 = perm(P[3], P[2], 0x05040100u), H1 = perm(P[3], P[2], 0x07060302u);
        planes(g, L0, H0, L1, H1);
        count_planes(acc, L0, H0, L1, H1);
    }
}

}  // namespace fsk

#endif
