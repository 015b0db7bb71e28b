// flagstat_wide_where_device.h -- internal, device code only: the selection of the `where` kernels over 4-byte and 8-byte
// elements, shared by flagstat_wide_where.hip (one row for the whole array) and flagstat_segments_wide_where.hip (one row per
// segment): the guarded loader of a vector's bitmap bits and the zeroing of the elements that a selection word leaves out.  The
// derivation (which byte, which shift, which two bytes of a funnelled lane) is written out at the top of flagstat_wide_where.hip.
#ifndef FLAGSTAT_WIDE_WHERE_DEVICE_H_
#define FLAGSTAT_WIDE_WHERE_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flagstat_count_core.h"
#include "flagstat_where_device.h"

namespace fsk {

// Bitmap form, edge steps: the selection bits of vector j from bit 0 on; bit q + shift of `sel` belongs to grid position q.
// Positions outside [lo, hi) read as not selected and their bytes are not touched.
template <int W>
__device__ __forceinline__ uint32_t load_bits_wide_guarded(const uint8_t* __restrict__ sel, uint32_t shift, uint64_t j, uint64_t lo, uint64_t hi)
{
    constexpr int EPV = 16 / W;
    const uint64_t f0 = j * EPV;
    uint32_t w = 0;
    if (f0 + EPV <= lo || f0 >= hi) return 0u;
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
        const uint64_t f = f0 + e;
        if (f >= lo && f < hi) {
            const uint64_t b = f + shift;
            w |= ((static_cast<uint32_t>(sel[b >> 3]) >> (b & 7)) & 1u) << e;
        }
    }
    return w;
}

// Zero every dword of the elements of x that the selection word m leaves out (bitmap: the EPV bits from bit sh of m on; bytes:
// the EPV bytes of m); the number selected is added to cnt.
template <int W, int SEL_BITS>
__device__ __forceinline__ void select_elements(uint4& x, uint32_t m, uint32_t sh, uint32_t& cnt)
{
    constexpr int EPV = 16 / W;
    constexpr int ST = SEL_BITS == 1 ? 1 : 8;   // bits between two elements' flags in `bits`
    uint32_t bits;
    if constexpr (SEL_BITS == 1)
        bits = __builtin_amdgcn_ubfe(m, sh, EPV);
    else
        (void)bytes_mask(m, bits);
    cnt += __builtin_popcount(bits);
    auto keep = [&](int e) { return static_cast<uint32_t>(static_cast<int32_t>(bits << (31 - e * ST)) >> 31); };
    if constexpr (W == 4) {
        x.x &= keep(0);
        x.y &= keep(1);
        x.z &= keep(2);
        x.w &= keep(3);
    } else {
        const uint32_t k0 = keep(0), k1 = keep(1);
        x.x &= k0;
        x.y &= k0;
        x.z &= k1;
        x.w &= k1;
    }
}

}  // namespace fsk

#endif
