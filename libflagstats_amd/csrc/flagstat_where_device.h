// flagstat_where_device.h -- internal, device code only: the selection of the `where` kernels as the counting kernels apply it,
// shared by flagstat_where.hip (one row for the whole array) and flagstat_segments_where.hip (one row per segment).  What a lane
// holds of the selection per vector, its loaders (plain and guarded), and the bitmap form's selector table: entry, split and
// lookup.  The derivation is written out at the top of flagstat_where.hip.
#ifndef FLAGSTAT_WHERE_DEVICE_H_
#define FLAGSTAT_WHERE_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flagstat_count_core.h"

namespace fsk {

// what a lane holds of the selection per vector: the byte (two, funnelled) with its 8 bits, or its 8 bytes
template <int SEL_BITS>
struct SelWord {
    typedef uint32_t type;
};
template <>
struct SelWord<8> {
    typedef uint2 type;
};

typedef uint16_t u16_any __attribute__((aligned(1)));
typedef uint32_t u32x2_any __attribute__((ext_vector_type(2), aligned(1)));

// the selection of one vector on a fast step (every position is an element)
template <int SEL_BITS, bool FUNNEL>
__device__ __forceinline__ typename SelWord<SEL_BITS>::type load_sel(const uint8_t* __restrict__ p)
{
    if constexpr (SEL_BITS == 1) {
        if constexpr (FUNNEL)
            return __builtin_nontemporal_load(reinterpret_cast<const u16_any*>(p));
        else
            return __builtin_nontemporal_load(p);
    } else {
        const u32x2_any t = __builtin_nontemporal_load(reinterpret_cast<const u32x2_any*>(p));
        return make_uint2(t.x, t.y);
    }
}

// the selection of vector j on an edge step: positions outside [lo, hi) read as not selected and their bytes are not touched.
// Bitmap form: the 8 bits come back at bit 0 (the step then runs with sh == 0).
template <int SEL_BITS>
__device__ __forceinline__ typename SelWord<SEL_BITS>::type load_sel_guarded(const uint8_t* __restrict__ sel, uint32_t sh, uint64_t j,
                                                                             uint64_t lo, uint64_t hi)
{
    const uint64_t f0 = j * 8;
    if constexpr (SEL_BITS == 1) {
        if (f0 + 8 <= lo || f0 >= hi) return 0u;
        const uint32_t e0 = f0 >= lo ? 0u : static_cast<uint32_t>(lo - f0);            // first and last position that is an element
        const uint32_t e1 = f0 + 8 <= hi ? 7u : static_cast<uint32_t>(hi - 1 - f0);
        uint32_t w = 0;
        if (e0 + sh < 8) w = sel[j];
        if (e1 + sh >= 8) w |= static_cast<uint32_t>(sel[j + 1]) << 8;
        return (w >> sh) & (0xFFu >> (7 - e1)) & (0xFFu << e0);
    } else {
        uint32_t w[2] = {0, 0};
        if (f0 + 8 <= lo || f0 >= hi) return make_uint2(0, 0);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const uint64_t f = f0 + e;
            if (f >= lo && f < hi) w[e >> 2] |= static_cast<uint32_t>(sel[f]) << (8 * (e & 3));
        }
        return make_uint2(w[0], w[1]);
    }
}

// 4 selection bytes to 4 byte masks (any non-zero byte selects); s = 0x01 per selected flag (also flagstat_wide_where.hip's test)
__device__ __forceinline__ uint32_t bytes_mask(uint32_t x, uint32_t& s)
{
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;   // bit 7 of a byte: one of its bits 0-6 is set (no carry leaves a byte)
    s = ((t | x) & 0x80808080u) >> 7;
    return perm(0u, 0x0000FF00u, s);
}

// 4 selection bits (bit k = flag k) to 4 byte masks
__device__ __forceinline__ uint32_t nibble_mask(uint32_t nib)
{
    // bit k lands on bits k, k + 7, k + 14, k + 21, all distinct for k < 4: bit 8 k is bit k
    return perm(0u, 0x0000FF00u, __umul24(nib, 0x204081u) & 0x01010101u);
}

// Bitmap form: the mask costs no VALU op of its own.  split_out's four v_perm_b32 take their byte selectors from registers
// instead of constants, and a selector byte of 0x0C makes v_perm_b32 write 0x00: entry i of a 256-entry table in LDS holds, for
// the selection byte i, the four selectors (low and high byte planes of flags 0-3 and of flags 4-7) in which every flag that is
// not selected has 0x0C.  One ds_read_b128 per vector fetches them.
constexpr uint32_t kSplitLo = 0x06040200u, kSplitHi = 0x07050301u;   // split_out's selectors

__device__ __forceinline__ uint4 selector_entry(uint32_t i)
{
    const uint32_t M0 = nibble_mask(i & 15u), M1 = nibble_mask(i >> 4);
    return make_uint4((kSplitLo & M0) | (0x0C0C0C0Cu & ~M0), (kSplitHi & M0) | (0x0C0C0C0Cu & ~M0), (kSplitLo & M1) | (0x0C0C0C0Cu & ~M1),
                      (kSplitHi & M1) | (0x0C0C0C0Cu & ~M1));
}

// split_out (flagstat_count_core.h) under the selectors of a table entry: the planes of the selected flags, zero elsewhere
__device__ __forceinline__ void split_out_selected(const uint4& o, const uint4& sel, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1)
{
    asm volatile("v_perm_b32 %0, %5, %4, %8\n\tv_perm_b32 %1, %5, %4, %9\n\tv_perm_b32 %2, %7, %6, %10\n\tv_perm_b32 %3, %7, %6, %11"
                 : "=&v"(L0), "=&v"(H0), "=&v"(L1), "=&v"(H1)
                 : "v"(o.x), "v"(o.y), "v"(o.z), "v"(o.w), "v"(sel.x), "v"(sel.y), "v"(sel.z), "v"(sel.w));
}

// the table entry of the vector whose 8 selection bits start at bit sh of w; the number selected is added to cnt
__device__ __forceinline__ uint4 lookup(const uint4* __restrict__ lut, uint32_t w, uint32_t sh, uint32_t& cnt)
{
    const uint32_t bits = __builtin_amdgcn_ubfe(w, sh, 8);
    cnt += __builtin_popcount(bits);
    return lut[bits];
}

}  // namespace fsk

#endif
