// flagstat_filter_device.h -- internal, device code only: samtools' view filter as the counting kernels apply it, shared by
// flagstat_filter.hip (one row for the whole array) and flagstat_segments_filter.hip (one row per segment).  The predicate of a
// launch in byte-replicated form, the test of 4 flags on their byte planes, the MAPQ loaders and the bits that say which
// positions of a vector are elements.  The derivation of the test is written out at the top of flagstat_filter.hip.
#ifndef FLAGSTAT_FILTER_DEVICE_H_
#define FLAGSTAT_FILTER_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsk {

typedef uint32_t mq_u32x2_any __attribute__((ext_vector_type(2), aligned(1)));

// the predicate of a launch, byte-replicated: wave-uniform
struct FilterArgs {
    uint32_t rL, mL, rH, mH;   // require and require | exclude, low and high byte plane
    uint32_t y7;               // (min_mapq & 0x7F) in every byte
    uint32_t k;                // 0x80808080 when min_mapq < 128, else 0
};

// require & exclude == 0, both below 2^16, min_mapq below 256
__device__ __forceinline__ FilterArgs filter_args_of(uint32_t require, uint32_t exclude, uint32_t min_mapq)
{
    FilterArgs f;
    const uint32_t m = require | exclude;
    f.rL = (require & 0xFFu) * 0x01010101u;
    f.rH = ((require >> 8) & 0xFFu) * 0x01010101u;
    f.mL = (m & 0xFFu) * 0x01010101u;
    f.mH = ((m >> 8) & 0xFFu) * 0x01010101u;
    f.y7 = (min_mapq & 0x7Fu) * 0x01010101u;
    f.k = min_mapq < 128u ? 0x80808080u : 0u;
    return f;
}

// the MAPQ bytes of one vector all of whose positions are elements
__device__ __forceinline__ uint2 load_mapq(const uint8_t* __restrict__ p)
{
    const mq_u32x2_any t = __builtin_nontemporal_load(reinterpret_cast<const mq_u32x2_any*>(p));
    return make_uint2(t.x, t.y);
}

// the MAPQ bytes of vector j at an edge: bytes of positions outside [lo, hi) are not touched and read as 0
__device__ __forceinline__ uint2 load_mapq_guarded(const uint8_t* __restrict__ mq, uint64_t j, uint64_t lo, uint64_t hi)
{
    const uint64_t f0 = j * 8;
    uint32_t w[2] = {0, 0};
    if (f0 + 8 <= lo || f0 >= hi) return make_uint2(0, 0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint64_t f = f0 + e;
        if (f >= lo && f < hi) w[e >> 2] |= static_cast<uint32_t>(mq[f]) << (8 * (e & 3));
    }
    return make_uint2(w[0], w[1]);
}

// bit e of the result: position 8 j + e lies in [lo, hi)
__device__ __forceinline__ uint32_t valid_bits(uint64_t j, uint64_t lo, uint64_t hi)
{
    const uint64_t f0 = j * 8;
    if (f0 + 8 <= lo || f0 >= hi) return 0u;
    const uint32_t e0 = f0 >= lo ? 0u : static_cast<uint32_t>(lo - f0);
    const uint32_t e1 = f0 + 8 <= hi ? 7u : static_cast<uint32_t>(hi - 1 - f0);
    return (0xFFu >> (7 - e1)) & (0xFFu << e0);
}

// 4 bits (bit k = flag k) to 0x80 per set bit: bit k lands on bits k, k + 7, k + 14, k + 21, all distinct for k < 4
__device__ __forceinline__ uint32_t nibble_to_bit7(uint32_t nib)
{
    return (__umul24(nib, 0x204081u) & 0x01010101u) << 7;
}

// v_bitop3_b32 truth tables, written as the expression over a = 0xF0, b = 0xCC, c = 0xAA
constexpr uint32_t kTtXorAnd = (0xF0 ^ 0xCC) & 0xAA;                          // (a ^ b) & c
constexpr uint32_t kTtOrAnd = (0xF0 | 0xCC) & 0xAA;                           // (a | b) & c
constexpr uint32_t kTtOr3 = 0xF0 | 0xCC | 0xAA;                               // a | b | c
constexpr uint32_t kTtNotAnd = (~0xF0 & 0xCC) & 0xFF;                         // ~a & b
constexpr uint32_t kTtNotAndAnd = (~0xF0 & 0xCC & 0xAA) & 0xFF;               // ~a & b & c
constexpr uint32_t kTtMajority = (0xF0 & 0xCC) | ((0xF0 | 0xCC) & 0xAA);      // (a & b) | ((a | b) & c)

// 0x80 per flag of the planes L, H that passes; w: the MAPQ bytes of the same 4 flags
template <bool MAPQ>
__device__ __forceinline__ uint32_t pass4(const FilterArgs& f, uint32_t L, uint32_t H, uint32_t w)
{
    const uint32_t x1 = __builtin_amdgcn_bitop3_b32(L, f.rL, f.mL, kTtXorAnd);
    const uint32_t x2 = __builtin_amdgcn_bitop3_b32(H, f.rH, f.mH, kTtXorAnd);
    const uint32_t t = __builtin_amdgcn_bitop3_b32(x1, x2, 0x7F7F7F7Fu, kTtOrAnd) + 0x7F7F7F7Fu;
    const uint32_t q = __builtin_amdgcn_bitop3_b32(t, x1, x2, kTtOr3);
    if constexpr (MAPQ) {
        const uint32_t t2 = (w | 0x80808080u) - f.y7;
        const uint32_t g = __builtin_amdgcn_bitop3_b32(w, t2, f.k, kTtMajority);
        return __builtin_amdgcn_bitop3_b32(q, g, 0x80808080u, kTtNotAndAnd);
    } else {
        return __builtin_amdgcn_bitop3_b32(q, 0x80808080u, 0u, kTtNotAnd);
    }
}

}  // namespace fsk

#endif
