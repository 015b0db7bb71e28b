// flagstat_wide_filter_device.h -- internal, device code only: what the filtered kernels over 4-byte and 8-byte elements share
// (flagstat_wide_filter.hip: one row for the whole array; flagstat_segments_wide_filter.hip: one row per segment).  The MAPQ
// loaders on the grid of W-byte elements, the bits that say which positions of a vector are elements, and the filtered step:
// the wide kernel's step (flagstat_wide_device.h) with pass4 (flagstat_filter_device.h) in front of front4.  How the pieces fit,
// and why the MAPQ bytes of an 8-byte group come from two places, is written out at the top of flagstat_wide_filter.hip.
#ifndef FLAGSTAT_WIDE_FILTER_DEVICE_H_
#define FLAGSTAT_WIDE_FILTER_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flagstat_count_core.h"
#include "flagstat_filter_device.h"
#include "flagstat_wide_device.h"

namespace fsk {

typedef uint32_t mq_u32_any __attribute__((aligned(1)));
typedef uint16_t mq_u16_any __attribute__((aligned(1)));

// the MAPQ bytes of one vector all of whose positions are elements: 4 bytes (W = 4) or 2, in the low half (W = 8)
template <int W>
__device__ __forceinline__ uint32_t load_mapq_wide(const uint8_t* __restrict__ p)
{
    if constexpr (W == 4)
        return __builtin_nontemporal_load(reinterpret_cast<const mq_u32_any*>(p));
    else
        return __builtin_nontemporal_load(reinterpret_cast<const mq_u16_any*>(p));
}

// the MAPQ bytes of vector j at an edge, in the same layout: bytes of positions outside [lo, hi) are not touched and read as 0
template <int W>
__device__ __forceinline__ uint32_t load_mapq_wide_guarded(const uint8_t* __restrict__ mq, uint64_t j, uint64_t lo, uint64_t hi)
{
    constexpr int EPV = 16 / W;
    const uint64_t f0 = j * EPV;
    uint32_t w = 0;
    if (f0 + EPV <= lo || f0 >= hi) return 0u;
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
        const uint64_t f = f0 + e;
        if (f >= lo && f < hi) w |= static_cast<uint32_t>(mq[f]) << (8 * e);
    }
    return w;
}

// bit e of the result: position j * 16 / W + e lies in [lo, hi) (4 bits at W = 4, 2 at W = 8)
template <int W>
__device__ __forceinline__ uint32_t valid_bits_wide(uint64_t j, uint64_t lo, uint64_t hi)
{
    constexpr uint32_t EPV = 16 / W;
    const uint64_t f0 = j * EPV;
    if (f0 + EPV <= lo || f0 >= hi) return 0u;
    const uint32_t e0 = f0 >= lo ? 0u : static_cast<uint32_t>(lo - f0);
    const uint32_t e1 = f0 + EPV <= hi ? EPV - 1 : static_cast<uint32_t>(hi - 1 - f0);
    constexpr uint32_t all = (1u << EPV) - 1u;
    return (all >> (EPV - 1 - e1)) & (all << e0) & all;
}

// One step: 8 vectors of 16 B per lane = 32 / W groups of 4 flags each, the predicate applied to every group in front of front4.
// ROLL 0 (edge steps, per-piece units): the vectors are in v[], their MAPQ bytes in m[], the bits of their positions that are
// elements in vb[] (the pass bits of the others are cleared).  ROLL 1, 2: K1's schedule 71 through reissue(); the MAPQ bytes of a
// vector are re-issued right in front of it; vb[] is not looked at.  STRIDE: vectors between a lane's consecutive loads
// (kWaveStride in flagstat_wide_filter.hip, kSegRowVecs in flagstat_segments_wide_filter.hip), 16 / W MAPQ bytes each.
// (Unlike wide_step_with the re-issue is not the caller's callable: with a callable the compiler keeps a non-temporal hint on the
// first MAPQ load of the loop that it drops in this form, and the two flagstat_count_wide_filter<W, true> kernels would differ from
// their measured form in that instruction.)
template <int W, bool MAPQ, int ROLL, int STRIDE, int DEPTH>
__device__ __forceinline__ void wide_filter_step_with(Lane<DEPTH>& s, const FilterArgs& f, uint4 (&v)[kUnroll], uint32_t (&m)[kUnroll],
                                                      const uint32_t (&vb)[kUnroll], uint32_t blk, uint32_t& cnt, uint32_t& or_even,
                                                      uint32_t& or_odd, const uint4* __restrict__ cur, const uint4* __restrict__ next,
                                                      const uint8_t* __restrict__ mcur, const uint8_t* __restrict__ mnext)
{
    constexpr int NIN = 32 / W;
    uint32_t T[NIN], F[NIN], S[NIN];
    uint32_t held = 0, held_mq = 0;   // W = 8: the even vector's P and MAPQ bytes until the odd one's arrive
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        uint32_t p0, p1 = 0, w = 0;
        __builtin_amdgcn_sched_barrier(0);
        narrow_out<W>(v[u], p0, p1, or_even, or_odd);
        if constexpr (MAPQ) {
            w = m[u];
            reissue<ROLL>(u, m, mcur, mnext, STRIDE * (16 / W), load_mapq_wide<W>);
        }
        reissue<ROLL>(u, v, cur, next, STRIDE, load_vec<true>);
        __builtin_amdgcn_sched_barrier(0);
        if (W == 8 && (u & 1) == 0) {
            held = p0;
            held_mq = w;
            continue;
        }
        const uint32_t a = W == 4 ? p0 : held, b = W == 4 ? p1 : p0;   // flags 0,1 and 2,3
        uint32_t L = perm(b, a, 0x05040100u), H = perm(b, a, 0x07060302u);
        if (W == 8) w = held_mq | (w << 16);
        uint32_t p = pass4<MAPQ>(f, L, H, w);
        if constexpr (ROLL == 0) p &= nibble_to_bit7(W == 4 ? vb[u] : (vb[u - (W == 8)] | (vb[u] << 2)));
        cnt += __builtin_popcount(p);
        const uint32_t M = perm(0u, 0u, p);   // selector 0x80 -> 0xFF, 0x00 -> source byte 0 = 0x00
        L &= M;
        H &= M;
        const int i = W == 4 ? u : u / 2;
        uint32_t q, k;
        front4(L, H, T[i], q, k);
        F[i] = T[i] & perm(0u, 0xFF00FF00u, q);
        S[i] = perm(0u, 0x84428140u, q) & (k | 0x3F3F3F3Fu);
    }
    const uint32_t ct = wide_tree(T, s.t1, s.t2, s.t4, s.t8);
    const uint32_t cf = wide_tree(F, s.f1, s.f2, s.f4, s.f8);
    const uint32_t cs = wide_tree(S, s.s1, s.s2, s.s4, s.s8);
    chain_push<0, DEPTH>(s, blk, ct, cf, cs);
}

}  // namespace fsk

#endif
