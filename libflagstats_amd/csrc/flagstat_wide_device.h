// flagstat_wide_device.h -- internal, device code only: what the kernels over 4-byte and 8-byte elements share
// (flagstat_wide.hip, flagstat_wide_filter.hip, flagstat_segments_wide.hip, flagstat_segments_wide_filter.hip): the read-out of a
// loaded vector into the pair dword P and the mask accumulators, the short carry-save tree of a step with 8 or 4 inputs, the
// unfiltered step built from them (wide_step_with), the guarded loader of an edge step, the zeroing of a vector's elements outside
// a range and the OR over a wave.  How the pieces fit is written out at the top of flagstat_wide.hip.
#ifndef FLAGSTAT_WIDE_DEVICE_H_
#define FLAGSTAT_WIDE_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flagstat_count_core.h"

namespace fsk {

// Read a just-loaded vector out of its registers AT THIS POINT of the instruction stream (they are re-targeted by the load of
// a later vector right after, as in K1's split_out): the flag-carrying dwords pairwise to P = [a.b0, b.b0, a.b1, b.b1], every
// dword into the mask accumulators.  W = 4: two P (elements 0,1 and 2,3).  W = 8: one P (the even dwords), p1 untouched.
template <int W>
__device__ __forceinline__ void narrow_out(const uint4& o, uint32_t& p0, uint32_t& p1, uint32_t& or_even, uint32_t& or_odd)
{
    const uint32_t sel = 0x05010400u;
    if constexpr (W == 4) {
        asm volatile("v_perm_b32 %0, %4, %3, %7\n\tv_perm_b32 %1, %6, %5, %7\n\tv_or3_b32 %2, %2, %3, %4\n\tv_or3_b32 %2, %2, %5, %6"
                     : "=&v"(p0), "=&v"(p1), "+v"(or_even)
                     : "v"(o.x), "v"(o.y), "v"(o.z), "v"(o.w), "s"(sel));
    } else {
        asm volatile("v_perm_b32 %0, %5, %3, %7\n\tv_or3_b32 %1, %1, %3, %5\n\tv_or3_b32 %2, %2, %4, %6"
                     : "=&v"(p0), "+v"(or_even), "+v"(or_odd)
                     : "v"(o.x), "v"(o.y), "v"(o.z), "v"(o.w), "s"(sel));
    }
}

// one level of K1's carry-save tree on CNT inputs of the plane's weight (CNT == 1: the lone carry walks up)
template <int CNT, int N>
__device__ __forceinline__ void wide_level(uint32_t (&x)[N], uint32_t& plane)
{
    if constexpr (CNT >= 2) {
#pragma unroll
        for (int i = 0; i < CNT / 2; ++i) csa(x[i], plane, plane, x[2 * i], x[2 * i + 1]);
    } else {
        csa(x[0], plane, plane, x[0], 0u);
    }
}

// N inputs of weight 1 through the planes of weight 1, 2, 4, 8: the weight-16 carry
template <int N>
__device__ __forceinline__ uint32_t wide_tree(uint32_t (&x)[N], uint32_t& p1, uint32_t& p2, uint32_t& p4, uint32_t& p8)
{
    static_assert(N == 4 || N == 8, "a 32 KiB step holds 8 (W = 4) or 4 (W = 8) inputs per lane");
    wide_level<N>(x, p1);
    wide_level<N / 2>(x, p2);
    wide_level<N / 4>(x, p4);
    wide_level<(N >= 8 ? N / 8 : 1)>(x, p8);
    return x[0];
}

// One step: 8 vectors of 16 B per lane = 32 / W inputs of 4 flags each, ONE weight-16 push into the lane's chain at `blk`.
// `reissue_vec(u)` is the caller's re-issue of vector u's registers right after they have been read out, between the two
// sched_barriers of a rolling schedule (K1's schedule 71 through reissue(), at the caller's stride between a lane's consecutive
// loads: kWaveStride in flagstat_wide.hip, kSegRowVecs in flagstat_segments_wide.hip), or nothing when the vectors are all in v[].
// `select_vec(u)` runs right in front of the read-out and may change v[u] in its registers: flagstat_wide_where.hip zeroes the
// elements that its selection leaves out there, so that neither the counters nor the mask accumulators see them.
template <int W, int DEPTH, typename Reissue, typename Select>
__device__ __forceinline__ void wide_step_with(Lane<DEPTH>& s, uint4 (&v)[kUnroll], uint32_t blk, uint32_t& or_even, uint32_t& or_odd,
                                               Reissue&& reissue_vec, Select&& select_vec)
{
    constexpr int NIN = 32 / W;
    uint32_t T[NIN], F[NIN], S[NIN];
    uint32_t held = 0;       // W = 8: the even vector's P until the odd one's arrives
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        uint32_t p0, p1 = 0;
        __builtin_amdgcn_sched_barrier(0);
        select_vec(u);
        narrow_out<W>(v[u], p0, p1, or_even, or_odd);
        reissue_vec(u);
        __builtin_amdgcn_sched_barrier(0);
        if (W == 8 && (u & 1) == 0) {
            held = p0;
            continue;
        }
        const uint32_t a = W == 4 ? p0 : held, b = W == 4 ? p1 : p0;   // flags 0,1 and 2,3
        const uint32_t L = perm(b, a, 0x05040100u), H = perm(b, a, 0x07060302u);
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

// the step over every element of its vectors
template <int W, int DEPTH, typename Reissue>
__device__ __forceinline__ void wide_step_with(Lane<DEPTH>& s, uint4 (&v)[kUnroll], uint32_t blk, uint32_t& or_even, uint32_t& or_odd,
                                               Reissue&& reissue_vec)
{
    wide_step_with<W>(s, v, blk, or_even, or_odd, reissue_vec, [](int) __attribute__((always_inline)) {});
}

// Vector j of the 16-byte grid holds element positions [j * 16 / W, (j + 1) * 16 / W); positions in [lo, hi) are the caller's
// elements, everything else reads as zero.  Only dwords of elements inside [lo, hi) are ever read.
template <int W>
__device__ __forceinline__ uint4 load_guarded_wide(const uint4* __restrict__ a0, uint64_t j, uint64_t lo, uint64_t hi)
{
    constexpr int EPV = 16 / W, DPE = W / 4;
    const uint64_t f0 = j * EPV;
    if (f0 >= lo && f0 + EPV <= hi) return a0[j];
    uint32_t w[4] = {0, 0, 0, 0};
    if (f0 + EPV <= lo || f0 >= hi) return make_uint4(0, 0, 0, 0);
    const uint32_t* p = reinterpret_cast<const uint32_t*>(a0 + j);
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
        const uint64_t f = f0 + e;
        if (f >= lo && f < hi) {
#pragma unroll
            for (int d = 0; d < DPE; ++d) w[e * DPE + d] = p[e * DPE + d];
        }
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// the elements of vector x (grid positions q .. q + 16 / W - 1) that lie in [b, e); every dword of the others becomes 0
template <int W>
__device__ __forceinline__ uint4 mask_vec_wide(uint4 x, uint64_t q, uint64_t b, uint64_t e)
{
    constexpr uint32_t EPV = 16 / W;
    const uint32_t lk = b > q ? static_cast<uint32_t>(b - q < EPV ? b - q : EPV) : 0u;  // first kept element
    const uint32_t hk = e > q ? static_cast<uint32_t>(e - q < EPV ? e - q : EPV) : 0u;  // one past the last
    auto keep = [&](uint32_t k) { return k >= lk && k < hk ? 0xFFFFFFFFu : 0u; };
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
    return x;
}

// OR of x over the 64 lanes of a wave, valid in lane 63 only (the DPP steps of wave_sum_lane63 with | for +; lanes a step does
// not write read 0)
__device__ __forceinline__ uint32_t wave_or_lane63(uint32_t x)
{
    x |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0xB1, 0xF, 0xF, false));
    x |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x4E, 0xF, 0xF, false));
    x |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x141, 0xF, 0xF, false));
    x |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x140, 0xF, 0xF, false));
    x |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x142, 0xA, 0xF, false));
    x |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x143, 0xC, 0xF, false));
    return x;
}

}  // namespace fsk

#endif
