// flagstat_segments_shared.h -- internal: what the segmented kernels share (flagstat_segments.hip, flagstat_segments_filter.hip).
// Device code: the geometry of a wave's unit, the per-flag count of a vector, the clamped grid position of an offset, the walk
// of a writer over the segments that intersect it (64-ary search, 64-offset window) and the map from a wave's 21 totals to the 32
// slots of a row.  Host code: the checks and buffers of the synchronous entries over host offsets.
// (Product library only: the entries check allocation extents, which the host-stub build does not have.)
#ifndef FLAGSTAT_SEGMENTS_SHARED_H_
#define FLAGSTAT_SEGMENTS_SHARED_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

#include "flagstat_count_core.h"
#include "flagstat_engine.h"
#include "flagstat_segments.h"

namespace fsk {

constexpr int kSegRowVecs = 64;                    // vectors per row (one per lane)
constexpr int kSegUnitVecs = kSegWaveFlags / 8;    // 512 vectors per unit
constexpr int kSegFilterDepth = 8;                 // chain depth of the selecting kernels, as K1: epochs of 255 units

// Per-flag form: 8 flags on their byte planes (L: FLAG bits 0-7, H: bits 8-15; 4 flags per dword) straight into the 21 lane
// counters (T bits 0-7, F bits 0-7, S bits 0-2 and 6-7).
__device__ __forceinline__ void count_planes(uint32_t (&acc)[kInternal], uint32_t L0, uint32_t H0, uint32_t L1, uint32_t H1)
{
    uint32_t T0, T1, qa, qb, ka, kb;
    front4(L0, H0, T0, qa, ka);
    front4(L1, H1, T1, qb, kb);
    const uint32_t F0 = T0 & perm(0u, 0xFF00FF00u, qa), F1 = T1 & perm(0u, 0xFF00FF00u, qb);
    const uint32_t S0 = perm(0u, 0x84428140u, qa) & (ka | 0x3F3F3F3Fu), S1 = perm(0u, 0x84428140u, qb) & (kb | 0x3F3F3F3Fu);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t m = 0x01010101u << c;
        acc[c] += __builtin_popcount(T0 & m) + __builtin_popcount(T1 & m);
        acc[8 + c] += __builtin_popcount(F0 & m) + __builtin_popcount(F1 & m);
    }
#pragma unroll
    for (int c = 0; c < kInternal - 16; ++c) {
        const uint32_t m = 0x01010101u << (c < 3 ? c : c + 3);
        acc[16 + c] += __builtin_popcount(S0 & m) + __builtin_popcount(S1 & m);
    }
}

// the 8 flags of one vector
__device__ __forceinline__ void count8(uint32_t (&acc)[kInternal], const uint4& x)
{
    const uint32_t L0 = perm(x.y, x.x, 0x06040200u), H0 = perm(x.y, x.x, 0x07050301u);
    const uint32_t L1 = perm(x.w, x.z, 0x06040200u), H1 = perm(x.w, x.z, 0x07050301u);
    count_planes(acc, L0, H0, L1, H1);
}

// what lane t < 32 contributes to slot t of a segment row (K1's slot_value, indexed by lane instead of thread)
__device__ __forceinline__ uint64_t seg_slot_value(const uint32_t* tot, uint32_t t, int mode, uint64_t len)
{
    // slot -> internal T index + 1, one nibble per slot (0: no T/F counter): 2->2, 6->6, 7->7, 8->0, 11->3, 12->1, 13->4, 14->5
    constexpr uint64_t kTOfSlot = 0x0652400187000300ull;
    const uint32_t slot = t & 15u;
    const bool fail = t >= 16;
    const int ti = static_cast<int>((kTOfSlot >> (4 * slot)) & 15u) - 1;
    uint64_t add = 0;
    if (ti >= 0) add = fail ? tot[8 + ti] : static_cast<uint64_t>(tot[ti]) - tot[8 + ti];
    if (slot == 10) add = fail ? tot[18] : tot[17];
    if (slot == 9 && fail) add = static_cast<uint64_t>(tot[16]) + tot[18];
    if (mode & 2) {
        if (slot == 0) add = fail ? tot[20] : tot[19];
        if (slot == 9 && !fail) add = len - (static_cast<uint64_t>(tot[16]) + tot[18]);
    }
    return add;
}

// the selecting kernels (flagstat_segments_filter.hip, flagstat_segments_where.hip): the wave's counters of the piece of segment s
// it holds -> out[s][32], and its passing (selected) count -> selected[s]
__device__ __forceinline__ void segf_emit(Lane<kSegFilterDepth>& st, uint32_t& blk, uint32_t& cnt, uint32_t* red, uint64_t* __restrict__ out,
                                          uint64_t* __restrict__ selected, uint64_t s, bool plain, int mode, uint32_t lane)
{
    if (blk) {
        flush(st, blk);
        blk = 0;
    }
    uint32_t w[kInternal + 1];
#pragma unroll
    for (int c = 0; c < kInternal; ++c) {
        w[c] = wave_sum_lane63(st.acc[c]);
        st.acc[c] = 0;
    }
    w[kInternal] = wave_sum_lane63(cnt);
    cnt = 0;
    if (lane == 63) {
#pragma unroll
        for (int c = 0; c <= kInternal; ++c) red[c] = w[c];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < 32 || (lane == 32 && selected != nullptr)) {
        const uint64_t passing = red[kInternal];
        const uint64_t add = lane < 32 ? seg_slot_value(red, lane, mode, passing) : passing;
        uint64_t* o = lane < 32 ? out + s * 32 + lane : selected + s;
        if (plain)
            *o = add;  // store form, the whole segment in this wave: all 32 slots and the count
        else if (add)
            (void)__hip_atomic_fetch_add(o, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_wave_barrier();  // red[] is rewritten by the next segment's totals only after every lane has read it
}

// grid position of offset i: clamped to the chunk [base, base + m]
__device__ __forceinline__ uint64_t seg_pos(const uint64_t* __restrict__ off, uint64_t i, uint64_t base, uint64_t m, uint64_t lo0)
{
    uint64_t v = off[i];
    v = v < base ? base : v;
    v = v > base + m ? base + m : v;
    return v - base + lo0;
}

__device__ __forceinline__ uint64_t uniform64(uint64_t x)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x));
    const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x >> 32));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// every lane of the wave active, all arguments wave-uniform
struct SegWalk {
    const uint64_t* off;
    uint64_t nseg, base, m, lo0;
    uint32_t lane;
    uint64_t wb;             // window: lane i holds the grid position of offset wb + i (clamped to nseg)
    uint32_t wlo, whi;

    __device__ __forceinline__ void load_window(uint64_t first)
    {
        wb = first;
        const uint64_t i = first + lane;
        const uint64_t v = seg_pos(off, i <= nseg ? i : nseg, base, m, lo0);
        wlo = static_cast<uint32_t>(v);
        whi = static_cast<uint32_t>(v >> 32);
    }
    // offsets s and s + 1 (s < nseg)
    __device__ __forceinline__ void bounds(uint64_t s, uint64_t& sb, uint64_t& se)
    {
        if (s + 1 >= wb + 64) load_window(s);
        const int k = static_cast<int>(s - wb);
        sb = (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(whi), k))) << 32) |
             static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(wlo), k));
        se = (static_cast<uint64_t>(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(whi), k + 1))) << 32) |
             static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(wlo), k + 1));
    }
    // the first segment s whose (clamped) end lies beyond grid position p; nseg if none.  64-ary search: one load per lane and
    // round; with monotone offsets the answer is exact, with any offsets it is an index in [0, nseg].
    __device__ __forceinline__ uint64_t first_segment(uint64_t p)
    {
        uint64_t lo = 1, hi = nseg + 1;  // the answer + 1 lies in [lo, hi]
        while (lo < hi) {
            const uint64_t step = (hi - lo + 63) / 64;
            const uint64_t i = lo + lane * step;
            bool gt = true;
            if (i < hi) gt = seg_pos(off, i, base, m, lo0) > p;
            const uint64_t mask = __ballot(gt);
            if (mask == 0) {
                lo = lo + 63 * step + 1;
                continue;
            }
            const uint64_t f = static_cast<uint64_t>(__builtin_ctzll(mask));
            const uint64_t nhi = lo + f * step < hi ? lo + f * step : hi;
            lo = f ? lo + (f - 1) * step + 1 : lo;
            hi = nhi;
            lo = uniform64(lo);
            hi = uniform64(hi);
        }
        return lo - 1;
    }
};

}  // namespace fsk

// ------------------------------------------------------------------ host side of the synchronous entries
namespace fsseg {

constexpr uint64_t kMaxSegments = (~0ull) / 256 - 1;  // nseg * 256 bytes of counters must be a size

// workgroups of a launch by a public entry: the segments policy's blocks per CU
inline uint32_t seg_grid(const fsint::Engine& e)
{
    uint32_t min_units = 0, blocks_per_cu = 1;
    fsk_segments_policy(&min_units, &blocks_per_cu);
    return static_cast<uint32_t>(e.cus) * blocks_per_cu;
}

// host offsets: non-decreasing, last <= n
inline int check_host_offsets(const uint64_t* offsets, uint64_t nseg, uint64_t n)
{
    char buf[192];
    for (uint64_t i = 0; i < nseg; ++i) {
        if (offsets[i + 1] < offsets[i]) {
            std::snprintf(buf, sizeof buf, "offsets must be non-decreasing: offsets[%llu] = %llu > offsets[%llu] = %llu",
                          static_cast<unsigned long long>(i), static_cast<unsigned long long>(offsets[i]),
                          static_cast<unsigned long long>(i + 1), static_cast<unsigned long long>(offsets[i + 1]));
            return fsint::fail_text(buf);
        }
    }
    if (offsets[nseg] > n) {
        std::snprintf(buf, sizeof buf, "offsets[nseg] = %llu exceeds the array's %llu flags",
                      static_cast<unsigned long long>(offsets[nseg]), static_cast<unsigned long long>(n));
        return fsint::fail_text(buf);
    }
    return 0;
}

// device counters + device offsets of one synchronous call; `words` per segment: 32, or 33 with the selected count behind the
// rows (at cnt + nseg * 32)
struct SegBuffers {
    uint64_t* cnt = nullptr;
    uint64_t* off = nullptr;
    ~SegBuffers()
    {
        if (cnt) (void)hipFree(cnt);
        if (off) (void)hipFree(off);
    }
    int alloc(uint64_t nseg, uint64_t words = 32)
    {
        hipError_t e = hipMalloc(&cnt, nseg * words * sizeof(uint64_t));
        if (e != hipSuccess) {
            cnt = nullptr;
            (void)hipGetLastError();
            char buf[160];
            std::snprintf(buf, sizeof buf, "cannot allocate %llu bytes of device counters for %llu segments",
                          static_cast<unsigned long long>(nseg * words * 8), static_cast<unsigned long long>(nseg));
            return fsint::fail_text(buf);
        }
        e = hipMalloc(&off, (nseg + 1) * sizeof(uint64_t));
        if (e != hipSuccess) {
            off = nullptr;
            return fsint::fail_hip("hipMalloc(segment offsets)", e);
        }
        return 0;
    }
};

inline int host_args(const uint64_t* offsets, uint64_t nseg, const void* out)
{
    if (!offsets || !out) return fsint::fail_text("NULL offsets or out with nseg > 0");
    if (nseg > kMaxSegments) return fsint::fail_text("nseg is too large: its counters cannot be allocated");
    return 0;
}

// host copy of the device rows: allocated without exceptions (none may cross the C boundary), before any GPU work is queued
struct HostRows {
    std::unique_ptr<uint64_t[]> p;
    uint64_t words = 0;
    int alloc(uint64_t nseg, uint64_t words_per_segment = 32)
    {
        words = nseg * words_per_segment;
        p.reset(new (std::nothrow) uint64_t[words]);
        if (!p) {
            char buf[160];
            std::snprintf(buf, sizeof buf, "cannot allocate %llu bytes of host memory for the rows of %llu segments",
                          static_cast<unsigned long long>(words * 8), static_cast<unsigned long long>(nseg));
            return fsint::fail_text(buf);
        }
        return 0;
    }
};

// `words` of a call's result into the caller's host words: stored (flags bit 0) or accumulated
inline void apply(uint64_t* out, const uint64_t* got, uint64_t words, int flags)
{
    if (flags & 1)
        std::memcpy(out, got, words * sizeof(uint64_t));
    else
        for (uint64_t i = 0; i < words; ++i) out[i] += got[i];
}

// rows, then selected counts, of a synchronous call into the caller's host words
inline void apply_both(uint64_t* out, uint64_t* selected, const fsseg::HostRows& got, uint64_t nseg, int flags)
{
    fsseg::apply(out, got.p.get(), nseg * 32, flags);
    if (selected) fsseg::apply(selected, got.p.get() + nseg * 32, nseg, flags);
}

// a wave's totals are uint32: every wave must own fewer than 2^32 flags
inline bool wave_totals_fit(uint64_t nunits, uint32_t g)
{
    const uint64_t waves = static_cast<uint64_t>(g) * (fsk::kThreads / 64);
    return (nunits + waves - 1) / waves < (1ull << 32) / fsk::kSegWaveFlags;
}

// units and workgroups of a launch over m > 0 uint16 flags at `addr` with at most `grid` workgroups
inline void launch_shape(uintptr_t addr, uint64_t m, uint32_t grid, uint64_t* lo0, uint64_t* nunits, uint32_t* g)
{
    *lo0 = (addr & 15u) / 2;
    *nunits = (*lo0 + m + fsk::kSegWaveFlags - 1) / fsk::kSegWaveFlags;
    const uint64_t want = (*nunits + 3) / 4;  // one unit per wave at least
    *g = want < grid ? static_cast<uint32_t>(want) : grid;
}

}  // namespace fsseg

#endif
