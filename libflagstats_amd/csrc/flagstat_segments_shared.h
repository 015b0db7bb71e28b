// flagstat_segments_shared.h -- internal: what the eight segmented kernels share (flagstat_segments.hip and its derivations
// flagstat_segments_{filter,where,filter_where,wide,wide_filter,wide_where,wide_filter_where}.hip).
// Device code: the geometry of a wave's unit, the per-flag count of a vector, the clamped grid position of an offset, the search
// and window over the offsets (SegWalk), the walk of a writer over the segments that intersect it (seg_walk<UE>: the kernels hand in
// their chain run, their unit load, their piece count and their emission), the map from a wave's 21 totals to the 32 slots of a
// row and the one emission (seg_emit<COUNT, MASK>).  Host code: launch_shape / wave_totals_fit / fits, the segmented rule of an
// entry's arguments (check_segments), the checks and buffers over host offsets, and the bodies of the three entry forms
// (device_call, sync_call, host_call).
// (Product library only: the entries check allocation extents, which the host-stub build does not have.)
#ifndef FLAGSTAT_SEGMENTS_SHARED_H_
#define FLAGSTAT_SEGMENTS_SHARED_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>

#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_engine.h"
#include "flagstat_segments.h"
#include "flagstat_wide_device.h"

namespace fsk {

constexpr int kSegRowVecs = 64;                    // vectors per row (one per lane)
constexpr int kSegUnitVecs = kSegWaveFlags / 8;    // 512 vectors per unit, 8 KiB, at every element size
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

// The wave's counters of the piece of segment s it holds -> out[s][32]: the chain is flushed, the 21 lane counters are summed
// over the wave (DPP) and reset, lane 63 hands the totals over through red[] and lanes 0-31 of one instruction write the row.
// COUNT: the passing count is summed, handed over and reset with them (red[21]); it is the `len` of the superset slot 9 in
// place of the piece's length, and lane 32 writes it to selected[s] (which may be nullptr).  MASK: the two mask accumulators are
// ORed over the wave and reset (red[21], red[22], one further on with COUNT) and the lane behind the count's -- 32, or 33 with
// COUNT -- writes high[s] (which may be nullptr).  Plain stores where the row is stored plainly (store form, the whole segment in
// this wave), else relaxed agent-scope atomics (add, add, OR) issued only for non-zero values.  A kernel without a count or a
// mask passes any lvalue for cnt, or_even and or_odd: they are not touched.
template <bool COUNT, bool MASK, int DEPTH>
__device__ __forceinline__ void seg_emit(Lane<DEPTH>& st, uint32_t& blk, uint32_t& cnt, uint32_t& or_even, uint32_t& or_odd, uint32_t* red,
                                         uint64_t* __restrict__ out, uint64_t* __restrict__ selected, uint64_t* __restrict__ high, uint64_t s,
                                         uint64_t len, bool plain, int mode, uint32_t lane)
{
    constexpr int kSums = kInternal + (COUNT ? 1 : 0);   // red[0 .. kSums): sums; red[kSums], red[kSums + 1]: the mask
    constexpr uint32_t kMaskLane = COUNT ? 33u : 32u;
    if (blk) {
        flush(st, blk);
        blk = 0;
    }
    uint32_t w[kInternal + 1];
#pragma unroll
    for (int i = 0; i < kInternal; ++i) {
        w[i] = wave_sum_lane63(st.acc[i]);
        st.acc[i] = 0;
    }
    if constexpr (COUNT) {
        w[kInternal] = wave_sum_lane63(cnt);
        cnt = 0;
    }
    uint32_t we = 0, wo = 0;
    if constexpr (MASK) {
        we = wave_or_lane63(or_even & 0xFFFF0000u);   // the even-dword stream: bits 16-31 of every element
        wo = wave_or_lane63(or_odd);                   // W = 8: bits 32-63
        or_even = 0;
        or_odd = 0;
    }
    if (lane == 63) {
#pragma unroll
        for (int i = 0; i < kSums; ++i) red[i] = w[i];
        if constexpr (MASK) {
            red[kSums] = we;
            red[kSums + 1] = wo;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    bool adds = lane < 32;
    if constexpr (COUNT) adds = adds || (lane == 32 && selected != nullptr);
    if (adds) {
        uint64_t add;
        uint64_t* o;
        if constexpr (COUNT) {
            const uint64_t passing = red[kInternal];
            add = lane < 32 ? seg_slot_value(red, lane, mode, passing) : passing;
            o = lane < 32 ? out + s * 32 + lane : selected + s;
        } else {
            add = seg_slot_value(red, lane, mode, len);
            o = out + s * 32 + lane;
        }
        if (plain)
            *o = add;
        else if (add)
            (void)__hip_atomic_fetch_add(o, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (MASK && lane == kMaskLane && high != nullptr) {
        const uint64_t m = (static_cast<uint64_t>(red[kSums + 1]) << 32) | red[kSums];
        if (plain)
            high[s] = m;
        else if (m)
            (void)__hip_atomic_fetch_or(high + s, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// The walk of one wave -- a writer -- over the segments that intersect its run of units, for every segmented kernel.  UE:
// grid positions per unit (kSegWaveFlags, or kSegWideUnitBytes / W).  a chunk's elements occupy grid positions [lo0, hi0) and
// are global elements [base, base + hi0 - lo0); nunits = ceil(hi0 / UE); mode bit 0: store form.  Every lane of the wave is
// active in every call it makes.  The kernel keeps its own state (the lane's chain and counters, its passing count or mask
// accumulators, its row registers, its filter or table) and hands in, as always-inline callables:
//   chain(u, k)       count the k whole units from unit u, all of one segment, through its carry-save chain
//   load(u, whole)    load the 8 rows of unit u, and what rides with them, for the per-piece count: with plain loads if `whole`
//                     (the unit lies wholly inside [lo0, hi0)), else through its guarded loaders
//   piece(w0, b, e)   count the piece [b, e) of the unit loaded last, which starts at grid position w0
//   emit(s, len, plain)  add what it holds to row s and reset it: len is the length of the piece of s this writer holds, plain
//                     says the whole segment lies in this writer and the launch is in the store form
template <uint64_t UE, typename Chain, typename Load, typename Piece, typename Emit>
__device__ __forceinline__ void seg_walk(uint64_t lo0, uint64_t hi0, uint64_t base, const uint64_t* __restrict__ off, uint64_t nseg, int mode,
                                         uint64_t nunits, uint32_t min_units, Chain&& chain, Load&& load, Piece&& piece, Emit&& emit_fn)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kThreads / 64);
    const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * (kThreads / 64) + wave;
    const uint64_t u_begin = gw * nunits / waves, u_end = (gw + 1) * nunits / waves;
    const uint64_t p0 = u_begin * UE > lo0 ? u_begin * UE : lo0;  // this writer: grid positions [p0, E)
    const uint64_t E = u_end * UE < hi0 ? u_end * UE : hi0;
    if (p0 >= E) return;

    SegWalk sw{off, nseg, base, hi0 - lo0, lo0, lane, 0, 0, 0};
    uint64_t s = sw.first_segment(p0);
    if (s >= nseg) return;
    sw.load_window(s);

    bool open = false;  // the kernel's state holds counts of segment s not yet emitted
    uint64_t sb = 0, se = 0;
    auto emit = [&](uint64_t seg, uint64_t b_, uint64_t e_) __attribute__((always_inline)) {
        const uint64_t pb = b_ > p0 ? b_ : p0, pe = e_ < E ? e_ : E;
        emit_fn(seg, pe - pb, (mode & 1) && b_ >= p0 && e_ <= E);
    };

    uint64_t u = p0 / UE;
    while (s < nseg && u < u_end) {
        sw.bounds(s, sb, se);
        const uint64_t w0 = u * UE;
        const uint64_t x = w0 > p0 ? w0 : p0;
        // A segment that begins at or past this writer's end is not its business, nor (monotone offsets) is any later one.  This
        // test comes first: a launch on one chunk of a longer array (the host form) clamps every later segment to an empty one
        // at the chunk's end, and stepping through those one by one would cost the chunk's last writer O(nseg) per launch.
        if (sb >= E) break;
        if (se <= sb || se <= x) {  // empty (or, with malformed offsets, reversed or behind)
            ++s;
            continue;
        }
        if (sb >= w0 + UE) {  // elements before the segment belong to none: skip whole units unread
            u = sb / UE;
            continue;
        }
        const uint64_t seg_e = se < E ? se : E;
        if (sb <= w0 && w0 >= lo0) {
            const uint64_t k = (seg_e - w0) / UE;  // whole units of segment s from here on
            if (k >= min_units && k > 0) {
                chain(u, k);
                u += k;
                open = true;
                if (u * UE >= se) {
                    emit(s, sb, se);
                    open = false;
                    ++s;
                }
                continue;
            }
        }
        // per-piece unit: its 8 rows loaded at once, then every segment piece in it
        load(u, w0 >= lo0 && w0 + UE <= hi0);
        const uint64_t w1 = w0 + UE;
        uint64_t xx = x;
        for (;;) {
            // s < nseg, sb < se, se > xx, sb < w1; the piece [b, e) lies inside [p0, E) and so inside [lo0, hi0)
            const uint64_t b = sb > xx ? sb : xx, e = se < w1 ? se : w1;
            piece(w0, b, e);
            open = true;
            if (e < se) break;  // segment s goes on in the next unit
            emit(s, sb, se);
            open = false;
            ++s;
            xx = e;
            bool more = false;
            while (s < nseg) {
                sw.bounds(s, sb, se);
                if (sb >= E) break;  // (as in the outer walk: before the empty test)
                if (se <= sb || se <= xx) {
                    ++s;
                    continue;
                }
                more = sb < w1;
                break;
            }
            if (!more) break;
        }
        ++u;
    }
    if (open) emit(s, sb, se);  // this writer's range ends inside segment s
}

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

// The segmented rule of an entry's arguments, asked once nseg > 0 (a unit's *_args returns 0 for nseg == 0 in front of it; the
// other rules are flagstat_derived_host.h's): offsets and rows are given -- `null_text` names them as the entry does, d_offsets /
// d_out on the caller's stream -- and the counters of nseg segments can be allocated: at most `max_nseg`, kMaxSegments for rows of
// 32 words, half of it for rows with trailing words (33 or 34).
inline int check_segments(const void* offsets, const void* out, uint64_t nseg, const char* null_text, uint64_t max_nseg)
{
    if (!offsets || !out) return fsint::fail_text(null_text);
    if (nseg > max_nseg) return fsint::fail_text("nseg is too large: its counters cannot be allocated");
    return 0;
}

constexpr const char* kNullHost = "NULL offsets or out with nseg > 0";        // the entries that take host offsets
constexpr const char* kNullDevice = "NULL d_offsets or d_out with nseg > 0";  // the entries on the caller's stream

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

// the masks of a call's result into the caller's host words: stored (flags bit 0) or ORed
inline void apply_masks(uint64_t* high, const uint64_t* got, uint64_t nseg, int flags)
{
    if (!high) return;
    for (uint64_t i = 0; i < nseg; ++i) high[i] = (flags & 1) ? got[i] : (high[i] | got[i]);
}

// rows, selected counts, then masks (34 words per segment) of a synchronous call into the caller's host words: rows and counts
// stored or added, masks stored or ORed
inline void apply_all(uint64_t* out, uint64_t* selected, uint64_t* high, const fsseg::HostRows& got, uint64_t nseg, int flags)
{
    apply_both(out, selected, got, nseg, flags);
    apply_masks(high, got.p.get() + nseg * 33, nseg, flags);
}

// a wave's totals are uint32: every wave must own fewer than 2^32 elements (ue: elements per unit)
inline bool wave_totals_fit(uint64_t nunits, uint32_t g, uint64_t ue)
{
    const uint64_t waves = static_cast<uint64_t>(g) * (fsk::kThreads / 64);
    return (nunits + waves - 1) / waves < (1ull << 32) / ue;
}

// units and workgroups of a launch over m > 0 elements at `addr` with at most `grid` workgroups; ue: elements per 8 KiB unit
// (fsk::kSegWaveFlags, or fsk::kSegWideUnitBytes / W), so an element has W = 8192 / ue bytes
inline void launch_shape(uintptr_t addr, uint64_t m, uint64_t ue, uint32_t grid, uint64_t* lo0, uint64_t* nunits, uint32_t* g)
{
    const uint64_t W = fsk::kSegUnitVecs * 16 / ue;
    *lo0 = (addr & 15u) / W;
    *nunits = (*lo0 + m + ue - 1) / ue;
    const uint64_t want = (*nunits + 3) / 4;  // one unit per wave at least
    *g = want < grid ? static_cast<uint32_t>(want) : grid;
}

// what the entries of the kernels with a fit check refuse once the grid is known
inline int fits(const void* array, uint64_t n, uint64_t ue, uint32_t grid)
{
    if (n == 0) return 0;
    uint64_t lo0 = 0, nunits = 0;
    uint32_t g = 0;
    launch_shape(reinterpret_cast<uintptr_t>(array), n, ue, grid, &lo0, &nunits, &g);
    return wave_totals_fit(nunits, g, ue) ? 0 : fsdrv::fail_wave_totals();
}

// the inputs table of an entry on the caller's stream: the device offsets, in front of the columns the unit then adds
inline fsdrv::Inputs offsets_input(const uint64_t* d_offsets, uint64_t nseg)
{
    fsdrv::Inputs in;
    in.add(d_offsets, "d_offsets", (nseg + 1) * sizeof(uint64_t));
    return in;
}

// ------------------------------------------------------------------ the bodies of the three entry forms, for all eight units
// What differs between the units arrives as arguments and callables (the pattern of flagstat_derived_host.h): the unit's own
// argument check runs in front; its trailing words (none, selected, high, or both), its inputs with the names its refusals use,
// its fit check, its words per segment (32 / 33 / 34), how a chunk's extra column is staged, its launch and how its result is
// applied.  A HIP call that a callable makes goes through FS_HIP_TRY there, so the text of its failure names the caller's own
// expression.

// On the caller's stream (nseg > 0, arguments checked): d_out and the trailing words are plain device memory on one device with
// every input; `fits(grid)` may still refuse; every allocation holds what the call touches of it; then `launch(grid, s)`.
template <typename Fits, typename Launch>
int device_call(const void* d_out, const fsdrv::DeviceWord* words, int nwords, const fsdrv::Input* in, int inputs, uint64_t nseg,
                void* stream, Fits&& fits_fn, Launch&& launch)
{
    int rc;
    fsdrv::DeviceCall call;
    if ((rc = call.open(d_out, words, nwords, in, inputs, stream))) return rc;
    const uint32_t grid = seg_grid(*call.e);
    if ((rc = fits_fn(grid))) return rc;
    if ((rc = fsint::check_extent(d_out, nseg * 32 * sizeof(uint64_t), "d_out"))) return rc;
    for (int k = 0; k < nwords; ++k)
        if (words[k].p && (rc = fsint::check_extent(words[k].p, nseg * sizeof(uint64_t), words[k].name))) return rc;
    for (int i = 0; i < inputs; ++i)
        if ((rc = fsint::check_extent(in[i].p, in[i].bytes, in[i].name))) return rc;
    return launch(grid, call.s);
}

// Synchronous over device memory and host offsets (nseg > 0, arguments checked): the inputs (none if n == 0) live on one device,
// the first one's; under its engine's lock `fits(grid)` may still refuse; rows of `words` uint64 per segment and the offsets get
// device buffers of their own, the offsets are checked and copied, `launch(buf, grid, s)` counts in the store form on the
// engine's first stream and `apply_fn(got)` takes the result to the caller's host words.
template <typename Fits, typename Launch, typename Apply>
int sync_call(const fsdrv::Input* in, int inputs, uint64_t n, const uint64_t* offsets, uint64_t nseg, uint64_t words, Fits&& fits_fn,
              Launch&& launch, Apply&& apply_fn)
{
    int rc, dev = -1, dev_i = -1;
    fsint::Engine* ep = nullptr;
    if (inputs) {
        if ((rc = fsint::device_of_pointer(in[0].p, in[0].name, &dev))) return rc;
        for (int i = 1; i < inputs; ++i) {
            if ((rc = fsint::device_of_pointer(in[i].p, in[i].name, &dev_i))) return rc;
            if (dev_i != dev) return fsdrv::fail_devices(in[i].name, in[0].name);
        }
        ep = fsint::engine_for_device(dev);
    } else {
        ep = fsint::default_engine();
    }
    if (!ep) return -1;
    fsint::Engine& e = *ep;
    std::lock_guard<std::mutex> lk(e.mu);
    if (fsint::engine_alive(e)) return -1;
    fsint::DeviceGuard guard(e.device);
    if (!guard.ok()) return -1;
    const uint32_t grid = seg_grid(e);
    if ((rc = fits_fn(grid))) return rc;
    SegBuffers buf;
    HostRows got;
    if ((rc = buf.alloc(nseg, words)) || (rc = got.alloc(nseg, words))) return rc;
    if ((rc = check_host_offsets(offsets, nseg, n))) return rc;
    for (int i = 0; i < inputs; ++i)
        if ((rc = fsint::check_extent(in[i].p, in[i].bytes, in[i].name))) return rc;
    hipStream_t s = e.stream[0];
    FS_HIP_TRY(hipMemcpyAsync(buf.off, offsets, (nseg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    if ((rc = launch(buf, grid, s))) return rc;
    FS_HIP_TRY(hipMemcpyAsync(got.p.get(), buf.cnt, got.words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    FS_HIP_TRY(hipStreamSynchronize(s));
    apply_fn(got);
    return 0;
}

// Over host memory (nseg > 0, arguments checked): only what some segment covers crosses the bus -- the elements [offsets[0], last)
// in chunks of `chunk` elements, alternating between the default engine's two streams and staging buffers (the copy of chunk
// k + 1 overlaps the kernel on chunk k).  `last_fn()` is offsets[nseg], or offsets[0] where the unit knows that nothing is selected;
// it is asked only once the rows are allocated and the offsets checked (an absurd nseg is refused before offsets[nseg] is read).
// `slot_flags(cap)` is the size of a staging slot in uint16 for chunks of at most `cap` elements; `chunk_fn(e, buf, sl, pos, c,
// cap, grid)` copies the inputs of elements [pos, pos + c) into e.stage[sl] and launches on e.stream[sl]; every chunk's launch
// adds the pieces of the segments it holds to the same device rows (`words` uint64 per segment, zeroed in front).
template <typename Last, typename SlotFlags, typename Chunk, typename Apply>
int host_call(uint64_t n, const uint64_t* offsets, uint64_t nseg, uint64_t words, uint64_t chunk, Last&& last_fn, SlotFlags&& slot_flags,
              Chunk&& chunk_fn, Apply&& apply_fn)
{
    int rc;
    fsint::Engine* ep = fsint::default_engine();
    if (!ep) return -1;
    fsint::Engine& e = *ep;
    std::lock_guard<std::mutex> lk(e.mu);
    if (fsint::engine_alive(e)) return -1;
    fsint::DeviceGuard guard(e.device);
    if (!guard.ok()) return -1;
    fsint::lz4_gpu_other_use(e);
    SegBuffers buf;
    HostRows got;
    if ((rc = buf.alloc(nseg, words)) || (rc = got.alloc(nseg, words))) return rc;
    if ((rc = check_host_offsets(offsets, nseg, n))) return rc;
    if ((rc = fsint::engine_second(e))) return rc;
    const uint64_t first = offsets[0], last = last_fn();
    const uint64_t cap = last - first < chunk ? (last - first ? last - first : 1) : chunk;   // elements of the largest chunk
    const int slots = last - first > chunk ? 2 : 1;
    for (int i = 0; i < slots; ++i)
        if ((rc = fsint::stage_reserve(e, i, slot_flags(cap)))) return rc;
    hipStream_t s0 = e.stream[0];
    FS_HIP_TRY(hipMemsetAsync(buf.cnt, 0, nseg * words * sizeof(uint64_t), s0));
    FS_HIP_TRY(hipMemcpyAsync(buf.off, offsets, (nseg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s0));
    if (slots == 2 && (rc = fsint::stream_wait_stream(e, e.stream[1], s0))) return rc;
    const uint32_t grid = seg_grid(e);
    uint64_t k = 0;
    for (uint64_t pos = first; pos < last; pos += chunk, ++k) {
        const int sl = static_cast<int>(k % static_cast<uint64_t>(slots));
        const uint64_t c = last - pos < chunk ? last - pos : chunk;
        if ((rc = chunk_fn(e, buf, sl, pos, c, cap, grid))) return rc;
    }
    if (slots == 2 && (rc = fsint::stream_wait_stream(e, s0, e.stream[1]))) return rc;
    FS_HIP_TRY(hipMemcpyAsync(got.p.get(), buf.cnt, got.words * sizeof(uint64_t), hipMemcpyDeviceToHost, s0));
    FS_HIP_TRY(hipStreamSynchronize(s0));
    if (slots == 2) FS_HIP_TRY(hipStreamSynchronize(e.stream[1]));
    apply_fn(got);
    return 0;
}

}  // namespace fsseg

#endif
