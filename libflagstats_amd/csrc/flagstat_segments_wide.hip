// flagstat_segments_wide.hip -- segmented flagstat of a FLAG array held as 4-byte or 8-byte little-endian integers (int32 / int64
// columns), read in place: one row of 32 counters per CSR segment, counted from the low 16 bits of its elements exactly as the
// uint16 segmented kernel counts them, and per segment the OR of every bit above bit 15 that one of ITS elements carries, in one
// launch.  The segmented kernel's work split, walk and emission (flagstat_segments.hip) over the wide kernel's read-out of an
// element (flagstat_wide.hip).
//
// Geometry.  The array is addressed on the 16-byte grid of its aligned-down base; positions are elements of W bytes.  A wave's
// unit stays 8 KiB -- 8 rows of 64 lanes x 16 B, 2048 elements at W = 4 and 1024 at W = 8, exactly one wave's share of a wide-kernel
// step -- so every load instruction of a wave still covers 1 KiB contiguously.  Every wave of the grid is a writer over a
// contiguous run of units; SegWalk, seg_pos and seg_slot_value (flagstat_segments_shared.h) work in positions and are used as they
// are.  tests/segments_wide_oracle.WideWriterSplit mirrors the split.
//
// Two regimes, chosen per stretch as in flagstat_segments.hip (the same policy: fsk_segments_policy):
//   * a run of at least `min_units` whole units inside one segment goes through the wide kernel's step (wide_step_with of
//     flagstat_wide_device.h: narrow_out, front4, wide_tree over 32 / W inputs, one weight-16 chain_push per unit) under K1's
//     rolling load schedule with the contiguous per-wave stride; epochs of 255 units, flushed exactly when the segment ends;
//   * every other unit is loaded once (through load_guarded_wide where it is not wholly inside the array) and counted per piece:
//     the elements of a vector outside the piece [b, e) of one segment are zeroed -- all their dwords -- then the vector is
//     narrowed to byte planes with the wide kernel's two perms and counted with count_planes, 2 (W = 4) or 4 (W = 8) rows a call.
//
// Mask.  Both regimes OR dwords into the lane's or_even / or_odd, which hold bits of the open segment only: a chain unit lies
// wholly inside its segment, and the per-piece form ORs a vector after the foreign elements have been zeroed.  At a segment's
// emission the even stream is cut to bits 16-31, the wave ORs over its lanes (DPP), both accumulators are reset, and lane 32 of
// the instruction that writes the row writes high[s]: a plain store where the row is stored plainly, else one relaxed
// agent-scope atomic OR, only if the word is non-zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_engine.h"
#include "flagstat_segments.h"
#include "flagstat_segments_shared.h"
#include "flagstat_segments_wide.h"
#include "flagstat_segments_wide_device.h"
#include "flagstat_wide_device.h"

namespace fsk {

constexpr int kSegWideDepth = 8;   // chain depth as K1: epochs of 255 units

template <int W, bool HAS_NEXT>
__device__ __forceinline__ void segw_step_and_count(Lane<kSegWideDepth>& s, uint4 (&v)[kUnroll], uint32_t& blk, uint32_t& or_even,
                                                    uint32_t& or_odd, const uint4* cur, const uint4* next)
{
    blk = __builtin_amdgcn_readfirstlane(blk);
    wide_step_with<W>(s, v, blk, or_even, or_odd, [&](int u) __attribute__((always_inline)) {
        reissue<HAS_NEXT ? 1 : 2>(u, v, cur, next, kSegRowVecs, load_vec<true>);
    });
    end_step<kSegWideDepth>(s, blk);
}

// the piece [b, e) of the unit starting at grid position w0 (its 8 rows in v[]) into the lane counters and the lane's mask
// accumulators; only dwords of elements inside the piece reach either (count_piece_wide_with of flagstat_segments_wide_device.h,
// nothing done to the planes)
template <int W>
__device__ __forceinline__ void count_piece_wide(uint32_t (&acc)[kInternal], uint32_t& or_even, uint32_t& or_odd, const uint4 (&v)[kUnroll],
                                                 uint64_t w0, uint64_t b, uint64_t e, uint32_t lane)
{
    count_piece_wide_with<W>(acc, or_even, or_odd, v, w0, b, e, lane,
                             [](int, uint32_t&, uint32_t&, uint32_t&, uint32_t&) __attribute__((always_inline)) {});
}

// the wave's counters of the piece of segment s it holds -> out[s][32], and the piece's mask -> high[s]
__device__ __forceinline__ void segw_emit(Lane<kSegWideDepth>& st, uint32_t& blk, uint32_t& or_even, uint32_t& or_odd, uint32_t* red,
                                          uint64_t* __restrict__ out, uint64_t* __restrict__ high, uint64_t s, uint64_t len, bool plain,
                                          int mode, uint32_t lane)
{
    if (blk) {
        flush(st, blk);
        blk = 0;
    }
    uint32_t w[kInternal];
#pragma unroll
    for (int c = 0; c < kInternal; ++c) {
        w[c] = wave_sum_lane63(st.acc[c]);
        st.acc[c] = 0;
    }
    const uint32_t we = wave_or_lane63(or_even & 0xFFFF0000u);   // the even-dword stream: bits 16-31 of every element
    const uint32_t wo = wave_or_lane63(or_odd);                   // W = 8: bits 32-63
    or_even = 0;
    or_odd = 0;
    if (lane == 63) {
#pragma unroll
        for (int c = 0; c < kInternal; ++c) red[c] = w[c];
        red[kInternal] = we;
        red[kInternal + 1] = wo;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < 32) {
        const uint64_t add = seg_slot_value(red, lane, mode, len);
        uint64_t* o = out + s * 32 + lane;
        if (plain)
            *o = add;  // store form, the whole segment in this wave: all 32 slots
        else if (add)
            (void)__hip_atomic_fetch_add(o, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (lane == 32 && high != nullptr) {
        const uint64_t m = (static_cast<uint64_t>(red[kInternal + 1]) << 32) | red[kInternal];
        if (plain)
            high[s] = m;
        else if (m)
            (void)__hip_atomic_fetch_or(high + s, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_wave_barrier();  // red[] is rewritten by the next segment's totals only after every lane has read it
}

// a0: 16-B aligned-down base; the chunk's elements occupy grid positions [lo0, hi0) (elements of W bytes) and are global elements
// [base, base + hi0 - lo0).  nunits = ceil(hi0 / (8192 / W)).  mode: bit 0 store form (out[] and high[] zeroed in front), bit 1
// superset.  high may be nullptr.
template <int W>
__global__ __launch_bounds__(kThreads) void flagstat_segments_wide(const uint4* __restrict__ a0, uint64_t lo0, uint64_t hi0, uint64_t base,
                                                                   const uint64_t* __restrict__ off, uint64_t nseg,
                                                                   uint64_t* __restrict__ out, uint64_t* __restrict__ high, int mode,
                                                                   uint64_t nunits, uint32_t min_units)
{
    static_assert(W == 4 || W == 8, "4-byte or 8-byte elements");
    constexpr uint64_t UE = kSegWideUnitBytes / W;   // elements per unit
    __shared__ uint32_t red_all[kThreads / 64][24];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kThreads / 64);
    const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * (kThreads / 64) + wave;
    const uint64_t u_begin = gw * nunits / waves, u_end = (gw + 1) * nunits / waves;
    const uint64_t p0 = u_begin * UE > lo0 ? u_begin * UE : lo0;  // this writer: grid positions [p0, E)
    const uint64_t E = u_end * UE < hi0 ? u_end * UE : hi0;
    if (p0 >= E) return;
    uint32_t* red = red_all[wave];

    SegWalk sw{off, nseg, base, hi0 - lo0, lo0, lane, 0, 0, 0};
    uint64_t s = sw.first_segment(p0);
    if (s >= nseg) return;
    sw.load_window(s);

    Lane<kSegWideDepth> st;
    lane_init(st);
    uint32_t blk = 0;
    uint32_t or_even = 0, or_odd = 0;   // dwords of segment s's elements not yet emitted
    bool open = false;                  // st and the mask accumulators hold segment s's, not yet emitted
    uint64_t sb = 0, se = 0;
    auto emit = [&](uint64_t seg, uint64_t b_, uint64_t e_) {
        const uint64_t pb = b_ > p0 ? b_ : p0, pe = e_ < E ? e_ : E;
        segw_emit(st, blk, or_even, or_odd, red, out, high, seg, pe - pb, (mode & 1) && b_ >= p0 && e_ <= E, mode, lane);
    };

    uint64_t u = p0 / UE;
    while (s < nseg && u < u_end) {
        sw.bounds(s, sb, se);
        const uint64_t w0 = u * UE;
        const uint64_t x = w0 > p0 ? w0 : p0;
        // (the order of these tests is flagstat_segments.hip's, for its reasons)
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
                const uint4* p = a0 + u * kSegUnitVecs + lane;
                uint4 v[kUnroll];
#pragma unroll
                for (int r = 0; r < kRollDistance; ++r) {
                    v[r] = load_vec<true>(p + r * kSegRowVecs);
                    __builtin_amdgcn_sched_barrier(0);
                }
                for (uint64_t i = 1; i < k; ++i) {
                    const uint4* pn = p + kSegUnitVecs;
                    segw_step_and_count<W, true>(st, v, blk, or_even, or_odd, p, pn);
                    p = pn;
                }
                segw_step_and_count<W, false>(st, v, blk, or_even, or_odd, p, nullptr);
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
        uint4 v[kUnroll];
        const uint64_t j0 = u * kSegUnitVecs + lane;
        if (w0 >= lo0 && w0 + UE <= hi0) {
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) v[r] = load_vec<true>(a0 + j0 + r * kSegRowVecs);
        } else {
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) v[r] = load_guarded_wide<W>(a0, j0 + r * kSegRowVecs, lo0, hi0);
        }
        const uint64_t w1 = w0 + UE;
        uint64_t xx = x;
        for (;;) {
            // s < nseg, sb < se, se > xx, sb < w1; the piece [b, e) lies inside [p0, E) and so inside [lo0, hi0)
            const uint64_t b = sb > xx ? sb : xx, e = se < w1 ? se : w1;
            count_piece_wide<W>(st.acc, or_even, or_odd, v, w0, b, e, lane);
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

// ------------------------------------------------------------------ launcher
namespace {

// a wave's totals are uint32: every wave must own fewer than 2^32 elements
bool wave_totals_fit(uint64_t nunits, uint32_t g, uint64_t unit_elems)
{
    const uint64_t waves = static_cast<uint64_t>(g) * (fsk::kThreads / 64);
    return (nunits + waves - 1) / waves < (1ull << 32) / unit_elems;
}

// units and workgroups of a launch over m > 0 elements of W bytes at `addr` with at most `grid` workgroups
void launch_shape(uintptr_t addr, uint64_t m, uint64_t W, uint32_t grid, uint64_t* lo0, uint64_t* nunits, uint32_t* g)
{
    const uint64_t ue = fsk::kSegWideUnitBytes / W;
    *lo0 = (addr & 15u) / W;
    *nunits = (*lo0 + m + ue - 1) / ue;
    const uint64_t want = (*nunits + 3) / 4;  // one unit per wave at least
    *g = want < grid ? static_cast<uint32_t>(want) : grid;
}

}  // namespace

extern "C" hipError_t fsk_launch_segments_wide(const void* d_chunk, int elem_bytes, uint64_t base, uint64_t m, const uint64_t* d_offsets,
                                               uint64_t nseg, uint64_t* d_out, uint64_t* d_high, int mode, uint32_t grid,
                                               hipStream_t stream)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || (mode & ~3) || grid == 0) return hipErrorInvalidValue;
    if (nseg == 0) return hipSuccess;
    if (d_out == nullptr || d_offsets == nullptr || (m && d_chunk == nullptr)) return hipErrorInvalidValue;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_chunk);
    if ((addr & (W - 1)) || m > (~0ull - 64) / W) return hipErrorInvalidValue;
    uint64_t lo0 = 0, nunits = 0;
    uint32_t g = 0;
    if (m) {
        launch_shape(addr, m, W, grid, &lo0, &nunits, &g);
        if (!wave_totals_fit(nunits, g, fsk::kSegWideUnitBytes / W)) return hipErrorInvalidValue;
    }
    if (mode & 1) {
        const bool together = d_high == d_out + nseg * 32;
        hipError_t e = fsk_zero_words(d_out, together ? nseg * 33 : nseg * 32, stream);
        if (e == hipSuccess && d_high && !together) e = fsk_zero_words(d_high, nseg, stream);
        if (e != hipSuccess) return e;
    }
    if (m == 0) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(addr & ~static_cast<uintptr_t>(15));
    const uint64_t hi0 = lo0 + m;
    uint32_t min_units = 0, blocks_per_cu = 0;
    fsk_segments_policy(&min_units, &blocks_per_cu);
    const dim3 gd(g), bd(fsk::kThreads);
    if (elem_bytes == 4)
        hipLaunchKernelGGL(fsk::flagstat_segments_wide<4>, gd, bd, 0, stream, a0, lo0, hi0, base, d_offsets, nseg, d_out, d_high, mode & 3,
                           nunits, min_units);
    else
        hipLaunchKernelGGL(fsk::flagstat_segments_wide<8>, gd, bd, 0, stream, a0, lo0, hi0, base, d_offsets, nseg, d_out, d_high, mode & 3,
                           nunits, min_units);
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
using fsint::DeviceGuard;
using fsint::Engine;
using fsint::fail_text;
using fsseg::seg_grid;

namespace {

// what every form refuses before it touches the GPU (nseg > 0 from the NULL checks on)
int segw_args(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg, const void* out, int flags,
              const char* null_text)
{
    if (elem_bytes == 2)
        return fail_text("elem_bytes 2: 16-bit arrays go to the u16 entries (FLAGSTATS_hip_u16_x64_segments, FLAGSTATS_hip_device_u16_segments)");
    if (elem_bytes != 4 && elem_bytes != 8) return fail_text("elem_bytes must be 4 or 8");
    if (flags & ~3) return fail_text("flags: bit 0 store, bit 1 superset; no other bits");
    if (nseg == 0) return 0;
    if (!offsets || !out) return fail_text(null_text);
    if (nseg > fsseg::kMaxSegments / 2) return fail_text("nseg is too large: its counters cannot be allocated");   // 33 words each
    if (n && !array) return fail_text("NULL array with n > 0");
    if (reinterpret_cast<uintptr_t>(array) & static_cast<uintptr_t>(elem_bytes - 1))
        return fail_text(elem_bytes == 4 ? "array must be 4-byte aligned (elem_bytes 4)" : "array must be 8-byte aligned (elem_bytes 8)");
    if (n > (~0ull - 64) / static_cast<uint64_t>(elem_bytes)) return fail_text("n * elem_bytes is not a size");
    return 0;
}

int segw_fits(const void* array, uint64_t n, int elem_bytes, uint32_t grid)
{
    if (n == 0) return 0;
    uint64_t lo0 = 0, nunits = 0;
    uint32_t g = 0;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    launch_shape(reinterpret_cast<uintptr_t>(array), n, W, grid, &lo0, &nunits, &g);
    if (!wave_totals_fit(nunits, g, fsk::kSegWideUnitBytes / W))
        return fail_text("n is too large for this grid: a wave's uint32 totals could overflow (split the array)");
    return 0;
}

// rows, then masks, of a synchronous call into the caller's host words: rows stored or added, masks stored or ORed
void apply_rows_and_masks(uint64_t* out, uint64_t* high, const fsseg::HostRows& got, uint64_t nseg, int flags)
{
    fsseg::apply(out, got.p.get(), nseg * 32, flags);
    if (!high) return;
    const uint64_t* m = got.p.get() + nseg * 32;
    for (uint64_t i = 0; i < nseg; ++i) high[i] = (flags & 1) ? m[i] : (high[i] | m[i]);
}

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_wide_segments(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* d_offsets, uint64_t nseg,
                                       uint64_t* d_out, uint64_t* d_high, int flags, void* stream)
{
    FS_ENTRY();
    int rc = segw_args(d_array, n, elem_bytes, d_offsets, nseg, d_out, flags, "NULL d_offsets or d_out with nseg > 0");
    if (rc || nseg == 0) return rc;
    const fsdrv::DeviceWord word{d_high, "d_high", "the masks are ORed with device atomics"};
    const fsdrv::Input in[] = {{d_offsets, "d_offsets", (nseg + 1) * sizeof(uint64_t)}, {d_array, "d_array", n * static_cast<uint64_t>(elem_bytes)}};
    const int inputs = n ? 2 : 1;
    fsdrv::DeviceCall call;
    if ((rc = call.open(d_out, word, in, inputs, stream))) return rc;
    const uint32_t grid = seg_grid(*call.e);
    if ((rc = segw_fits(d_array, n, elem_bytes, grid))) return rc;
    if ((rc = fsint::check_extent(d_out, nseg * 32 * sizeof(uint64_t), "d_out"))) return rc;
    if (d_high && (rc = fsint::check_extent(d_high, nseg * sizeof(uint64_t), "d_high"))) return rc;
    for (int i = 0; i < inputs; ++i)
        if ((rc = fsint::check_extent(in[i].p, in[i].bytes, in[i].name))) return rc;
    FS_HIP_TRY(fsk_launch_segments_wide(d_array, elem_bytes, 0, n, d_offsets, nseg, d_out, d_high, flags & 3, grid, call.s));
    return 0;
}

int FLAGSTATS_hip_device_wide_segments_sync(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg,
                                            uint64_t* out, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = segw_args(d_array, n, elem_bytes, offsets, nseg, out, flags, "NULL offsets or out with nseg > 0");
    if (rc || nseg == 0) return rc;
    Engine* ep = nullptr;
    if (n) {
        int dev = -1;
        if ((rc = fsint::device_of_pointer(d_array, "d_array", &dev))) return rc;
        ep = fsint::engine_for_device(dev);
    } else {
        ep = fsint::default_engine();
    }
    if (!ep) return -1;
    Engine& e = *ep;
    std::lock_guard<std::mutex> lk(e.mu);
    if (fsint::engine_alive(e)) return -1;
    DeviceGuard guard(e.device);
    if (!guard.ok()) return -1;
    const uint32_t grid = seg_grid(e);
    if ((rc = segw_fits(d_array, n, elem_bytes, grid))) return rc;
    fsseg::SegBuffers buf;     // rows, then the masks
    fsseg::HostRows got;
    if ((rc = buf.alloc(nseg, 33)) || (rc = got.alloc(nseg, 33))) return rc;
    if ((rc = fsseg::check_host_offsets(offsets, nseg, n))) return rc;
    if (n && (rc = fsint::check_extent(d_array, n * static_cast<uint64_t>(elem_bytes), "d_array"))) return rc;
    hipStream_t s = e.stream[0];
    FS_HIP_TRY(hipMemcpyAsync(buf.off, offsets, (nseg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    FS_HIP_TRY(fsk_launch_segments_wide(d_array, elem_bytes, 0, n, buf.off, nseg, buf.cnt, buf.cnt + nseg * 32, 1 | (flags & 2), grid, s));
    FS_HIP_TRY(hipMemcpyAsync(got.p.get(), buf.cnt, got.words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    FS_HIP_TRY(hipStreamSynchronize(s));
    apply_rows_and_masks(out, high, got, nseg, flags);
    return 0;
}

int FLAGSTATS_hip_wide_x64_segments(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg, uint64_t* out,
                                    uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = segw_args(array, n, elem_bytes, offsets, nseg, out, flags, "NULL offsets or out with nseg > 0");
    if (rc || nseg == 0) return rc;
    Engine* ep = fsint::default_engine();
    if (!ep) return -1;
    Engine& e = *ep;
    std::lock_guard<std::mutex> lk(e.mu);
    if (fsint::engine_alive(e)) return -1;
    DeviceGuard guard(e.device);
    if (!guard.ok()) return -1;
    fsint::lz4_gpu_other_use(e);
    fsseg::SegBuffers buf;     // rows, then the masks
    fsseg::HostRows got;
    if ((rc = buf.alloc(nseg, 33)) || (rc = got.alloc(nseg, 33))) return rc;
    if ((rc = fsseg::check_host_offsets(offsets, nseg, n))) return rc;
    if ((rc = fsint::engine_second(e))) return rc;
    // only the elements some segment covers cross the bus, as they are: [offsets[0], offsets[nseg]) in chunks of "chunk_flags" * 2
    // bytes (the wide host entry's), alternating between the engine's two streams and staging buffers; every chunk's launch adds
    // the pieces of the segments it holds to the same device rows and ORs into the same device masks
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const uint64_t chunk = fsdrv::chunk_flags() * 2 / W;   // elements per chunk (at least 2)
    const uint64_t first = offsets[0], last = offsets[nseg];
    const uint64_t cap = last - first < chunk ? (last - first ? last - first : 1) : chunk;   // elements of the largest chunk
    const int slots = last - first > chunk ? 2 : 1;
    for (int i = 0; i < slots; ++i)
        if ((rc = fsint::stage_reserve(e, i, cap * W / 2))) return rc;
    hipStream_t s0 = e.stream[0];
    FS_HIP_TRY(hipMemsetAsync(buf.cnt, 0, nseg * 33 * sizeof(uint64_t), s0));
    FS_HIP_TRY(hipMemcpyAsync(buf.off, offsets, (nseg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s0));
    if (slots == 2 && (rc = fsint::stream_wait_stream(e, e.stream[1], s0))) return rc;
    const uint32_t grid = seg_grid(e);
    const int mode = flags & 2;
    const uint8_t* src = static_cast<const uint8_t*>(array);
    uint64_t k = 0;
    for (uint64_t pos = first; pos < last; pos += chunk, ++k) {
        const int sl = static_cast<int>(k % static_cast<uint64_t>(slots));
        const uint64_t c = last - pos < chunk ? last - pos : chunk;
        FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], src + pos * W, c * W, hipMemcpyHostToDevice, e.stream[sl]));
        FS_HIP_TRY(fsk_launch_segments_wide(e.stage[sl], elem_bytes, pos, c, buf.off, nseg, buf.cnt, buf.cnt + nseg * 32, mode, grid,
                                            e.stream[sl]));
    }
    if (slots == 2 && (rc = fsint::stream_wait_stream(e, s0, e.stream[1]))) return rc;
    FS_HIP_TRY(hipMemcpyAsync(got.p.get(), buf.cnt, got.words * sizeof(uint64_t), hipMemcpyDeviceToHost, s0));
    FS_HIP_TRY(hipStreamSynchronize(s0));
    if (slots == 2) FS_HIP_TRY(hipStreamSynchronize(e.stream[1]));
    apply_rows_and_masks(out, high, got, nseg, flags);
    return 0;
}

}  // extern "C"
