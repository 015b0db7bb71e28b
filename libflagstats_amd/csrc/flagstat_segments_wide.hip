// flagstat_segments_wide.hip -- segmented flagstat of a FLAG array held as 4-byte or 8-byte little-endian integers (int32 / int64
// columns), read in place: one row of 32 counters per CSR segment, counted from the low 16 bits of its elements exactly as the
// uint16 segmented kernel counts them, and per segment the OR of every bit above bit 15 that one of ITS elements carries, in one
// launch.  The segmented kernels' work split, walk and emission (seg_walk<UE> and seg_emit<false, true> of
// flagstat_segments_shared.h) over the wide kernel's read-out of an element (flagstat_wide.hip).
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
    uint32_t* red = red_all[threadIdx.x >> 6];
    Lane<kSegWideDepth> st;
    lane_init(st);
    uint32_t blk = 0;
    uint32_t or_even = 0, or_odd = 0;   // dwords of the open segment's elements
    uint32_t none = 0;                  // no passing count
    uint4 v[kUnroll];
    seg_walk<UE>(
        lo0, hi0, base, off, nseg, mode, nunits, min_units,
        [&](uint64_t u, uint64_t k) __attribute__((always_inline)) {
            const uint4* p = a0 + u * kSegUnitVecs + lane;
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
        },
        [&](uint64_t u, bool whole) __attribute__((always_inline)) {
            const uint64_t j0 = u * kSegUnitVecs + lane;
            if (whole) {
#pragma unroll
                for (int r = 0; r < kUnroll; ++r) v[r] = load_vec<true>(a0 + j0 + r * kSegRowVecs);
            } else {
#pragma unroll
                for (int r = 0; r < kUnroll; ++r) v[r] = load_guarded_wide<W>(a0, j0 + r * kSegRowVecs, lo0, hi0);
            }
        },
        [&](uint64_t w0, uint64_t b, uint64_t e) __attribute__((always_inline)) {
            count_piece_wide<W>(st.acc, or_even, or_odd, v, w0, b, e, lane);
        },
        [&](uint64_t s, uint64_t len, bool plain) __attribute__((always_inline)) {
            seg_emit<false, true>(st, blk, none, or_even, or_odd, red, out, nullptr, high, s, len, plain, mode, lane);
        });
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
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
        fsseg::launch_shape(addr, m, fsk::kSegWideUnitBytes / W, grid, &lo0, &nunits, &g);
        if (!fsseg::wave_totals_fit(nunits, g, fsk::kSegWideUnitBytes / W)) return hipErrorInvalidValue;
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
// The bodies of the three forms are fsseg's (flagstat_segments_shared.h): 33 words per segment, the rows, then the masks.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU (nseg > 0 from the NULL checks on)
int segw_args(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg, const void* out, int flags,
              const char* null_text)
{
    using namespace fsdrv;
    if (check_elem_bytes(elem_bytes, "elem_bytes 2: 16-bit arrays go to the u16 entries (FLAGSTATS_hip_u16_x64_segments, "
                                     "FLAGSTATS_hip_device_u16_segments)") ||
        check_flags(flags))
        return -1;
    if (nseg == 0) return 0;
    return refused(fsseg::check_segments(offsets, out, nseg, null_text, fsseg::kMaxSegments / 2) || check_array_given(array, n) ||
                   check_array_layout(array, n, elem_bytes));
}

// rows, then masks, of a synchronous call into the caller's host words: rows stored or added, masks stored or ORed
void apply_rows_and_masks(uint64_t* out, uint64_t* high, const fsseg::HostRows& got, uint64_t nseg, int flags)
{
    fsseg::apply(out, got.p.get(), nseg * 32, flags);
    fsseg::apply_masks(high, got.p.get() + nseg * 32, nseg, flags);
}

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_wide_segments(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* d_offsets, uint64_t nseg,
                                       uint64_t* d_out, uint64_t* d_high, int flags, void* stream)
{
    FS_ENTRY();
    int rc = segw_args(d_array, n, elem_bytes, d_offsets, nseg, d_out, flags, fsseg::kNullDevice);
    if (rc || nseg == 0) return rc;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const fsdrv::DeviceWord word{d_high, "d_high", "the masks are ORed with device atomics"};
    fsdrv::Inputs in = fsseg::offsets_input(d_offsets, nseg);
    in.add_columns(d_array, n, W, nullptr, 0, 0, nullptr, 0);
    return fsseg::device_call(
        d_out, &word, 1, in.in, in.count, nseg, stream,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWideUnitBytes / W, grid); },
        [&](uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_wide(d_array, elem_bytes, 0, n, d_offsets, nseg, d_out, d_high, flags & 3, grid, s));
            return 0;
        });
}

int FLAGSTATS_hip_device_wide_segments_sync(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg,
                                            uint64_t* out, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = segw_args(d_array, n, elem_bytes, offsets, nseg, out, flags, fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    fsdrv::Inputs in;
    in.add_columns(d_array, n, W, nullptr, 0, 0, nullptr, 0);
    return fsseg::sync_call(
        in.in, in.count, n, offsets, nseg, 33, [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWideUnitBytes / W, grid); },
        [&](fsseg::SegBuffers& buf, uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_wide(d_array, elem_bytes, 0, n, buf.off, nseg, buf.cnt, buf.cnt + nseg * 32, 1 | (flags & 2), grid, s));
            return 0;
        },
        [&](const fsseg::HostRows& got) { apply_rows_and_masks(out, high, got, nseg, flags); });
}

int FLAGSTATS_hip_wide_x64_segments(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg, uint64_t* out,
                                    uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = segw_args(array, n, elem_bytes, offsets, nseg, out, flags, fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    // the elements cross the bus as they are, in chunks of "chunk_flags" * 2 bytes (the wide host entry's); every chunk's launch
    // adds to the same device rows and ORs into the same device masks
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const int mode = flags & 2;
    const uint8_t* src = static_cast<const uint8_t*>(array);
    return fsseg::host_call(
        n, offsets, nseg, 33, fsdrv::chunk_flags() * 2 / W, [&] { return offsets[nseg]; }, [&](uint64_t cap) { return cap * W / 2; },
        [&](Engine& e, fsseg::SegBuffers& buf, int sl, uint64_t pos, uint64_t c, uint64_t, uint32_t grid) {
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], src + pos * W, c * W, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_segments_wide(e.stage[sl], elem_bytes, pos, c, buf.off, nseg, buf.cnt, buf.cnt + nseg * 32, mode, grid,
                                                e.stream[sl]));
            return 0;
        },
        [&](const fsseg::HostRows& got) { apply_rows_and_masks(out, high, got, nseg, flags); });
}

}  // extern "C"
