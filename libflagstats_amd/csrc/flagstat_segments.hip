// flagstat_segments.hip -- segmented flagstat: one row of 32 counters per CSR segment of a uint16 FLAG array, in one launch.
//
// Work split.  The flags are addressed on the 16-byte grid of the array's aligned-down base (as K1 does) and cut into units of
// 4096 flags (8 KiB: 8 rows of 512 flags, one 16-byte vector per lane and row, so every load instruction of a wave covers 1 KiB
// contiguously).  Every wave of the grid owns one contiguous run of units -- a writer -- and walks the segments that intersect
// it: it finds the first one with a 64-ary search over the offsets (one load per lane and round), then walks forward through
// a window of 64 offsets held one per lane.  Each wave counts into the bit-sliced lane state of K1 (flagstat_count_core.h) and,
// whenever a segment ends or its range does, reduces the lane counters over the wave (DPP), maps the 21 totals to the 32 slots
// and adds them to out[seg][32] with relaxed agent-scope atomics (K1's direct epilogue, per segment).  No workspace, no second
// kernel.  A segment that lies entirely inside one writer's range is stored with plain stores in the store form (which zeroes
// out[] in front, so empty segments and never-written slots read 0).
//
// Two regimes, chosen per stretch:
//   * a run of at least `min_units` whole units inside one segment goes through K1's carry-save chain with K1's rolling load
//     schedule (6 vectors in flight per lane): the shared tree_step, end_step and reissue of flagstat_count_core.h; the
//     chain is flushed (exact at any step count) when the segment ends;
//   * every other unit -- a segment's ragged head and tail, and units dense with boundaries -- is loaded once (8 vectors in
//     flight) and counted per flag: front4's bytes are popcounted into the lane counters, one piece of the unit per segment it
//     holds (lanes and flags outside the piece read as zero, which counts nothing), and the wave reduction runs once per
//     segment end, not per flag or per row.
// The threshold is measured (tests/perf/segments_sweep.py).
//
// The walk itself (seg_walk<UE>), the emission (seg_emit<COUNT, MASK>) and the bodies of the three entry forms are
// flagstat_segments_shared.h's, for all five segmented kernels; this unit holds what is its own: the chain step, the masked
// per-flag count of a piece, the policy and the launcher.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_engine.h"
#include "flagstat_segments.h"
#include "flagstat_segments_shared.h"

namespace fsk {

constexpr int kSegDepth = 8;                       // chain depth as K1: epochs of 255 units

// K1's step at the default schedule (schedule 71 with non-temporal loads, each wave a contiguous 8 KiB): vector u's registers are
// re-issued for vector u + 6 of the same unit (`cur`) or u - 2 of the next (`next`, if HAS_NEXT).
template <bool HAS_NEXT>
__device__ __forceinline__ void seg_step_and_count(Lane<kSegDepth>& s, uint4 (&v)[kUnroll], uint32_t& blk, const uint4* cur,
                                                   const uint4* next)
{
    blk = __builtin_amdgcn_readfirstlane(blk);
    tree_step<kSegDepth>(s, blk, [&](int uu, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        split_out(v[uu], L0, H0, L1, H1);
        reissue<HAS_NEXT ? 1 : 2>(uu, v, cur, next, kSegRowVecs, load_vec<true>);
        __builtin_amdgcn_sched_barrier(0);
    });
    end_step<kSegDepth>(s, blk);
}

// the flags of vector x (grid positions q .. q+7) that lie in [b, e); the others become 0
__device__ __forceinline__ uint4 mask_vec(uint4 x, uint64_t q, uint64_t b, uint64_t e)
{
    const uint32_t lk = b > q ? static_cast<uint32_t>(b - q < 8 ? b - q : 8) : 0u;  // first kept element
    const uint32_t hk = e > q ? static_cast<uint32_t>(e - q < 8 ? e - q : 8) : 0u;  // one past the last
    auto keep = [&](uint32_t k) { return k >= lk && k < hk; };
    x.x &= (keep(0) ? 0xFFFFu : 0u) | (keep(1) ? 0xFFFF0000u : 0u);
    x.y &= (keep(2) ? 0xFFFFu : 0u) | (keep(3) ? 0xFFFF0000u : 0u);
    x.z &= (keep(4) ? 0xFFFFu : 0u) | (keep(5) ? 0xFFFF0000u : 0u);
    x.w &= (keep(6) ? 0xFFFFu : 0u) | (keep(7) ? 0xFFFF0000u : 0u);
    return x;
}

// the piece [b, e) of the unit starting at grid position w0 (its 8 rows in v[]) into the lane counters
__device__ __forceinline__ void count_piece(uint32_t (&acc)[kInternal], const uint4 (&v)[kUnroll], uint64_t w0, uint64_t b,
                                            uint64_t e, uint32_t lane)
{
#pragma unroll
    for (int r = 0; r < kUnroll; ++r) {
        const uint64_t r0 = w0 + static_cast<uint64_t>(r) * 512u;
        if (r0 + 512u <= b || r0 >= e) continue;  // wave-uniform
        if (r0 >= b && r0 + 512u <= e)
            count8(acc, v[r]);
        else
            count8(acc, mask_vec(v[r], r0 + 8u * lane, b, e));
    }
}

// a0: 16-B aligned-down base; the chunk's flags occupy grid positions [lo0, hi0) and are global flags [base, base + hi0 - lo0).
// nunits = ceil(hi0 / 4096).  mode: bit 0 store form (out[] zeroed in front), bit 1 superset.
__global__ __launch_bounds__(kThreads) void flagstat_segments(const uint4* __restrict__ a0, uint64_t lo0, uint64_t hi0, uint64_t base,
                                                              const uint64_t* __restrict__ off, uint64_t nseg,
                                                              uint64_t* __restrict__ out, int mode, uint64_t nunits,
                                                              uint32_t min_units)
{
    __shared__ uint32_t red_all[kThreads / 64][24];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* red = red_all[threadIdx.x >> 6];
    Lane<kSegDepth> st;
    lane_init(st);
    uint32_t blk = 0;
    uint32_t none = 0;  // neither a passing count nor a mask
    uint4 v[kUnroll];
    seg_walk<kSegWaveFlags>(
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
                seg_step_and_count<true>(st, v, blk, p, pn);
                p = pn;
            }
            seg_step_and_count<false>(st, v, blk, p, nullptr);
        },
        [&](uint64_t u, bool whole) __attribute__((always_inline)) {
            const uint64_t j0 = u * kSegUnitVecs + lane;
            if (whole) {
#pragma unroll
                for (int r = 0; r < kUnroll; ++r) v[r] = load_vec<true>(a0 + j0 + r * kSegRowVecs);
            } else {
#pragma unroll
                for (int r = 0; r < kUnroll; ++r) v[r] = load_guarded(a0, j0 + r * kSegRowVecs, lo0, hi0);
            }
        },
        [&](uint64_t w0, uint64_t b, uint64_t e) __attribute__((always_inline)) { count_piece(st.acc, v, w0, b, e, lane); },
        [&](uint64_t s, uint64_t len, bool plain) __attribute__((always_inline)) {
            seg_emit<false, false>(st, blk, none, none, none, red, out, nullptr, nullptr, s, len, plain, mode, lane);
        });
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
static std::atomic<uint32_t> g_seg_min_units{2};      // whole units in one segment from which the chain pays
static std::atomic<uint32_t> g_seg_blocks_per_cu{1};

extern "C" void fsk_segments_policy(uint32_t* min_units, uint32_t* blocks_per_cu)
{
    *min_units = g_seg_min_units.load();
    *blocks_per_cu = g_seg_blocks_per_cu.load();
}

extern "C" void fsk_set_segments_policy(uint32_t min_units, uint32_t blocks_per_cu)
{
    g_seg_min_units = min_units;
    g_seg_blocks_per_cu = blocks_per_cu < 1 ? 1 : (blocks_per_cu > 8 ? 8 : blocks_per_cu);
}

extern "C" hipError_t fsk_launch_segments(const uint16_t* d_chunk, uint64_t base, uint64_t m, const uint64_t* d_offsets, uint64_t nseg,
                                          uint64_t* d_out, int mode, uint32_t grid, hipStream_t stream)
{
    if (nseg == 0) return hipSuccess;
    if (d_out == nullptr || d_offsets == nullptr || grid == 0 || (m && d_chunk == nullptr)) return hipErrorInvalidValue;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_chunk);
    if (addr & 1u) return hipErrorInvalidValue;
    if (mode & 1) {
        const hipError_t e = fsk_zero_words(d_out, nseg * 32, stream);
        if (e != hipSuccess) return e;
    }
    if (m == 0) return hipSuccess;
    uint64_t lo0 = 0, nunits = 0;
    uint32_t g = 0;
    fsseg::launch_shape(addr, m, fsk::kSegWaveFlags, grid, &lo0, &nunits, &g);   // no fit check: the limit is flagstat_segments.h's
    const uintptr_t a0 = addr & ~static_cast<uintptr_t>(15);
    hipLaunchKernelGGL(fsk::flagstat_segments, dim3(g), dim3(fsk::kThreads), 0, stream, reinterpret_cast<const uint4*>(a0), lo0, lo0 + m,
                       base, d_offsets, nseg, d_out, mode & 3, nunits, g_seg_min_units.load());
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The bodies of the three forms are fsseg's (flagstat_segments_shared.h); this unit has no trailing word and no fit check.
using fsint::Engine;
using fsint::fail_text;

extern "C" {

int FLAGSTATS_hip_device_u16_segments(const uint16_t* d_array, uint64_t n, const uint64_t* d_offsets, uint64_t nseg, uint64_t* d_out,
                                      int flags, void* stream)
{
    FS_ENTRY();
    if (fsdrv::check_flags(flags)) return -1;
    if (nseg == 0) return 0;
    // this entry asks for the array before it looks at nseg, and words the latter its own way
    if (!d_offsets || !d_out) return fail_text(fsseg::kNullDevice);
    if (fsdrv::check_array_given(d_array, n)) return -1;
    if (nseg > fsseg::kMaxSegments) return fail_text("nseg is too large for its counters to be a size");
    if (fsdrv::check_array_aligned(d_array, 2)) return -1;
    fsdrv::Inputs in = fsseg::offsets_input(d_offsets, nseg);
    in.add_columns(d_array, n, 2, nullptr, 0, 0, nullptr, 0);
    return fsseg::device_call(d_out, nullptr, 0, in.in, in.count, nseg, stream, [](uint32_t) { return 0; },
                              [&](uint32_t grid, hipStream_t s) {
                                  FS_HIP_TRY(fsk_launch_segments(d_array, 0, n, d_offsets, nseg, d_out, flags & 3, grid, s));
                                  return 0;
                              });
}

int FLAGSTATS_hip_device_u16_segments_sync(const uint16_t* d_array, uint64_t n, const uint64_t* offsets, uint64_t nseg, uint64_t* out,
                                           int flags)
{
    FS_ENTRY();
    if (fsdrv::check_flags(flags)) return -1;
    if (nseg == 0) return 0;
    if (fsseg::check_segments(offsets, out, nseg, fsseg::kNullHost, fsseg::kMaxSegments) || fsdrv::check_array_given(d_array, n) ||
        fsdrv::check_array_aligned(d_array, 2))
        return -1;
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, nullptr, 0, 0, nullptr, 0);
    return fsseg::sync_call(
        in.in, in.count, n, offsets, nseg, 32, [](uint32_t) { return 0; },
        [&](fsseg::SegBuffers& buf, uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments(d_array, 0, n, buf.off, nseg, buf.cnt, 1 | (flags & 2), grid, s));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply(out, got.p.get(), got.words, flags); });
}

int FLAGSTATS_hip_u16_x64_segments(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg, uint64_t* out, int flags)
{
    FS_ENTRY();
    if (fsdrv::check_flags(flags)) return -1;
    if (nseg == 0) return 0;
    if (fsseg::check_segments(offsets, out, nseg, fsseg::kNullHost, fsseg::kMaxSegments) || fsdrv::check_array_given(array, n)) return -1;
    const int mode = flags & 2;
    return fsseg::host_call(
        n, offsets, nseg, 32, fsdrv::chunk_flags(), [&] { return offsets[nseg]; }, [](uint64_t cap) { return cap; },
        [&](Engine& e, fsseg::SegBuffers& buf, int sl, uint64_t pos, uint64_t c, uint64_t, uint32_t grid) {
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], array + pos, c * sizeof(uint16_t), hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_segments(e.stage[sl], pos, c, buf.off, nseg, buf.cnt, mode, grid, e.stream[sl]));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply(out, got.p.get(), got.words, flags); });
}

}  // extern "C"
