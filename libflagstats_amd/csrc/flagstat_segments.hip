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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <mutex>

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

// the wave's counters of the piece of segment s it holds -> out[s][32]
__device__ __forceinline__ void seg_emit(Lane<kSegDepth>& st, uint32_t& blk, uint32_t* red, uint64_t* __restrict__ out, uint64_t s,
                                         uint64_t len, bool plain, int mode, uint32_t lane)
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
    if (lane == 63) {
#pragma unroll
        for (int c = 0; c < kInternal; ++c) red[c] = w[c];
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
    }
    __builtin_amdgcn_wave_barrier();  // red[] is rewritten by the next segment's totals only after every lane has read it
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
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kThreads / 64);
    const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * (kThreads / 64) + wave;
    const uint64_t u_begin = gw * nunits / waves, u_end = (gw + 1) * nunits / waves;
    const uint64_t p0 = u_begin * kSegWaveFlags > lo0 ? u_begin * kSegWaveFlags : lo0;  // this writer: grid positions [p0, E)
    const uint64_t E = u_end * kSegWaveFlags < hi0 ? u_end * kSegWaveFlags : hi0;
    if (p0 >= E) return;
    uint32_t* red = red_all[wave];

    SegWalk sw{off, nseg, base, hi0 - lo0, lo0, lane, 0, 0, 0};
    uint64_t s = sw.first_segment(p0);
    if (s >= nseg) return;
    sw.load_window(s);

    Lane<kSegDepth> st;
    lane_init(st);
    uint32_t blk = 0;
    bool open = false;  // st holds counts of segment s not yet emitted
    uint64_t sb = 0, se = 0;
    auto emit = [&](uint64_t seg, uint64_t b_, uint64_t e_) {
        const uint64_t pb = b_ > p0 ? b_ : p0, pe = e_ < E ? e_ : E;
        seg_emit(st, blk, red, out, seg, pe - pb, (mode & 1) && b_ >= p0 && e_ <= E, mode, lane);
    };

    uint64_t u = p0 / kSegWaveFlags;
    while (s < nseg && u < u_end) {
        sw.bounds(s, sb, se);
        const uint64_t w0 = u * kSegWaveFlags;
        const uint64_t x = w0 > p0 ? w0 : p0;
        // A segment that begins at or past this writer's end is not its business, nor (monotone offsets) is any later one.  This
        // test comes first: a launch on one chunk of a longer array (the host form) clamps every later segment to an empty one
        // at the chunk's end, and stepping through those one by one would cost the chunk's last writer O(nseg) per launch.
        if (sb >= E) break;
        if (se <= sb || se <= x) {  // empty (or, with malformed offsets, reversed or behind)
            ++s;
            continue;
        }
        if (sb >= w0 + kSegWaveFlags) {  // flags before the segment belong to none: skip whole units unread
            u = sb / kSegWaveFlags;
            continue;
        }
        const uint64_t seg_e = se < E ? se : E;
        if (sb <= w0 && w0 >= lo0) {
            const uint64_t k = (seg_e - w0) / kSegWaveFlags;  // whole units of segment s from here on
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
                    seg_step_and_count<true>(st, v, blk, p, pn);
                    p = pn;
                }
                seg_step_and_count<false>(st, v, blk, p, nullptr);
                u += k;
                open = true;
                if (u * kSegWaveFlags >= se) {
                    emit(s, sb, se);
                    open = false;
                    ++s;
                }
                continue;
            }
        }
        // per-flag unit: its 8 rows loaded at once, then every segment piece in it
        uint4 v[kUnroll];
        const uint64_t j0 = u * kSegUnitVecs + lane;
        if (w0 >= lo0 && w0 + kSegWaveFlags <= hi0) {
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) v[r] = load_vec<true>(a0 + j0 + r * kSegRowVecs);
        } else {
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) v[r] = load_guarded(a0, j0 + r * kSegRowVecs, lo0, hi0);
        }
        const uint64_t w1 = w0 + kSegWaveFlags;
        uint64_t xx = x;
        for (;;) {
            // s < nseg, sb < se, se > xx, sb < w1
            const uint64_t b = sb > xx ? sb : xx, e = se < w1 ? se : w1;
            count_piece(st.acc, v, w0, b, e, lane);
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
    const uintptr_t a0 = addr & ~static_cast<uintptr_t>(15);
    const uint64_t lo0 = (addr - a0) / 2, hi0 = lo0 + m;
    const uint64_t nunits = (hi0 + fsk::kSegWaveFlags - 1) / fsk::kSegWaveFlags;
    const uint64_t want = (nunits + 3) / 4;  // one unit per wave at least
    const uint32_t g = want < grid ? static_cast<uint32_t>(want) : grid;
    hipLaunchKernelGGL(fsk::flagstat_segments, dim3(g), dim3(fsk::kThreads), 0, stream, reinterpret_cast<const uint4*>(a0), lo0, hi0,
                       base, d_offsets, nseg, d_out, mode & 3, nunits, g_seg_min_units.load());
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
using fsint::DeviceGuard;
using fsint::Engine;
using fsint::fail_hip;
using fsint::fail_text;

using fsseg::apply;
using fsseg::check_host_offsets;
using fsseg::host_args;
using fsseg::HostRows;
using fsseg::kMaxSegments;
using fsseg::SegBuffers;
using fsseg::seg_grid;

extern "C" {

int FLAGSTATS_hip_device_u16_segments(const uint16_t* d_array, uint64_t n, const uint64_t* d_offsets, uint64_t nseg, uint64_t* d_out,
                                      int flags, void* stream)
{
    FS_ENTRY();
    if (flags & ~3) return fail_text("flags: bit 0 store, bit 1 superset; no other bits");
    if (nseg == 0) return 0;
    if (!d_offsets || !d_out) return fail_text("NULL d_offsets or d_out with nseg > 0");
    if (n && !d_array) return fail_text("NULL array with n > 0");
    if (nseg > kMaxSegments) return fail_text("nseg is too large for its counters to be a size");
    if (reinterpret_cast<uintptr_t>(d_array) & 1u) return fail_text("array must be 2-byte aligned");
    int dev_out = -1, dev = -1;
    bool plain = false;
    int rc = fsint::device_of_pointer(d_out, "d_out", &dev_out, &plain);
    if (rc) return rc;
    if (!plain) return fail_text("d_out must be device memory (the counters are added with device atomics)");
    rc = fsint::device_of_pointer(d_offsets, "d_offsets", &dev);
    if (rc) return rc;
    if (dev != dev_out) return fail_text("d_offsets and d_out live on different devices");
    if (n) {
        rc = fsint::device_of_pointer(d_array, "d_array", &dev);
        if (rc) return rc;
        if (dev != dev_out) return fail_text("d_array and d_out live on different devices");
    }
    Engine* e = fsint::engine_for_device(dev_out);
    if (!e) return -1;
    DeviceGuard guard(e->device);
    if (!guard.ok()) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = fsint::check_stream_device(s, e->device);
    if (rc) return rc;
    if ((rc = fsint::check_extent(d_out, nseg * 32 * sizeof(uint64_t), "d_out")) || (rc = fsint::check_extent(d_offsets, (nseg + 1) * sizeof(uint64_t), "d_offsets")))
        return rc;
    if (n && (rc = fsint::check_extent(d_array, n * sizeof(uint16_t), "d_array"))) return rc;
    FS_HIP_TRY(fsk_launch_segments(d_array, 0, n, d_offsets, nseg, d_out, flags & 3, seg_grid(*e), s));
    return 0;
}

int FLAGSTATS_hip_device_u16_segments_sync(const uint16_t* d_array, uint64_t n, const uint64_t* offsets, uint64_t nseg, uint64_t* out,
                                           int flags)
{
    FS_ENTRY();
    if (flags & ~3) return fail_text("flags: bit 0 store, bit 1 superset; no other bits");
    if (nseg == 0) return 0;
    int rc = host_args(offsets, nseg, out);
    if (rc) return rc;
    if (n && !d_array) return fail_text("NULL array with n > 0");
    if (reinterpret_cast<uintptr_t>(d_array) & 1u) return fail_text("array must be 2-byte aligned");
    Engine* ep = nullptr;
    if (n) {
        int dev = -1;
        rc = fsint::device_of_pointer(d_array, "d_array", &dev);
        if (rc) return rc;
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
    SegBuffers buf;
    HostRows got;
    if ((rc = buf.alloc(nseg)) || (rc = got.alloc(nseg))) return rc;
    if ((rc = check_host_offsets(offsets, nseg, n))) return rc;
    if (n && (rc = fsint::check_extent(d_array, n * sizeof(uint16_t), "d_array"))) return rc;
    hipStream_t s = e.stream[0];
    FS_HIP_TRY(hipMemcpyAsync(buf.off, offsets, (nseg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    FS_HIP_TRY(fsk_launch_segments(d_array, 0, n, buf.off, nseg, buf.cnt, 1 | (flags & 2), seg_grid(e), s));
    FS_HIP_TRY(hipMemcpyAsync(got.p.get(), buf.cnt, got.words * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    FS_HIP_TRY(hipStreamSynchronize(s));
    apply(out, got.p.get(), got.words, flags);
    return 0;
}

int FLAGSTATS_hip_u16_x64_segments(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg, uint64_t* out, int flags)
{
    FS_ENTRY();
    if (flags & ~3) return fail_text("flags: bit 0 store, bit 1 superset; no other bits");
    if (nseg == 0) return 0;
    int rc = host_args(offsets, nseg, out);
    if (rc) return rc;
    if (n && !array) return fail_text("NULL array with n > 0");
    Engine* ep = fsint::default_engine();
    if (!ep) return -1;
    Engine& e = *ep;
    std::lock_guard<std::mutex> lk(e.mu);
    if (fsint::engine_alive(e)) return -1;
    DeviceGuard guard(e.device);
    if (!guard.ok()) return -1;
    fsint::lz4_gpu_other_use(e);
    SegBuffers buf;
    HostRows got;
    if ((rc = buf.alloc(nseg)) || (rc = got.alloc(nseg))) return rc;
    if ((rc = check_host_offsets(offsets, nseg, n))) return rc;
    if ((rc = fsint::engine_second(e))) return rc;
    // only the flags some segment covers cross the bus: [offsets[0], offsets[nseg]) in chunks of "chunk_flags", alternating
    // between the engine's two streams and staging buffers (the copy of chunk k + 1 overlaps the kernel on chunk k); every
    // chunk's launch adds the pieces of the segments it holds to the same device counters
    const uint64_t chunk = fsint::knobs().chunk_flags.load() < 8 ? 8 : fsint::knobs().chunk_flags.load();
    const uint64_t first = offsets[0], last = offsets[nseg];
    const int slots = last - first > chunk ? 2 : 1;
    for (int i = 0; i < slots; ++i)
        if ((rc = fsint::stage_reserve(e, i, last - first < chunk ? (last - first ? last - first : 1) : chunk))) return rc;
    hipStream_t s0 = e.stream[0];
    FS_HIP_TRY(hipMemsetAsync(buf.cnt, 0, nseg * 32 * sizeof(uint64_t), s0));
    FS_HIP_TRY(hipMemcpyAsync(buf.off, offsets, (nseg + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s0));
    if (slots == 2 && (rc = fsint::stream_wait_stream(e, e.stream[1], s0))) return rc;
    const uint32_t grid = seg_grid(e);
    const int mode = flags & 2;
    uint64_t k = 0;
    for (uint64_t pos = first; pos < last; pos += chunk, ++k) {
        const int sl = static_cast<int>(k % static_cast<uint64_t>(slots));
        const uint64_t c = last - pos < chunk ? last - pos : chunk;
        FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], array + pos, c * sizeof(uint16_t), hipMemcpyHostToDevice, e.stream[sl]));
        FS_HIP_TRY(fsk_launch_segments(e.stage[sl], pos, c, buf.off, nseg, buf.cnt, mode, grid, e.stream[sl]));
    }
    if (slots == 2 && (rc = fsint::stream_wait_stream(e, s0, e.stream[1]))) return rc;
    FS_HIP_TRY(hipMemcpyAsync(got.p.get(), buf.cnt, got.words * sizeof(uint64_t), hipMemcpyDeviceToHost, s0));
    FS_HIP_TRY(hipStreamSynchronize(s0));
    if (slots == 2) FS_HIP_TRY(hipStreamSynchronize(e.stream[1]));
    apply(out, got.p.get(), got.words, flags);
    return 0;
}

}  // extern "C"
