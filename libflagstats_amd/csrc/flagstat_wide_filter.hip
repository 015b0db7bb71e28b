// flagstat_wide_filter.hip -- flagstat of the elements of a FLAG array held as 4-byte or 8-byte little-endian integers (int32 /
// int64 columns, read in place) that pass samtools' view filter.  With f(i) = element[i] & 0xFFFF and
//   pass(i) = (f(i) & require) == require && (f(i) & exclude) == 0 && (min_mapq == 0 || mapq[i] >= min_mapq)
// one kernel gives the 32 counters of {f(i) : pass(i)}, the number of i that pass, and the OR of element[i] & ~0xFFFF over ALL
// elements -- passing or not: the mask says whether the column is a FLAG column, the predicate sees the low 16 bits only.
//
// It is the wide kernel's walk (flagstat_wide.hip: geometry, narrowing to the byte planes (L, H) of 4 flags, the short tree with
// one weight-16 push per step, the mask accumulators; the pieces are flagstat_wide_device.h's, and what the segmented filtered
// kernel shares with this one -- the MAPQ loaders, valid_bits_wide and the step itself -- is flagstat_wide_filter_device.h's) with the filter kernel's predicate
// (flagstat_filter.hip, where the test is derived; pass4 of flagstat_filter_device.h) in front of front4: the flags that fail
// are zeroed on their planes, a zero flag counts nothing.  The mask is ORed from every loaded dword by narrow_out, in front of
// the predicate, exactly as in the wide kernel.
//
// MAPQ.  The launcher hands the kernel `mq` such that the byte of grid position q (an element of W bytes) is mq[q], at any
// alignment; vector j holds positions [j * 16 / W, (j + 1) * 16 / W).
//   W = 4: a vector is one (L, H) group, its MAPQ one unaligned dword at mq + 4 j.
//   W = 8: a group is the even dwords of vectors u and u + 1 of a lane, which lie 64 vectors = 128 elements apart, so its four
//          MAPQ bytes come from two places: one unaligned 16-bit load per vector (mq + 2 j), the dword assembled with one
//          v_lshl_or_b32 when the odd vector arrives.  (Re-pairing so that the bytes are adjacent would change which vectors a
//          lane loads, i.e. the wide kernel's walk and its coalescing; a 16-bit load costs the same issue slot as a dword load
//          and there are exactly as many of them as vectors either way.)
// On fast steps the MAPQ load of a vector is issued with the vector (reissue, schedule 71); all its positions are elements then.
// On edge steps MAPQ is read byte by byte, only at positions in [lo, hi).
//
// Edge steps.  The guarded loader zero-fills positions outside [lo, hi): they set no mask bit and count nothing, but a zero flag
// passes every predicate without `require` bits and would be counted in `selected`: their pass bits are cleared (valid bits of
// the vector's 4 or 2 positions, spread to bit 7 of the group's bytes with nibble_to_bit7).
//
// Epilogue.  The wide kernel's and the filter kernel's in one: finalize_slots<true> with the workgroup's `selected` entering
// slot 9 (superset), one relaxed agent-scope atomic add for `selected` and one atomic OR for the mask.  No workspace, no second
// kernel; the store form zeroes counters, count and mask in front (one memset when they are one allocation's 34 words).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_filter_device.h"
#include "flagstat_wide.h"
#include "flagstat_wide_device.h"
#include "flagstat_wide_filter.h"
#include "flagstat_wide_filter_device.h"

namespace fsk {

constexpr int kWideFilterDepth = 8;   // chain depth as K1: epochs of 255 steps

// One step (wide_filter_step_with of flagstat_wide_filter_device.h) at this kernel's strides.
// ROLL 0 (edge steps): the vectors are in v[], their MAPQ bytes in m[], the bits of their positions that are elements in vb[].
// ROLL 1, 2: K1's schedule 71 as the wide kernel runs it; the MAPQ bytes of a vector are re-issued right in front of it.
template <int W, bool MAPQ, int ROLL>
__device__ __forceinline__ void wide_filter_step(Lane<kWideFilterDepth>& s, const FilterArgs& f, uint4 (&v)[kUnroll], uint32_t (&m)[kUnroll],
                                                 const uint32_t (&vb)[kUnroll], uint32_t blk, uint32_t& cnt, uint32_t& or_even,
                                                 uint32_t& or_odd, const uint4* __restrict__ cur, const uint4* __restrict__ next,
                                                 const uint8_t* __restrict__ mcur, const uint8_t* __restrict__ mnext)
{
    wide_filter_step_with<W, MAPQ, ROLL, kWaveStride>(s, f, v, m, vb, blk, cnt, or_even, or_odd, cur, next, mcur, mnext);
}

template <int W, bool MAPQ, int ROLL>
__device__ __forceinline__ void wide_filter_step_and_count(Lane<kWideFilterDepth>& s, const FilterArgs& f, uint4 (&v)[kUnroll],
                                                           uint32_t (&m)[kUnroll], const uint32_t (&vb)[kUnroll], uint32_t& blk,
                                                           uint32_t& cnt, uint32_t& or_even, uint32_t& or_odd,
                                                           const uint4* __restrict__ cur = nullptr, const uint4* __restrict__ next = nullptr,
                                                           const uint8_t* __restrict__ mcur = nullptr,
                                                           const uint8_t* __restrict__ mnext = nullptr)
{
    blk = __builtin_amdgcn_readfirstlane(blk);
    wide_filter_step<W, MAPQ, ROLL>(s, f, v, m, vb, blk, cnt, or_even, or_odd, cur, next, mcur, mnext);
    end_step<kWideFilterDepth>(s, blk);
}

// a0: 16-B aligned-down base; the caller's elements occupy positions [lo, hi) of its grid of W-byte elements.  mq: the MAPQ
// column on the same grid (the byte of position q is mq[q]; not read when !MAPQ).  require & exclude == 0 (the launcher's
// business), both below 2^16, min_mapq in 1..255 when MAPQ.  mode: bit 1 superset (bit 0, the store form, is the launcher's
// memset).  selected and high may each be nullptr.
template <int W, bool MAPQ>
__global__ __launch_bounds__(kThreads) void flagstat_count_wide_filter(const uint4* __restrict__ a0, const uint8_t* __restrict__ mq,
                                                                       uint32_t require, uint32_t exclude, uint32_t min_mapq, uint64_t lo,
                                                                       uint64_t hi, uint64_t nsteps, uint64_t fast_begin, uint64_t fast_end,
                                                                       uint64_t* __restrict__ out, uint64_t* __restrict__ selected,
                                                                       uint64_t* __restrict__ high, int mode)
{
    static_assert(W == 4 || W == 8, "4-byte or 8-byte elements");
    Lane<kWideFilterDepth> s;
    lane_init(s);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    constexpr int VPS = kVecPerStep;
    constexpr int US = kWaveStride;
    constexpr int EPV = 16 / W;
    const uint64_t lane_off = static_cast<uint64_t>(wave) * (US * kUnroll) + lane;
    const uint64_t G = gridDim.x;
    const FilterArgs f = filter_args_of(require, exclude, min_mapq);
    uint32_t blk = stagger_start(wave);
    uint32_t cnt = 0;                           // passing elements of this lane
    uint32_t or_even = 0, or_odd = 0;

    auto edge_step = [&](uint64_t st) {
        uint4 v[kUnroll];
        uint32_t m[kUnroll], vb[kUnroll];
        const uint64_t j0 = st * VPS + lane_off;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            v[u] = load_guarded_wide<W>(a0, j0 + u * US, lo, hi);
            vb[u] = valid_bits_wide<W>(j0 + u * US, lo, hi);
            if constexpr (MAPQ)
                m[u] = load_mapq_wide_guarded<W>(mq, j0 + u * US, lo, hi);
            else
                m[u] = 0;
        }
        wide_filter_step_and_count<W, MAPQ, 0>(s, f, v, m, vb, blk, cnt, or_even, or_odd);
    };
    // ragged edge steps (at most the first and the last of the whole array), outside the pipelined loop
    if (fast_begin != 0 && blockIdx.x == 0) edge_step(0);
    if (nsteps > fast_end && nsteps - 1 >= fast_begin && (nsteps - 1) % G == blockIdx.x) edge_step(nsteps - 1);
    // first fully in-range step of this workgroup
    uint64_t st = blockIdx.x;
    if (st < fast_begin) st += G;  // fast_begin is 0 or 1
    if (st < fast_end) {
        constexpr int RD = kRollDistance;
        uint4 v[kUnroll];
        uint32_t m[kUnroll];
        const uint32_t vb[kUnroll] = {};        // not looked at on fast steps
        const uint4* p = a0 + st * VPS + lane_off;
        const uint8_t* pm = mq + (st * VPS + lane_off) * EPV;
        // the first RD vectors; the rest is issued as they are consumed
#pragma unroll
        for (int u = 0; u < RD; ++u) {
            if constexpr (MAPQ) m[u] = load_mapq_wide<W>(pm + u * US * EPV);
            v[u] = load_vec<true>(p + u * US);
            __builtin_amdgcn_sched_barrier(0);
        }
        for (; st + G < fast_end; st += G) {
            const uint4* pn = p + G * VPS;
            const uint8_t* pmn = pm + G * VPS * EPV;
            wide_filter_step_and_count<W, MAPQ, 1>(s, f, v, m, vb, blk, cnt, or_even, or_odd, p, pn, pm, pmn);
            p = pn;
            pm = pmn;
        }
        wide_filter_step_and_count<W, MAPQ, 2>(s, f, v, m, vb, blk, cnt, or_even, or_odd, p, nullptr, pm, nullptr);
    }
    flush(s, blk);

    // wave sums and ORs on the VALU (DPP), then the 4 waves through LDS; word kInternal is the number of passing elements
    constexpr int kWaves = kThreads / 64;
    __shared__ uint32_t red[kWaves][kInternal + 1];
    __shared__ uint32_t hred[kWaves][2];
    __shared__ uint64_t wg_tot[32];
    uint32_t wsum[kInternal + 1];
#pragma unroll
    for (int c = 0; c < kInternal; ++c) wsum[c] = wave_sum_lane63(s.acc[c]);
    wsum[kInternal] = wave_sum_lane63(cnt);
    const uint32_t we = wave_or_lane63(or_even & 0xFFFF0000u);   // the even-dword stream: bits 16-31 of every element
    const uint32_t wo = wave_or_lane63(or_odd);                   // W = 8: bits 32-63
    if (lane == 63) {
#pragma unroll
        for (int c = 0; c <= kInternal; ++c) red[wave][c] = wsum[c];
        hred[wave][0] = we;
        hred[wave][1] = wo;
    }
    __syncthreads();
    if (threadIdx.x <= kInternal) {
        uint64_t sum = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) sum += red[w][threadIdx.x];
        wg_tot[threadIdx.x] = sum;
    }
    if (threadIdx.x == 128 && high != nullptr) {
        uint32_t e = 0, o = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            e |= hred[w][0];
            o |= hred[w][1];
        }
        const uint64_t mask = (static_cast<uint64_t>(o) << 32) | e;
        if (mask) (void)__hip_atomic_fetch_or(high, mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const uint64_t wg_selected = wg_tot[kInternal];
    if (threadIdx.x == 64 && selected != nullptr && wg_selected)
        (void)__hip_atomic_fetch_add(selected, wg_selected, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // this workgroup's totals, mapped to the reference's slots, added to out[32]; every workgroup enters its own number of
    // passing elements into slot 9 (superset)
    finalize_slots<true>(wg_tot, out, mode, wg_selected);
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
extern "C" hipError_t fsk_launch_wide_filter(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                             const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* d_out32, uint64_t* d_selected,
                                             uint64_t* d_high, int mode, uint32_t grid, hipStream_t stream)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || (mode & ~3) || grid == 0 || d_out32 == nullptr || require > 0xFFFFu || exclude > 0xFFFFu ||
        min_mapq > 255u || (n && (d_array == nullptr || (min_mapq && d_mapq == nullptr))))
        return hipErrorInvalidValue;
    uint64_t geo[6];
    hipError_t e = fsk_wide_geometry(reinterpret_cast<uintptr_t>(d_array), n, elem_bytes, grid, geo);
    if (e != hipSuccess) return e;
    if ((mode & 1) && (e = fsdrv::zero_counters(d_out32, d_selected, d_high, stream)) != hipSuccess) return e;
    // a bit both required and excluded: no flag passes (samtools accepts the pair); the kernel's test assumes a disjoint pair.
    // Nothing is launched, so no element is read and the mask stays what the store form's memset or the caller left there.
    if (n == 0 || (require & exclude)) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(reinterpret_cast<uintptr_t>(d_array) & ~static_cast<uintptr_t>(15));
    // grid position q is element q - lo: its byte is d_mapq[q - lo]
    const uint8_t* mq = min_mapq ? reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_mapq) - geo[0]) : nullptr;
    const uint32_t mm = min_mapq;
    const dim3 g(static_cast<uint32_t>(geo[5])), b(fsk::kThreads);
#define FSK_WF_LAUNCH(W, Q)                                                                                                          \
    hipLaunchKernelGGL((fsk::flagstat_count_wide_filter<W, Q>), g, b, 0, stream, a0, mq, require, exclude, mm, geo[0], geo[1], geo[2], \
                       geo[3], geo[4], d_out32, d_selected, d_high, mode & 2)
    if (elem_bytes == 4) {
        if (min_mapq)
            FSK_WF_LAUNCH(4, true);
        else
            FSK_WF_LAUNCH(4, false);
    } else {
        if (min_mapq)
            FSK_WF_LAUNCH(8, true);
        else
            FSK_WF_LAUNCH(8, false);
    }
#undef FSK_WF_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The three forms are the shared bodies of flagstat_derived_host.h with two trailing words: the 33rd is the number of passing
// elements (added in the accumulate form), the 34th the mask (ORed).
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU: the wide entries' list, then the filter entries', in their words
int wide_filter_args(const void* array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude, const uint8_t* mapq,
                     uint32_t min_mapq, const void* out, int flags)
{
    using namespace fsdrv;
    return refused(check_elem_bytes(elem_bytes, "elem_bytes 2: 16-bit arrays go to the u16 filter entries (FLAGSTATS_hip_u16_x64_filter, "
                                                "FLAGSTATS_hip_device_u16_filter)") ||
                   check_predicate(require, exclude, min_mapq) || check_flags(flags) || check_array_given(array, n) ||
                   check_mapq_given(mapq, n, min_mapq) || check_array_layout(array, n, elem_bytes) || check_counters(out, n, flags));
}

constexpr const char* kWideFilterAlloc = "hipMalloc(wide filter counters)";

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_wide_filter(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                     const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected, uint64_t* d_high,
                                     int flags, void* stream)
{
    FS_ENTRY();
    int rc = wide_filter_args(d_array, n, elem_bytes, require, exclude, d_mapq, min_mapq, d_out, flags);
    if (rc) return rc;
    if (n == 0 && !(flags & 1)) return 0;
    const fsdrv::DeviceWord words[] = {{d_selected, "d_selected", "the count is added with a device atomic"},
                                       {d_high, "d_high", "the mask is ORed with a device atomic"}};
    fsdrv::Inputs in;
    in.add_columns(d_array, n, elem_bytes, nullptr, 0, 0, d_mapq, min_mapq);
    fsdrv::DeviceCall call;
    if ((rc = call.open(d_out, words, 2, in.in, in.count, stream))) return rc;
    Engine* e = call.e;
    hipStream_t s = call.s;
    if ((rc = fsdrv::step_fits(d_array, n, elem_bytes, fsint::grid_for(*e)))) return rc;
    if ((rc = fsdrv::check_extents(d_out, words, 2, in.in, in.count))) return rc;
    FS_HIP_TRY(fsk_launch_wide_filter(d_array, n, elem_bytes, require, exclude, d_mapq, min_mapq, d_out, d_selected, d_high, flags & 3,
                                      fsint::grid_for(*e), s));
    return 0;
}

int FLAGSTATS_hip_device_wide_filter_sync(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                          const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* out, uint64_t* selected, uint64_t* high,
                                          int flags)
{
    FS_ENTRY();
    int rc = wide_filter_args(d_array, n, elem_bytes, require, exclude, d_mapq, min_mapq, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, high, flags);
        return 0;
    }
    fsdrv::Inputs in;
    in.add_columns(d_array, n, elem_bytes, nullptr, 0, 0, d_mapq, min_mapq);
    return fsdrv::sync_call2(
        in.in, in.count, kWideFilterAlloc, out, selected, high, flags,
        [&](Engine& e) { return fsdrv::step_fits(d_array, n, elem_bytes, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_wide_filter(d_array, n, elem_bytes, require, exclude, d_mapq, min_mapq, row.d, row.d + 32, row.d + 33,
                                              1 | (flags & 2), fsint::grid_for(e), s));
            return 0;
        });
}

int FLAGSTATS_hip_wide_x64_filter(const void* array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude, const uint8_t* mapq,
                                  uint32_t min_mapq, uint64_t* out, uint64_t* selected, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = wide_filter_args(array, n, elem_bytes, require, exclude, mapq, min_mapq, out, flags);
    if (rc) return rc;
    // an overlapping pair passes nothing and reads no element: nothing crosses the bus
    if (n == 0 || (require & exclude)) {
        fsdrv::store_nothing(out, selected, high, flags);
        return 0;
    }
    // the array crosses the bus as it is, in chunks of "chunk_flags" * 2 bytes (as FLAGSTATS_hip_wide_x64); a chunk's slice of the
    // MAPQ column rides in the same staging buffer, behind its elements
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const uint64_t chunk = fsdrv::chunk_flags() * 2 / W;               // elements per chunk
    const uint64_t cap = n < chunk ? n : chunk;                         // elements of the largest chunk
    const uint64_t mapq_cap = min_mapq ? cap : 0;                       // bytes of its MAPQ slice
    const int mode = flags & 2;
    const uint8_t* src = static_cast<const uint8_t*>(array);
    return fsdrv::host_call2(
        n, chunk, cap * W / 2 + (mapq_cap + 1) / 2, kWideFilterAlloc, out, selected, high, flags,
        [&](Engine& e) { return fsdrv::step_fits(nullptr, cap, elem_bytes, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, int sl, uint64_t pos, uint64_t c) {
            const uint32_t grid = fsint::grid_for(e);
            uint8_t* d_mapq = reinterpret_cast<uint8_t*>(e.stage[sl]) + cap * W;
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], src + pos * W, c * W, hipMemcpyHostToDevice, e.stream[sl]));
            if (min_mapq) FS_HIP_TRY(hipMemcpyAsync(d_mapq, mapq + pos, c, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_wide_filter(e.stage[sl], c, elem_bytes, require, exclude, d_mapq, min_mapq, row.d, row.d + 32, row.d + 33,
                                              mode, grid, e.stream[sl]));
            return 0;
        });
}

}  // extern "C"
