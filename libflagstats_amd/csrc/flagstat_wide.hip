// flagstat_wide.hip -- flagstat of a FLAG array held as 4-byte or 8-byte little-endian integers (int32 / int64 columns), read in
// place: the low 16 bits of every element are counted exactly as K1 counts a uint16, and every bit above bit 15 that any
// element carries is ORed into one uint64 mask, in the same pass.
//
// Geometry.  K1's, in bytes: the array is addressed on the 16-byte grid of its aligned-down base and cut into steps of 32 KiB
// (256 lanes x 8 vectors of 16 B: 8,192 elements at W = 4, 4,096 at W = 8); workgroup b takes the head edge step (b == 0), the
// tail edge step, then the fully covered steps b, b + G, ...; each wave owns a contiguous 8 KiB of a step.  Edge steps go through
// a guarded, zero-filling loader (a zero element counts nothing and sets no mask bit); fast steps through K1's rolling load
// schedule (schedule 71: a vector's registers are re-issued for the vector six places on as soon as it has been read out:
// reissue, flagstat_count_core.h).  tests/steps_oracle.StepSplit(addr % 16, n * W / 2, grid) is the step split.
//
// Narrowing.  front4 (flagstat_count_core.h) wants 4 flags as a dword L of their low bytes and a dword H of their high bytes.
// One v_perm_b32 takes two flag-carrying dwords a, b to P = [a.b0, b.b0, a.b1, b.b1]; a second pair of perms takes two P to L
// and H.  At W = 4 every loaded vector (4 elements) gives one (L, H); at W = 8 the even dwords of two vectors do, and the odd
// dwords are all high bits and feed only the mask.  A step thus has 8 (W = 4) or 4 (W = 8) inputs where K1 has 16: they go
// through the first three (two) levels of K1's carry-save tree and the carry is walked up the remaining planes alone, so a step
// still ends in ONE weight-16 push into the lane's chain -- epochs of 255 steps, the flush and the wave stagger are K1's.
//
// Mask.  Each lane ORs its loaded dwords together (v_or3_b32: one per two dwords), even and -- at W = 8 -- odd dwords apart;
// at the end the even stream is cut to its bits 16-31, the wave ORs over its lanes (DPP), the workgroup over its waves (LDS),
// and a workgroup whose value is non-zero does one relaxed agent-scope atomic OR on the caller's word.
//
// Epilogue.  K1's direct one: every workgroup maps its 21 totals to the 32 slots and adds them to out[32] with relaxed
// agent-scope atomics.  No workspace, no second kernel; the store form zeroes counters and mask in front (one memset).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_wide.h"
#include "flagstat_wide_device.h"

namespace fsk {

constexpr int kWideDepth = 8;        // chain depth as K1: epochs of 255 steps

// narrow_out, wide_tree, wide_step_with, load_guarded_wide and wave_or_lane63 are flagstat_wide_device.h's (shared with
// flagstat_wide_filter.hip and flagstat_segments_wide.hip)

// One step (wide_step_with) under this kernel's load schedule.
// ROLL 0: the vectors are in v[].  ROLL 1, 2: K1's schedule 71 -- vector u's registers are re-issued for vector u + 6 of the same
// step (`cur`) or, ROLL 1 only, u - 2 of the next one (`next`): 6 loads = 24 KiB per CU in flight.
template <int W, int ROLL>
__device__ __forceinline__ void wide_step(Lane<kWideDepth>& s, uint4 (&v)[kUnroll], uint32_t blk, uint32_t& or_even, uint32_t& or_odd,
                                          const uint4* __restrict__ cur, const uint4* __restrict__ next)
{
    wide_step_with<W>(s, v, blk, or_even, or_odd, [&](int u) __attribute__((always_inline)) {
        reissue<ROLL>(u, v, cur, next, kWaveStride, load_vec<true>);
    });
}

template <int W, int ROLL>
__device__ __forceinline__ void wide_step_and_count(Lane<kWideDepth>& s, uint4 (&v)[kUnroll], uint32_t& blk, uint32_t& or_even,
                                                    uint32_t& or_odd, const uint4* __restrict__ cur = nullptr,
                                                    const uint4* __restrict__ next = nullptr)
{
    blk = __builtin_amdgcn_readfirstlane(blk);
    wide_step<W, ROLL>(s, v, blk, or_even, or_odd, cur, next);
    end_step<kWideDepth>(s, blk);
}

// a0: 16-B aligned-down base; the caller's elements occupy positions [lo, hi) of its grid of W-byte elements.  mode: bit 1
// superset (bit 0, the store form, is the launcher's memset).  high may be nullptr.
template <int W>
__global__ __launch_bounds__(kThreads) void flagstat_count_wide(const uint4* __restrict__ a0, uint64_t lo, uint64_t hi, uint64_t nsteps,
                                                                uint64_t fast_begin, uint64_t fast_end, uint64_t* __restrict__ out,
                                                                uint64_t* __restrict__ high, int mode)
{
    static_assert(W == 4 || W == 8, "4-byte or 8-byte elements");
    Lane<kWideDepth> s;
    lane_init(s);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    constexpr int VPS = kVecPerStep;
    constexpr int US = kWaveStride;
    const uint64_t lane_off = static_cast<uint64_t>(wave) * (US * kUnroll) + lane;
    const uint64_t G = gridDim.x;
    uint32_t blk = stagger_start(wave);
    uint32_t or_even = 0, or_odd = 0;

    auto edge_step = [&](uint64_t st) {
        uint4 v[kUnroll];
        const uint64_t j0 = st * VPS + lane_off;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) v[u] = load_guarded_wide<W>(a0, j0 + u * US, lo, hi);
        wide_step_and_count<W, 0>(s, v, blk, or_even, or_odd);
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
        const uint4* p = a0 + st * VPS + lane_off;
#pragma unroll
        for (int u = 0; u < RD; ++u) {  // the first RD vectors; the rest is issued as they are consumed
            v[u] = load_vec<true>(p + u * US);
            __builtin_amdgcn_sched_barrier(0);
        }
        for (; st + G < fast_end; st += G) {
            const uint4* pn = p + G * VPS;
            wide_step_and_count<W, 1>(s, v, blk, or_even, or_odd, p, pn);
            p = pn;
        }
        wide_step_and_count<W, 2>(s, v, blk, or_even, or_odd, p);
    }
    flush(s, blk);

    // wave sums and ORs on the VALU (DPP), then the 4 waves through LDS
    constexpr int kWaves = kThreads / 64;
    __shared__ uint32_t red[kWaves][kInternal];
    __shared__ uint32_t hred[kWaves][2];
    __shared__ uint64_t wg_tot[32];
    uint32_t wsum[kInternal];
#pragma unroll
    for (int c = 0; c < kInternal; ++c) wsum[c] = wave_sum_lane63(s.acc[c]);
    const uint32_t we = wave_or_lane63(or_even & 0xFFFF0000u);   // the even-dword stream: bits 16-31 of every element
    const uint32_t wo = wave_or_lane63(or_odd);                   // W = 8: bits 32-63
    if (lane == 63) {
#pragma unroll
        for (int c = 0; c < kInternal; ++c) red[wave][c] = wsum[c];
        hred[wave][0] = we;
        hred[wave][1] = wo;
    }
    __syncthreads();
    if (threadIdx.x < kInternal) {
        uint64_t sum = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) sum += red[w][threadIdx.x];
        wg_tot[threadIdx.x] = sum;
    }
    if (threadIdx.x == 64 && high != nullptr) {
        uint32_t e = 0, o = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            e |= hred[w][0];
            o |= hred[w][1];
        }
        const uint64_t m = (static_cast<uint64_t>(o) << 32) | e;
        if (m) (void)__hip_atomic_fetch_or(high, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    // this workgroup's totals, mapped to the reference's slots, added to out[32]; n enters slot 9 (superset) in workgroup 0
    finalize_slots<true>(wg_tot, out, mode, blockIdx.x == 0 ? hi - lo : 0);
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
// Host-side geometry: the shared step split (flagstat_derived_host.h) at W = 4 or 8.
extern "C" hipError_t fsk_wide_geometry(uint64_t address, uint64_t n, int elem_bytes, uint32_t grid, uint64_t* geo)
{
    if (elem_bytes != 4 && elem_bytes != 8) return hipErrorInvalidValue;
    return fsdrv::step_split(address, n, elem_bytes, grid, geo);
}

extern "C" hipError_t fsk_launch_wide(const void* d_array, uint64_t n, int elem_bytes, uint64_t* d_out32, uint64_t* d_high, int mode,
                                      uint32_t grid, hipStream_t stream)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || (mode & ~3) || grid == 0 || d_out32 == nullptr || (n && d_array == nullptr))
        return hipErrorInvalidValue;
    uint64_t geo[6];
    hipError_t e = fsk_wide_geometry(reinterpret_cast<uintptr_t>(d_array), n, elem_bytes, grid, geo);
    if (e != hipSuccess) return e;
    if ((mode & 1) && (e = fsdrv::zero_counters(d_out32, d_high, stream)) != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(reinterpret_cast<uintptr_t>(d_array) & ~static_cast<uintptr_t>(15));
    const dim3 g(static_cast<uint32_t>(geo[5])), b(fsk::kThreads);
    if (elem_bytes == 4)
        hipLaunchKernelGGL(fsk::flagstat_count_wide<4>, g, b, 0, stream, a0, geo[0], geo[1], geo[2], geo[3], geo[4], d_out32, d_high, mode & 2);
    else
        hipLaunchKernelGGL(fsk::flagstat_count_wide<8>, g, b, 0, stream, a0, geo[0], geo[1], geo[2], geo[3], geo[4], d_out32, d_high, mode & 2);
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The three forms are the shared bodies of flagstat_derived_host.h; the 33rd word is the mask, ORed in the accumulate form.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU
int wide_args(const void* array, uint64_t n, int elem_bytes, const void* out, int flags)
{
    using namespace fsdrv;
    return refused(check_elem_bytes(elem_bytes, "elem_bytes 2: 16-bit arrays go to the u16 entries (FLAGSTATS_u16_x64, FLAGSTATS_hip_device_u16)") ||
                   check_flags(flags) || check_array_given(array, n) || check_array_layout(array, n, elem_bytes) ||
                   check_counters(out, n, flags));
}

constexpr const char* kWideAlloc = "hipMalloc(wide counters)";

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_wide(const void* d_array, uint64_t n, int elem_bytes, uint64_t* d_out, uint64_t* d_high, int flags, void* stream)
{
    FS_ENTRY();
    int rc = wide_args(d_array, n, elem_bytes, d_out, flags);
    if (rc) return rc;
    if (n == 0 && !(flags & 1)) return 0;
    const fsdrv::DeviceWord word{d_high, "d_high", "the mask is ORed with a device atomic"};
    fsdrv::Inputs in;
    in.add_columns(d_array, n, elem_bytes, nullptr, 0, 0, nullptr, 0);
    fsdrv::DeviceCall call;
    if ((rc = call.open(d_out, word, in.in, in.count, stream))) return rc;
    if ((rc = fsdrv::check_extents(d_out, word, in.in, in.count))) return rc;
    Engine* e = call.e;
    hipStream_t s = call.s;
    FS_HIP_TRY(fsk_launch_wide(d_array, n, elem_bytes, d_out, d_high, flags & 3, fsint::grid_for(*e), s));
    return 0;
}

int FLAGSTATS_hip_device_wide_sync(const void* d_array, uint64_t n, int elem_bytes, uint64_t* out, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = wide_args(d_array, n, elem_bytes, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, high, flags);
        return 0;
    }
    fsdrv::Inputs in;
    in.add_columns(d_array, n, elem_bytes, nullptr, 0, 0, nullptr, 0);
    return fsdrv::sync_call(in.in, in.count, kWideAlloc, out, high, flags, fsdrv::kWordOr, fsdrv::fits_always, [&](Engine& e, fsdrv::Row& row, hipStream_t s) {
        FS_HIP_TRY(fsk_launch_wide(d_array, n, elem_bytes, row.d, row.d + 32, 1 | (flags & 2), fsint::grid_for(e), s));
        return 0;
    });
}

int FLAGSTATS_hip_wide_x64(const void* array, uint64_t n, int elem_bytes, uint64_t* out, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = wide_args(array, n, elem_bytes, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, high, flags);
        return 0;
    }
    // the array crosses the bus as it is, in chunks of "chunk_flags" * 2 bytes; every chunk's launch adds into the same device
    // counters and ORs into the same mask word
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const uint64_t chunk_flags = fsdrv::chunk_flags();
    const uint64_t chunk = chunk_flags * 2 / W;   // elements per chunk
    const int mode = flags & 2;
    const uint8_t* src = static_cast<const uint8_t*>(array);
    return fsdrv::host_call(n, chunk, n < chunk ? (n * W + 1) / 2 : chunk_flags, kWideAlloc, out, high, flags, fsdrv::kWordOr, fsdrv::fits_always,
                            [&](Engine& e, fsdrv::Row& row, int sl, uint64_t pos, uint64_t c) {
                                const uint32_t grid = fsint::grid_for(e);
                                FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], src + pos * W, c * W, hipMemcpyHostToDevice, e.stream[sl]));
                                FS_HIP_TRY(fsk_launch_wide(e.stage[sl], c, elem_bytes, row.d, row.d + 32, mode, grid, e.stream[sl]));
                                return 0;
                            });
}

}  // extern "C"
