// flagstat_filter.hip -- flagstat of the elements of a uint16 FLAG array that pass samtools' view filter: the 32 counters of
// {flag[i] : pass(i)} and the number of i that pass, where
//   pass(i) = (flag[i] & require) == require && (flag[i] & exclude) == 0 && (min_mapq == 0 || mapq[i] >= min_mapq)
// (-f require, -F exclude, -q min_mapq; mapq is one uint8 per element).  One pass over the array (and the MAPQ column when
// min_mapq > 0), one kernel, no selection array in memory.
//
// Geometry.  K1's and the selected-elements kernel's (flagstat_where.hip): the array is addressed on the 16-byte grid of its
// aligned-down base, the caller's flags occupy positions [lo, hi) of it, steps of 32 KiB = 16,384 flags; workgroup b takes the
// head edge step (b == 0), the tail edge step, then the fully covered steps b, b + G, ...; each wave owns a contiguous 8 KiB of a
// step and lane l takes vectors u * 64 + l.  Edge steps go through guarded, zero-filling loaders; fast steps through K1's rolling
// load schedule 71 (reissue, flagstat_count_core.h).  The step split is fsdrv::step_split's (flagstat_derived_host.h;
// tests/steps_oracle.StepSplit).
//
// MAPQ.  Addressed like the byte form of `where`: the launcher hands the kernel `mq` such that the 8 bytes of grid vector j are
// mq[8 j .. 8 j + 8), at any alignment; one unaligned dwordx2 per vector, loaded with the vector on fast steps.  Edge steps read
// only bytes of elements in [0, n).  The kernel is a template on whether the column is read at all (min_mapq == 0: it is not,
// and the pointer may be NULL).
//
// Predicate.  A zero flag counts nothing in any slot, so filtering is zeroing the flags that fail, in front of front4, on the
// byte planes L (FLAG bits 0-7 of 4 flags) and H (bits 8-15) that split_out produces.  With r = require, e = exclude, m = r | e
// and r & e == 0 (the launcher answers an overlapping pair itself: it selects nothing), a flag passes iff ((flag ^ r) & m) == 0.
// r, e and min_mapq are launch arguments, uniform over the grid; their byte-replicated forms live in registers.  Per 4 flags:
//   x1 = (L ^ rL) & mL                      v_bitop3_b32
//   x2 = (H ^ rH) & mH                      v_bitop3_b32
//   a  = (x1 | x2) & 0x7F..                 v_bitop3_b32
//   t  = a + 0x7F..                         v_add_u32       bit 7 of a byte: one of bits 0-6 of x1 | x2 is set (no carry leaves)
//   q  = t | x1 | x2                        v_bitop3_b32    bit 7 of a byte: the flag fails
//   p  = ~q & 0x80..                        v_bitop3_b32    0x80 per passing flag        [with MAPQ: ~q & g & 0x80.., see below]
//   M  = v_perm_b32(0, 0, p)                v_perm_b32      a selector byte of 0x80 writes 0xFF, one of 0x00 a source byte (0x00)
//   L &= M, H &= M                          2 x v_and_b32
//   cnt += popcount(p)                      v_bcnt_u32_b32
// = 10 VALU ops.  MAPQ adds 3: the byte-wise unsigned w >= y (gfx950 has no packed u8 compare) is SWAR across bit 7:
//   u  = w | 0x80..                         v_or_b32
//   t2 = u - (y & 0x7F) * 0x01..            v_sub_u32       every byte of u is >= 0x80 > y & 0x7F: no borrow leaves a byte;
//                                                           bit 7 of a byte: (w & 0x7F) >= (y & 0x7F)
//   g  = majority(w, t2, y < 128 ? 0x80.. : 0)              v_bitop3_b32    bit 7: y < 128: w7 | t2_7; y >= 128: w7 & t2_7
// Edge steps additionally clear p for positions outside [lo, hi) (a zero-filled position passes every predicate without
// `require` bits and would be counted in `selected`).
//
// Epilogue.  K1's direct one, as in flagstat_where.hip: finalize_slots<true> and one relaxed agent-scope atomic for `selected`,
// which is also what the superset slot 9 takes for the flag count.  No workspace, no second kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_filter.h"
#include "flagstat_filter_device.h"

namespace fsk {

constexpr int kFilterDepth = 8;       // chain depth as K1: epochs of 255 steps

// One step: 8 vectors of 16 B per lane = 64 flags through K1's tree (tree_step, flagstat_count_core.h), the predicate applied in
// the per-vector front.  ROLL 0 (edge steps): the vectors are in v[], their MAPQ bytes in m[], the bits of their positions that
// are elements in vb[].  ROLL 1, 2: K1's schedule 71 (reissue, same header); the MAPQ bytes of a vector are loaded right in
// front of it and read out with it.
template <bool MAPQ, int ROLL>
__device__ __forceinline__ void filter_step_and_count(Lane<kFilterDepth>& s, const FilterArgs& f, uint4 (&v)[kUnroll], uint2 (&m)[kUnroll],
                                                      const uint32_t (&vb)[kUnroll], uint32_t& blk, uint32_t& cnt,
                                                      const uint4* __restrict__ cur = nullptr, const uint4* __restrict__ next = nullptr,
                                                      const uint8_t* __restrict__ mcur = nullptr, const uint8_t* __restrict__ mnext = nullptr)
{
    blk = __builtin_amdgcn_readfirstlane(blk);
    tree_step<kFilterDepth>(s, blk, [&](int uu, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        split_out(v[uu], L0, H0, L1, H1);
        uint2 w = make_uint2(0, 0);
        if constexpr (MAPQ) {
            w = m[uu];
            reissue<ROLL>(uu, m, mcur, mnext, kWaveStride * 8, load_mapq);
        }
        reissue<ROLL>(uu, v, cur, next, kWaveStride, load_vec<true>);
        uint32_t p0 = pass4<MAPQ>(f, L0, H0, w.x);
        uint32_t p1 = pass4<MAPQ>(f, L1, H1, w.y);
        if constexpr (ROLL == 0) {
            p0 &= nibble_to_bit7(vb[uu] & 15u);
            p1 &= nibble_to_bit7(vb[uu] >> 4);
        }
        cnt += __builtin_popcount(p0);
        cnt += __builtin_popcount(p1);
        const uint32_t M0 = perm(0u, 0u, p0), M1 = perm(0u, 0u, p1);   // selector 0x80 -> 0xFF, 0x00 -> source byte 0 = 0x00
        L0 &= M0;
        H0 &= M0;
        L1 &= M1;
        H1 &= M1;
        __builtin_amdgcn_sched_barrier(0);
    });
    end_step<kFilterDepth>(s, blk);
}

// a0: 16-B aligned-down base; the caller's flags occupy positions [lo, hi) of its grid.  mq: the MAPQ column on the same grid
// (the byte of position q is mq[q]; not read when !MAPQ).  require & exclude == 0 (the launcher's business), both below 2^16,
// min_mapq in 1..255 when MAPQ.  mode: bit 1 superset (bit 0, the store form, is the launcher's memset).  selected may be nullptr.
template <bool MAPQ>
__global__ __launch_bounds__(kThreads) void flagstat_count_filter(const uint4* __restrict__ a0, const uint8_t* __restrict__ mq, uint32_t require,
                                                                  uint32_t exclude, uint32_t min_mapq, uint64_t lo, uint64_t hi,
                                                                  uint64_t nsteps, uint64_t fast_begin, uint64_t fast_end,
                                                                  uint64_t* __restrict__ out, uint64_t* __restrict__ selected, int mode)
{
    Lane<kFilterDepth> s;
    lane_init(s);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    constexpr int VPS = kVecPerStep;
    constexpr int US = kWaveStride;
    const uint64_t lane_off = static_cast<uint64_t>(wave) * (US * kUnroll) + lane;
    const uint64_t G = gridDim.x;
    const FilterArgs f = filter_args_of(require, exclude, min_mapq);
    uint32_t blk = stagger_start(wave);
    uint32_t cnt = 0;                           // passing elements of this lane

    auto edge_step = [&](uint64_t st) {
        uint4 v[kUnroll];
        uint2 m[kUnroll];
        uint32_t vb[kUnroll];
        const uint64_t j0 = st * VPS + lane_off;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            v[u] = load_guarded(a0, j0 + u * US, lo, hi);
            vb[u] = valid_bits(j0 + u * US, lo, hi);
            if constexpr (MAPQ)
                m[u] = load_mapq_guarded(mq, j0 + u * US, lo, hi);
            else
                m[u] = make_uint2(0, 0);
        }
        filter_step_and_count<MAPQ, 0>(s, f, v, m, vb, blk, cnt);
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
        uint2 m[kUnroll];
        const uint32_t vb[kUnroll] = {};        // not looked at on fast steps
        const uint4* p = a0 + st * VPS + lane_off;
        const uint8_t* pm = mq + (st * VPS + lane_off) * 8;
        // the first RD vectors; the rest is issued as they are consumed
#pragma unroll
        for (int u = 0; u < RD; ++u) {
            if constexpr (MAPQ) m[u] = load_mapq(pm + u * US * 8);
            v[u] = load_vec<true>(p + u * US);
            __builtin_amdgcn_sched_barrier(0);
        }
        for (; st + G < fast_end; st += G) {
            const uint4* pn = p + G * VPS;
            const uint8_t* pmn = pm + G * VPS * 8;
            filter_step_and_count<MAPQ, 1>(s, f, v, m, vb, blk, cnt, p, pn, pm, pmn);
            p = pn;
            pm = pmn;
        }
        filter_step_and_count<MAPQ, 2>(s, f, v, m, vb, blk, cnt, p, nullptr, pm, nullptr);
    }
    flush(s, blk);

    // wave sums on the VALU (DPP), then the 4 waves through LDS; word kInternal is the number of passing elements
    constexpr int kWaves = kThreads / 64;
    __shared__ uint32_t red[kWaves][kInternal + 1];
    __shared__ uint64_t wg_tot[32];
    uint32_t wsum[kInternal + 1];
#pragma unroll
    for (int c = 0; c < kInternal; ++c) wsum[c] = wave_sum_lane63(s.acc[c]);
    wsum[kInternal] = wave_sum_lane63(cnt);
    if (lane == 63) {
#pragma unroll
        for (int c = 0; c <= kInternal; ++c) red[wave][c] = wsum[c];
    }
    __syncthreads();
    if (threadIdx.x <= kInternal) {
        uint64_t sum = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) sum += red[w][threadIdx.x];
        wg_tot[threadIdx.x] = sum;
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
extern "C" hipError_t fsk_launch_filter(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                        uint32_t min_mapq, uint64_t* d_out32, uint64_t* d_selected, int mode, uint32_t grid,
                                        hipStream_t stream)
{
    if ((mode & ~3) || grid == 0 || d_out32 == nullptr || require > 0xFFFFu || exclude > 0xFFFFu || min_mapq > 255u ||
        (n && (d_array == nullptr || (min_mapq && d_mapq == nullptr))))
        return hipErrorInvalidValue;
    uint64_t geo[6];
    hipError_t e = fsdrv::step_split(reinterpret_cast<uintptr_t>(d_array), n, 2, grid, geo);
    if (e != hipSuccess) return e;
    if ((mode & 1) && (e = fsdrv::zero_counters(d_out32, d_selected, stream)) != hipSuccess) return e;
    // a bit both required and excluded: no flag passes (samtools accepts the pair); the kernel's test assumes a disjoint pair
    if (n == 0 || (require & exclude)) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(reinterpret_cast<uintptr_t>(d_array) & ~static_cast<uintptr_t>(15));
    const dim3 g(static_cast<uint32_t>(geo[5])), b(fsk::kThreads);
    if (min_mapq) {
        // grid position q is element q - lo: its byte is d_mapq[q - lo]
        const uint8_t* mq = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_mapq) - geo[0]);
        hipLaunchKernelGGL((fsk::flagstat_count_filter<true>), g, b, 0, stream, a0, mq, require, exclude, min_mapq, geo[0], geo[1], geo[2],
                           geo[3], geo[4], d_out32, d_selected, mode & 2);
    } else {
        hipLaunchKernelGGL((fsk::flagstat_count_filter<false>), g, b, 0, stream, a0, static_cast<const uint8_t*>(nullptr), require, exclude,
                           0u, geo[0], geo[1], geo[2], geo[3], geo[4], d_out32, d_selected, mode & 2);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The three forms are the shared bodies of flagstat_derived_host.h; the 33rd word is the number of passing elements.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU
int filter_args(const uint16_t* array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* mapq, uint32_t min_mapq,
                const void* out, int flags)
{
    using namespace fsdrv;
    return refused(check_predicate(require, exclude, min_mapq) || check_flags(flags) || check_array_given(array, n) ||
                   check_mapq_given(mapq, n, min_mapq) || check_array_layout(array, n, 2) || check_counters(out, n, flags));
}

constexpr const char* kFilterAlloc = "hipMalloc(filter counters)";

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_u16_filter(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                    uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected, int flags, void* stream)
{
    FS_ENTRY();
    int rc = filter_args(d_array, n, require, exclude, d_mapq, min_mapq, d_out, flags);
    if (rc) return rc;
    if (n == 0 && !(flags & 1)) return 0;
    const fsdrv::DeviceWord word{d_selected, "d_selected", "the count is added with a device atomic"};
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, nullptr, 0, 0, d_mapq, min_mapq);
    fsdrv::DeviceCall call;
    if ((rc = call.open(d_out, word, in.in, in.count, stream))) return rc;
    Engine* e = call.e;
    hipStream_t s = call.s;
    if ((rc = fsdrv::step_fits(d_array, n, 2, fsint::grid_for(*e)))) return rc;
    if ((rc = fsdrv::check_extents(d_out, word, in.in, in.count))) return rc;
    FS_HIP_TRY(fsk_launch_filter(d_array, n, require, exclude, d_mapq, min_mapq, d_out, d_selected, flags & 3, fsint::grid_for(*e), s));
    return 0;
}

int FLAGSTATS_hip_device_u16_filter_sync(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                         uint32_t min_mapq, uint64_t* out, uint64_t* selected, int flags)
{
    FS_ENTRY();
    int rc = filter_args(d_array, n, require, exclude, d_mapq, min_mapq, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, flags);
        return 0;
    }
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, nullptr, 0, 0, d_mapq, min_mapq);
    return fsdrv::sync_call(
        in.in, in.count, kFilterAlloc, out, selected, flags, fsdrv::kWordAdd,
        [&](Engine& e) { return fsdrv::step_fits(d_array, n, 2, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_filter(d_array, n, require, exclude, d_mapq, min_mapq, row.d, row.d + 32, 1 | (flags & 2), fsint::grid_for(e), s));
            return 0;
        });
}

int FLAGSTATS_hip_u16_x64_filter(const uint16_t* array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* mapq, uint32_t min_mapq,
                                 uint64_t* out, uint64_t* selected, int flags)
{
    FS_ENTRY();
    int rc = filter_args(array, n, require, exclude, mapq, min_mapq, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, flags);
        return 0;
    }
    // a chunk's slice of the MAPQ column rides in the same staging buffer, behind the flags
    const uint64_t chunk = fsdrv::chunk_flags();
    const uint64_t cap = n < chunk ? n : chunk;                         // flags of the largest chunk
    const uint64_t mapq_cap = min_mapq ? cap : 0;                       // bytes of its MAPQ slice
    const int mode = flags & 2;
    return fsdrv::host_call(
        n, chunk, cap + (mapq_cap + 1) / 2, kFilterAlloc, out, selected, flags, fsdrv::kWordAdd,
        [&](Engine& e) { return fsdrv::step_fits(nullptr, cap, 2, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, int sl, uint64_t pos, uint64_t c) {
            const uint32_t grid = fsint::grid_for(e);
            uint8_t* d_mapq = reinterpret_cast<uint8_t*>(e.stage[sl] + cap);
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], array + pos, c * 2, hipMemcpyHostToDevice, e.stream[sl]));
            if (min_mapq) FS_HIP_TRY(hipMemcpyAsync(d_mapq, mapq + pos, c, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_filter(e.stage[sl], c, require, exclude, d_mapq, min_mapq, row.d, row.d + 32, mode, grid, e.stream[sl]));
            return 0;
        });
}

}  // extern "C"
