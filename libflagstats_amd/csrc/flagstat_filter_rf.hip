// flagstat_filter_rf.hip -- flagstat of the elements of a uint16 FLAG array that pass samtools' whole view predicate on FLAG and
// MAPQ: the 32 counters of {flag[i] : pass(i)} and the number of i that pass, where
//   pass(i) = (flag[i] & require) == require && (flag[i] & exclude) == 0
//             && (include_any == 0 || (flag[i] & include_any) != 0)
//             && (exclude_all == 0 || (flag[i] & exclude_all) != exclude_all)
//             && (min_mapq == 0 || mapq[i] >= min_mapq)
// (-f require, -F exclude, --rf / --incl-flags include_any, -G exclude_all, -q min_mapq).  The any-of and the all-of test cannot
// be written as a require / exclude pair once they name two bits: -G 0xC drops the pairs of which read and mate are both
// unmapped, --rf 0x50 keeps first or reverse.
//
// Reduction.  What can be written as a pair is: fsk_filter_rf_reduce (host code, below; its rules are stated at its declaration in
// flagstat_filter_rf.h) folds single bits and bits that -f / -F already decide into require / exclude and finds the predicates
// that pass nothing.  The launcher hands a plain pair to fsk_launch_filter -- the shipped kernel at its measured speed -- and
// launches nothing for an empty predicate; only a residue of at least two free bits in --rf or -G reaches the kernel of this file.
//
// Kernel.  fsk::flagstat_count_filter_rf is flagstat_count_filter (flagstat_filter.hip: geometry, fsdrv::step_split, guarded edge
// steps, rolling schedule 71 on fast steps, chain depth 8 with epochs of 255 steps, the direct epilogue) with up to two more tests
// ANDed into the pass word of 4 flags (pass4_rf of flagstat_filter_rf_device.h), in front of the popcount and of the v_perm_b32
// masks.  On the byte planes L (FLAG bits 0-7) and H (bits 8-15), with a = include_any, g = exclude_all byte-replicated in
// wave-uniform registers and p the parent's pass word (0x80 per passing flag):
//   any-of   t = L & aL                          v_and_b32
//            y = (H & aH) | t                    v_bitop3_b32    a byte of y is 0 iff the flag has no bit of a
//            s = (y & 0x7F..) + 0x7F..           v_and_b32, v_add_u32     bit 7 of a byte: one of bits 0-6 of y is set (no carry
//                                                                         leaves a byte)
//            p = (s | y) & p                     v_bitop3_b32
//   all-of   t = ~L & gL                         v_bitop3_b32
//            z = (~H & gH) | t                   v_bitop3_b32    a byte of z is 0 iff the flag has every bit of g
//            s = (z & 0x7F..) + 0x7F..           v_and_b32, v_add_u32
//            p = (s | z) & p                     v_bitop3_b32
// = 5 VALU ops per test on top of the parent's 10 (13 with MAPQ).  The kernel is a template on the MAPQ column and on which of
// the two tests the residue holds, so a test that is off costs nothing: six instantiations (DESIGN.md section 4 has what a test
// costs in time).
// A zero-filled position of an edge step passes the all-of test and fails the any-of one; as in the parent, the positions that
// are no element are cleared from p (valid_bits) in front of the count of passing elements, so neither matters.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_filter.h"
#include "flagstat_filter_device.h"
#include "flagstat_filter_rf.h"
#include "flagstat_filter_rf_device.h"

namespace fsk {

constexpr int kFilterRfDepth = 8;     // chain depth as K1: epochs of 255 steps

// One step, as flagstat_filter.hip's filter_step_and_count: 8 vectors of 16 B per lane through K1's tree, the predicate applied in
// the per-vector front.  ROLL 0 (edge steps): the vectors are in v[], their MAPQ bytes in m[], the bits of their positions that
// are elements in vb[].  ROLL 1, 2: schedule 71; the MAPQ bytes of a vector are loaded right in front of it.
template <bool MAPQ, bool ANY, bool ALL, int ROLL>
__device__ __forceinline__ void filter_rf_step_and_count(Lane<kFilterRfDepth>& s, const FilterArgs& f, const FilterRfArgs& r,
                                                         uint4 (&v)[kUnroll], uint2 (&m)[kUnroll], const uint32_t (&vb)[kUnroll],
                                                         uint32_t& blk, uint32_t& cnt, const uint4* __restrict__ cur = nullptr,
                                                         const uint4* __restrict__ next = nullptr,
                                                         const uint8_t* __restrict__ mcur = nullptr,
                                                         const uint8_t* __restrict__ mnext = nullptr)
{
    blk = __builtin_amdgcn_readfirstlane(blk);
    tree_step<kFilterRfDepth>(s, blk, [&](int uu, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        split_out(v[uu], L0, H0, L1, H1);
        uint2 w = make_uint2(0, 0);
        if constexpr (MAPQ) {
            w = m[uu];
            reissue<ROLL>(uu, m, mcur, mnext, kWaveStride * 8, load_mapq);
        }
        reissue<ROLL>(uu, v, cur, next, kWaveStride, load_vec<true>);
        uint32_t p0 = pass4_rf<MAPQ, ANY, ALL>(f, r, L0, H0, w.x);
        uint32_t p1 = pass4_rf<MAPQ, ANY, ALL>(f, r, L1, H1, w.y);
        if constexpr (ROLL == 0) {
            // in front of the count: a zero-filled position passes the all-of test
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
    end_step<kFilterRfDepth>(s, blk);
}

// flagstat_count_filter's arguments (flagstat_filter.hip) with the residue behind `exclude`: the four masks are
// fsk_filter_rf_reduce's, so require & exclude == 0, include_any and exclude_all are disjoint from both, all below 2^16;
// include_any != 0 iff ANY, exclude_all != 0 iff ALL.  min_mapq in 1..255 when MAPQ.  mode: bit 1 superset.
template <bool MAPQ, bool ANY, bool ALL>
__global__ __launch_bounds__(kThreads) void flagstat_count_filter_rf(const uint4* __restrict__ a0, const uint8_t* __restrict__ mq,
                                                                     uint32_t require, uint32_t exclude, uint32_t include_any,
                                                                     uint32_t exclude_all, uint32_t min_mapq, uint64_t lo, uint64_t hi,
                                                                     uint64_t nsteps, uint64_t fast_begin, uint64_t fast_end,
                                                                     uint64_t* __restrict__ out, uint64_t* __restrict__ selected, int mode)
{
    static_assert(ANY || ALL, "a plain require / exclude pair is flagstat_count_filter's");
    Lane<kFilterRfDepth> s;
    lane_init(s);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    constexpr int VPS = kVecPerStep;
    constexpr int US = kWaveStride;
    const uint64_t lane_off = static_cast<uint64_t>(wave) * (US * kUnroll) + lane;
    const uint64_t G = gridDim.x;
    const FilterArgs f = filter_args_of(require, exclude, min_mapq);
    const FilterRfArgs r = filter_rf_args_of(include_any, exclude_all);
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
        filter_rf_step_and_count<MAPQ, ANY, ALL, 0>(s, f, r, v, m, vb, blk, cnt);
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
            filter_rf_step_and_count<MAPQ, ANY, ALL, 1>(s, f, r, v, m, vb, blk, cnt, p, pn, pm, pmn);
            p = pn;
            pm = pmn;
        }
        filter_rf_step_and_count<MAPQ, ANY, ALL, 2>(s, f, r, v, m, vb, blk, cnt, p, nullptr, pm, nullptr);
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

// ------------------------------------------------------------------ the reduction (host code; rules: flagstat_filter_rf.h)
extern "C" int fsk_filter_rf_reduce(uint32_t require, uint32_t exclude, uint32_t include_any, uint32_t exclude_all, uint32_t out[4])
{
    uint32_t r = require, e = exclude, a = include_any, g = exclude_all;
    const auto one_bit = [](uint32_t x) { return (x & (x - 1)) == 0; };   // of a non-zero x
    bool empty = (r & e) != 0;
    // again: a bit moved into require or exclude, which the other test has to see
    for (bool again = true; again && !empty;) {
        again = false;
        if (a & r) {
            a = 0;                              // satisfied
        } else if (a) {
            a &= ~e;
            if (a == 0) {
                empty = true;                   // every bit it offers is excluded
            } else if (one_bit(a)) {
                r |= a;
                a = 0;
                again = true;
            }
        }
        if (g & e) {
            g = 0;                              // never all set
        } else if (g) {
            g &= ~r;
            if (g == 0) {
                empty = true;                   // always all set
            } else if (one_bit(g)) {
                e |= g;
                g = 0;
                again = true;
            }
        }
    }
    if (empty) r = e = a = g = 0;
    out[0] = r;
    out[1] = e;
    out[2] = a;
    out[3] = g;
    return empty ? 0 : (a | g) ? 2 : 1;
}

// ------------------------------------------------------------------ launcher
namespace {

template <bool MAPQ>
void launch_residue(bool any, bool all, dim3 g, dim3 b, hipStream_t stream, const uint4* a0, const uint8_t* mq, const uint32_t (&m)[4],
                    uint32_t min_mapq, const uint64_t (&geo)[6], uint64_t* d_out32, uint64_t* d_selected, int mode)
{
    auto* kernel = any && all ? fsk::flagstat_count_filter_rf<MAPQ, true, true>
                   : any      ? fsk::flagstat_count_filter_rf<MAPQ, true, false>
                              : fsk::flagstat_count_filter_rf<MAPQ, false, true>;
    hipLaunchKernelGGL(kernel, g, b, 0, stream, a0, mq, m[0], m[1], m[2], m[3], min_mapq, geo[0], geo[1], geo[2], geo[3], geo[4], d_out32,
                       d_selected, mode);
}

}  // namespace

extern "C" hipError_t fsk_launch_filter_rf(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, uint32_t include_any,
                                           uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* d_out32,
                                           uint64_t* d_selected, int mode, uint32_t grid, hipStream_t stream)
{
    if (require > 0xFFFFu || exclude > 0xFFFFu || include_any > 0xFFFFu || exclude_all > 0xFFFFu) return hipErrorInvalidValue;
    uint32_t m[4];
    const int kind = fsk_filter_rf_reduce(require, exclude, include_any, exclude_all, m);
    // a plain pair is the shipped kernel's; so is an empty predicate, as the overlapping pair that launcher answers itself
    if (kind == 1) return fsk_launch_filter(d_array, n, m[0], m[1], d_mapq, min_mapq, d_out32, d_selected, mode, grid, stream);
    if (kind == 0) return fsk_launch_filter(d_array, n, 1u, 1u, d_mapq, min_mapq, d_out32, d_selected, mode, grid, stream);
    if ((mode & ~3) || grid == 0 || d_out32 == nullptr || min_mapq > 255u || (n && (d_array == nullptr || (min_mapq && d_mapq == nullptr))))
        return hipErrorInvalidValue;
    uint64_t geo[6];
    hipError_t e = fsdrv::step_split(reinterpret_cast<uintptr_t>(d_array), n, 2, grid, geo);
    if (e != hipSuccess) return e;
    if ((mode & 1) && (e = fsdrv::zero_counters(d_out32, d_selected, stream)) != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(reinterpret_cast<uintptr_t>(d_array) & ~static_cast<uintptr_t>(15));
    const dim3 g(static_cast<uint32_t>(geo[5])), b(fsk::kThreads);
    if (min_mapq) {
        // grid position q is element q - lo: its byte is d_mapq[q - lo]
        const uint8_t* mq = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_mapq) - geo[0]);
        launch_residue<true>(m[2] != 0, m[3] != 0, g, b, stream, a0, mq, m, min_mapq, geo, d_out32, d_selected, mode & 2);
    } else {
        launch_residue<false>(m[2] != 0, m[3] != 0, g, b, stream, a0, nullptr, m, 0u, geo, d_out32, d_selected, mode & 2);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The three forms are the shared bodies of flagstat_derived_host.h, as flagstat_filter.hip builds its three; the 33rd word is the
// number of passing elements.
using fsint::Engine;

namespace {

// what every form refuses before it touches the GPU
int filter_rf_args(const uint16_t* array, uint64_t n, uint32_t require, uint32_t exclude, uint32_t include_any, uint32_t exclude_all,
                   const uint8_t* mapq, uint32_t min_mapq, const void* out, int flags)
{
    using namespace fsdrv;
    return refused(check_predicate(require, exclude, min_mapq) || check_predicate_rf(include_any, exclude_all) || check_flags(flags) ||
                   check_array_given(array, n) || check_mapq_given(mapq, n, min_mapq) || check_array_layout(array, n, 2) ||
                   check_counters(out, n, flags));
}

constexpr const char* kFilterRfAlloc = "hipMalloc(filter_rf counters)";

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_u16_filter_rf(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, uint32_t include_any,
                                       uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* d_out,
                                       uint64_t* d_selected, int flags, void* stream)
{
    FS_ENTRY();
    int rc = filter_rf_args(d_array, n, require, exclude, include_any, exclude_all, d_mapq, min_mapq, d_out, flags);
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
    FS_HIP_TRY(fsk_launch_filter_rf(d_array, n, require, exclude, include_any, exclude_all, d_mapq, min_mapq, d_out, d_selected, flags & 3,
                                    fsint::grid_for(*e), s));
    return 0;
}

int FLAGSTATS_hip_device_u16_filter_rf_sync(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, uint32_t include_any,
                                            uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* out,
                                            uint64_t* selected, int flags)
{
    FS_ENTRY();
    int rc = filter_rf_args(d_array, n, require, exclude, include_any, exclude_all, d_mapq, min_mapq, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, flags);
        return 0;
    }
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, nullptr, 0, 0, d_mapq, min_mapq);
    return fsdrv::sync_call(
        in.in, in.count, kFilterRfAlloc, out, selected, flags, fsdrv::kWordAdd,
        [&](Engine& e) { return fsdrv::step_fits(d_array, n, 2, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_filter_rf(d_array, n, require, exclude, include_any, exclude_all, d_mapq, min_mapq, row.d, row.d + 32,
                                            1 | (flags & 2), fsint::grid_for(e), s));
            return 0;
        });
}

int FLAGSTATS_hip_u16_x64_filter_rf(const uint16_t* array, uint64_t n, uint32_t require, uint32_t exclude, uint32_t include_any,
                                    uint32_t exclude_all, const uint8_t* mapq, uint32_t min_mapq, uint64_t* out, uint64_t* selected,
                                    int flags)
{
    FS_ENTRY();
    int rc = filter_rf_args(array, n, require, exclude, include_any, exclude_all, mapq, min_mapq, out, flags);
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
        n, chunk, cap + (mapq_cap + 1) / 2, kFilterRfAlloc, out, selected, flags, fsdrv::kWordAdd,
        [&](Engine& e) { return fsdrv::step_fits(nullptr, cap, 2, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, int sl, uint64_t pos, uint64_t c) {
            const uint32_t grid = fsint::grid_for(e);
            uint8_t* d_mapq = reinterpret_cast<uint8_t*>(e.stage[sl] + cap);
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], array + pos, c * 2, hipMemcpyHostToDevice, e.stream[sl]));
            if (min_mapq) FS_HIP_TRY(hipMemcpyAsync(d_mapq, mapq + pos, c, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_filter_rf(e.stage[sl], c, require, exclude, include_any, exclude_all, d_mapq, min_mapq, row.d, row.d + 32,
                                            mode, grid, e.stream[sl]));
            return 0;
        });
}

}  // extern "C"
