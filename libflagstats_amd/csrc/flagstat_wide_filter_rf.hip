// flagstat_wide_filter_rf.hip -- flagstat of the elements of a FLAG array held as 4-byte or 8-byte little-endian integers (int32 /
// int64 columns, read in place) that pass samtools' whole view predicate on FLAG and MAPQ.  With f(i) = element[i] & 0xFFFF and
//   pass(i) = (f(i) & require) == require && (f(i) & exclude) == 0
//             && (include_any == 0 || (f(i) & include_any) != 0)
//             && (exclude_all == 0 || (f(i) & exclude_all) != exclude_all)
//             && (min_mapq == 0 || mapq[i] >= min_mapq)
// (-f require, -F exclude, --rf / --incl-flags include_any, -G exclude_all, -q min_mapq) the entries give the 32 counters of
// {f(i) : pass(i)}, the number of i that pass, and the OR of element[i] & ~0xFFFF over ALL elements -- passing or not: the mask
// says whether the column is a FLAG column, the predicate sees the low 16 bits only.
//
// Reduction.  As in flagstat_filter_rf.hip the four masks are first reduced exactly on the host (fsk_filter_rf_reduce; its rules
// are stated at its declaration in flagstat_filter_rf.h).  The launcher hands a plain pair to fsk_launch_wide_filter -- the shipped
// kernel at its measured speed -- and an empty predicate to the same launcher as an overlapping pair, which launches nothing and
// READS NO ELEMENT: the mask of such a call is 0 (store form) or untouched (+= form).  Only a residue of at least two free bits in
// --rf or -G reaches the kernel of this file.
//
// Kernel.  fsk::flagstat_count_wide_filter_rf is flagstat_count_wide_filter (flagstat_wide_filter.hip, where the walk, the MAPQ
// loaders, the W = 8 pairing, the edge steps and the epilogue are written out) with one difference: the pass word of a group of 4
// flags is pass4_rf<MAPQ, ANY, ALL> (flagstat_filter_rf_device.h; derived at the top of flagstat_filter_rf.hip) in place of
// pass4<MAPQ> -- 5 more VALU ops per test and group, a group being 16 B (W = 4) or 32 B (W = 8) of the column.  The mask streams
// are fed by narrow_out in front of the predicate, so the residue never sees a bit above bit 15 and `high` never depends on it.
// The kernel is a template on the width, on the MAPQ column and on which of the two tests the residue holds: 12 instantiations.
// A zero-filled position of an edge step passes the all-of test; as in the parent the positions that are no element are cleared
// from the pass word (valid_bits_wide) in front of the count of passing elements.
//
// The step is written here and not as a second form of wide_filter_step_with (flagstat_wide_filter_device.h): that header's
// kernels keep their measured instruction streams by not being touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_filter_device.h"
#include "flagstat_filter_rf.h"
#include "flagstat_filter_rf_device.h"
#include "flagstat_wide.h"
#include "flagstat_wide_device.h"
#include "flagstat_wide_filter.h"
#include "flagstat_wide_filter_device.h"
#include "flagstat_wide_filter_rf.h"

namespace fsk {

constexpr int kWideFilterRfDepth = 8;   // chain depth as K1: epochs of 255 steps

// One step, as wide_filter_step_with (flagstat_wide_filter_device.h) at this kernel's strides, under the residue: 8 vectors of
// 16 B per lane = 32 / W groups of 4 flags each, the whole predicate applied to every group in front of front4.
// ROLL 0 (edge steps): the vectors are in v[], their MAPQ bytes in m[], the bits of their positions that are elements in vb[].
// ROLL 1, 2: K1's schedule 71 through reissue(); the MAPQ bytes of a vector are re-issued right in front of it.
template <int W, bool MAPQ, bool ANY, bool ALL, int ROLL>
__device__ __forceinline__ void wide_filter_rf_step(Lane<kWideFilterRfDepth>& s, const FilterArgs& f, const FilterRfArgs& r,
                                                    uint4 (&v)[kUnroll], uint32_t (&m)[kUnroll], const uint32_t (&vb)[kUnroll],
                                                    uint32_t blk, uint32_t& cnt, uint32_t& or_even, uint32_t& or_odd,
                                                    const uint4* __restrict__ cur, const uint4* __restrict__ next,
                                                    const uint8_t* __restrict__ mcur, const uint8_t* __restrict__ mnext)
{
    constexpr int NIN = 32 / W;
    uint32_t T[NIN], F[NIN], S[NIN];
    uint32_t held = 0, held_mq = 0;   // W = 8: the even vector's P and MAPQ bytes until the odd one's arrive
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        uint32_t p0, p1 = 0, w = 0;
        __builtin_amdgcn_sched_barrier(0);
        narrow_out<W>(v[u], p0, p1, or_even, or_odd);
        if constexpr (MAPQ) {
            w = m[u];
            reissue<ROLL>(u, m, mcur, mnext, kWaveStride * (16 / W), load_mapq_wide<W>);
        }
        reissue<ROLL>(u, v, cur, next, kWaveStride, load_vec<true>);
        __builtin_amdgcn_sched_barrier(0);
        if (W == 8 && (u & 1) == 0) {
            held = p0;
            held_mq = w;
            continue;
        }
        const uint32_t a = W == 4 ? p0 : held, b = W == 4 ? p1 : p0;   // flags 0,1 and 2,3
        uint32_t L = perm(b, a, 0x05040100u), H = perm(b, a, 0x07060302u);
        if (W == 8) w = held_mq | (w << 16);
        uint32_t p = pass4_rf<MAPQ, ANY, ALL>(f, r, L, H, w);
        // in front of the count: a zero-filled position passes the all-of test
        if constexpr (ROLL == 0) p &= nibble_to_bit7(W == 4 ? vb[u] : (vb[u - (W == 8)] | (vb[u] << 2)));
        cnt += __builtin_popcount(p);
        const uint32_t M = perm(0u, 0u, p);   // selector 0x80 -> 0xFF, 0x00 -> source byte 0 = 0x00
        L &= M;
        H &= M;
        const int i = W == 4 ? u : u / 2;
        uint32_t q, k;
        front4(L, H, T[i], q, k);
        F[i] = T[i] & perm(0u, 0xFF00FF00u, q);
        S[i] = perm(0u, 0x84428140u, q) & (k | 0x3F3F3F3Fu);
    }
    const uint32_t ct = wide_tree(T, s.t1, s.t2, s.t4, s.t8);
    const uint32_t cf = wide_tree(F, s.f1, s.f2, s.f4, s.f8);
    const uint32_t cs = wide_tree(S, s.s1, s.s2, s.s4, s.s8);
    chain_push<0, kWideFilterRfDepth>(s, blk, ct, cf, cs);
}

template <int W, bool MAPQ, bool ANY, bool ALL, int ROLL>
__device__ __forceinline__ void wide_filter_rf_step_and_count(Lane<kWideFilterRfDepth>& s, const FilterArgs& f, const FilterRfArgs& r,
                                                              uint4 (&v)[kUnroll], uint32_t (&m)[kUnroll], const uint32_t (&vb)[kUnroll],
                                                              uint32_t& blk, uint32_t& cnt, uint32_t& or_even, uint32_t& or_odd,
                                                              const uint4* __restrict__ cur = nullptr,
                                                              const uint4* __restrict__ next = nullptr,
                                                              const uint8_t* __restrict__ mcur = nullptr,
                                                              const uint8_t* __restrict__ mnext = nullptr)
{
    blk = __builtin_amdgcn_readfirstlane(blk);
    wide_filter_rf_step<W, MAPQ, ANY, ALL, ROLL>(s, f, r, v, m, vb, blk, cnt, or_even, or_odd, cur, next, mcur, mnext);
    end_step<kWideFilterRfDepth>(s, blk);
}

// flagstat_count_wide_filter's arguments (flagstat_wide_filter.hip) with the residue behind `exclude`: the four masks are
// fsk_filter_rf_reduce's, so require & exclude == 0, include_any and exclude_all are disjoint from both, all below 2^16;
// include_any != 0 iff ANY, exclude_all != 0 iff ALL.  min_mapq in 1..255 when MAPQ.  mode: bit 1 superset (bit 0, the store
// form, is the launcher's memset).  selected and high may each be nullptr.
template <int W, bool MAPQ, bool ANY, bool ALL>
__global__ __launch_bounds__(kThreads) void flagstat_count_wide_filter_rf(const uint4* __restrict__ a0, const uint8_t* __restrict__ mq,
                                                                          uint32_t require, uint32_t exclude, uint32_t include_any,
                                                                          uint32_t exclude_all, uint32_t min_mapq, uint64_t lo, uint64_t hi,
                                                                          uint64_t nsteps, uint64_t fast_begin, uint64_t fast_end,
                                                                          uint64_t* __restrict__ out, uint64_t* __restrict__ selected,
                                                                          uint64_t* __restrict__ high, int mode)
{
    static_assert(W == 4 || W == 8, "4-byte or 8-byte elements");
    static_assert(ANY || ALL, "a plain require / exclude pair is flagstat_count_wide_filter's");
    Lane<kWideFilterRfDepth> s;
    lane_init(s);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    constexpr int VPS = kVecPerStep;
    constexpr int US = kWaveStride;
    constexpr int EPV = 16 / W;
    const uint64_t lane_off = static_cast<uint64_t>(wave) * (US * kUnroll) + lane;
    const uint64_t G = gridDim.x;
    const FilterArgs f = filter_args_of(require, exclude, min_mapq);
    const FilterRfArgs r = filter_rf_args_of(include_any, exclude_all);
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
        wide_filter_rf_step_and_count<W, MAPQ, ANY, ALL, 0>(s, f, r, v, m, vb, blk, cnt, or_even, or_odd);
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
            wide_filter_rf_step_and_count<W, MAPQ, ANY, ALL, 1>(s, f, r, v, m, vb, blk, cnt, or_even, or_odd, p, pn, pm, pmn);
            p = pn;
            pm = pmn;
        }
        wide_filter_rf_step_and_count<W, MAPQ, ANY, ALL, 2>(s, f, r, v, m, vb, blk, cnt, or_even, or_odd, p, nullptr, pm, nullptr);
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
namespace {

template <int W, bool MAPQ>
void launch_residue(bool any, bool all, dim3 g, dim3 b, hipStream_t stream, const uint4* a0, const uint8_t* mq, const uint32_t (&m)[4],
                    uint32_t min_mapq, const uint64_t (&geo)[6], uint64_t* d_out32, uint64_t* d_selected, uint64_t* d_high, int mode)
{
    auto* kernel = any && all ? fsk::flagstat_count_wide_filter_rf<W, MAPQ, true, true>
                   : any      ? fsk::flagstat_count_wide_filter_rf<W, MAPQ, true, false>
                              : fsk::flagstat_count_wide_filter_rf<W, MAPQ, false, true>;
    hipLaunchKernelGGL(kernel, g, b, 0, stream, a0, mq, m[0], m[1], m[2], m[3], min_mapq, geo[0], geo[1], geo[2], geo[3], geo[4], d_out32,
                       d_selected, d_high, mode);
}

}  // namespace

extern "C" hipError_t fsk_launch_wide_filter_rf(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                                uint32_t include_any, uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq,
                                                uint64_t* d_out32, uint64_t* d_selected, uint64_t* d_high, int mode, uint32_t grid,
                                                hipStream_t stream)
{
    if (require > 0xFFFFu || exclude > 0xFFFFu || include_any > 0xFFFFu || exclude_all > 0xFFFFu) return hipErrorInvalidValue;
    uint32_t m[4];
    const int kind = fsk_filter_rf_reduce(require, exclude, include_any, exclude_all, m);
    // a plain pair is the shipped kernel's; so is an empty predicate, as the overlapping pair that launcher answers itself
    // without reading an element
    if (kind == 1)
        return fsk_launch_wide_filter(d_array, n, elem_bytes, m[0], m[1], d_mapq, min_mapq, d_out32, d_selected, d_high, mode, grid, stream);
    if (kind == 0)
        return fsk_launch_wide_filter(d_array, n, elem_bytes, 1u, 1u, d_mapq, min_mapq, d_out32, d_selected, d_high, mode, grid, stream);
    if ((elem_bytes != 4 && elem_bytes != 8) || (mode & ~3) || grid == 0 || d_out32 == nullptr || min_mapq > 255u ||
        (n && (d_array == nullptr || (min_mapq && d_mapq == nullptr))))
        return hipErrorInvalidValue;
    uint64_t geo[6];
    hipError_t e = fsk_wide_geometry(reinterpret_cast<uintptr_t>(d_array), n, elem_bytes, grid, geo);
    if (e != hipSuccess) return e;
    if ((mode & 1) && (e = fsdrv::zero_counters(d_out32, d_selected, d_high, stream)) != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(reinterpret_cast<uintptr_t>(d_array) & ~static_cast<uintptr_t>(15));
    // grid position q is element q - lo: its byte is d_mapq[q - lo]
    const uint8_t* mq = min_mapq ? reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_mapq) - geo[0]) : nullptr;
    const dim3 g(static_cast<uint32_t>(geo[5])), b(fsk::kThreads);
    const bool any = m[2] != 0, all = m[3] != 0;
    if (elem_bytes == 4) {
        if (min_mapq)
            launch_residue<4, true>(any, all, g, b, stream, a0, mq, m, min_mapq, geo, d_out32, d_selected, d_high, mode & 2);
        else
            launch_residue<4, false>(any, all, g, b, stream, a0, mq, m, 0u, geo, d_out32, d_selected, d_high, mode & 2);
    } else {
        if (min_mapq)
            launch_residue<8, true>(any, all, g, b, stream, a0, mq, m, min_mapq, geo, d_out32, d_selected, d_high, mode & 2);
        else
            launch_residue<8, false>(any, all, g, b, stream, a0, mq, m, 0u, geo, d_out32, d_selected, d_high, mode & 2);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The three forms are the shared bodies of flagstat_derived_host.h, as flagstat_wide_filter.hip builds its three: the 33rd word is
// the number of passing elements (added in the accumulate form), the 34th the mask (ORed).
using fsint::Engine;

namespace {

// what every form refuses before it touches the GPU: the filtered wide entries' list in its order, the two new masks directly
// behind the predicate
int wide_filter_rf_args(const void* array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude, uint32_t include_any,
                        uint32_t exclude_all, const uint8_t* mapq, uint32_t min_mapq, const void* out, int flags)
{
    using namespace fsdrv;
    return refused(check_elem_bytes(elem_bytes, "elem_bytes 2: 16-bit arrays go to the u16 filter_rf entries "
                                                "(FLAGSTATS_hip_u16_x64_filter_rf, FLAGSTATS_hip_device_u16_filter_rf)") ||
                   check_predicate(require, exclude, min_mapq) || check_predicate_rf(include_any, exclude_all) || check_flags(flags) ||
                   check_array_given(array, n) || check_mapq_given(mapq, n, min_mapq) || check_array_layout(array, n, elem_bytes) ||
                   check_counters(out, n, flags));
}

// no 16-bit value passes the FLAG part: nothing is launched and no element is read, whatever the form
bool passes_nothing(uint32_t require, uint32_t exclude, uint32_t include_any, uint32_t exclude_all)
{
    uint32_t m[4];
    return fsk_filter_rf_reduce(require, exclude, include_any, exclude_all, m) == 0;
}

constexpr const char* kWideFilterRfAlloc = "hipMalloc(wide filter_rf counters)";

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_wide_filter_rf(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                        uint32_t include_any, uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq,
                                        uint64_t* d_out, uint64_t* d_selected, uint64_t* d_high, int flags, void* stream)
{
    FS_ENTRY();
    int rc = wide_filter_rf_args(d_array, n, elem_bytes, require, exclude, include_any, exclude_all, d_mapq, min_mapq, d_out, flags);
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
    FS_HIP_TRY(fsk_launch_wide_filter_rf(d_array, n, elem_bytes, require, exclude, include_any, exclude_all, d_mapq, min_mapq, d_out,
                                         d_selected, d_high, flags & 3, fsint::grid_for(*e), s));
    return 0;
}

int FLAGSTATS_hip_device_wide_filter_rf_sync(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                             uint32_t include_any, uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq,
                                             uint64_t* out, uint64_t* selected, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = wide_filter_rf_args(d_array, n, elem_bytes, require, exclude, include_any, exclude_all, d_mapq, min_mapq, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, high, flags);
        return 0;
    }
    fsdrv::Inputs in;
    in.add_columns(d_array, n, elem_bytes, nullptr, 0, 0, d_mapq, min_mapq);
    return fsdrv::sync_call2(
        in.in, in.count, kWideFilterRfAlloc, out, selected, high, flags,
        [&](Engine& e) { return fsdrv::step_fits(d_array, n, elem_bytes, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_wide_filter_rf(d_array, n, elem_bytes, require, exclude, include_any, exclude_all, d_mapq, min_mapq, row.d,
                                                 row.d + 32, row.d + 33, 1 | (flags & 2), fsint::grid_for(e), s));
            return 0;
        });
}

int FLAGSTATS_hip_wide_x64_filter_rf(const void* array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude, uint32_t include_any,
                                     uint32_t exclude_all, const uint8_t* mapq, uint32_t min_mapq, uint64_t* out, uint64_t* selected,
                                     uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = wide_filter_rf_args(array, n, elem_bytes, require, exclude, include_any, exclude_all, mapq, min_mapq, out, flags);
    if (rc) return rc;
    // a predicate that passes nothing reads no element: nothing crosses the bus
    if (n == 0 || passes_nothing(require, exclude, include_any, exclude_all)) {
        fsdrv::store_nothing(out, selected, high, flags);
        return 0;
    }
    // the array crosses the bus as it is, in chunks of "chunk_flags" * 2 bytes (as FLAGSTATS_hip_wide_x64_filter); a chunk's slice of
    // the MAPQ column rides in the same staging buffer, behind its elements
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const uint64_t chunk = fsdrv::chunk_flags() * 2 / W;               // elements per chunk
    const uint64_t cap = n < chunk ? n : chunk;                         // elements of the largest chunk
    const uint64_t mapq_cap = min_mapq ? cap : 0;                       // bytes of its MAPQ slice
    const int mode = flags & 2;
    const uint8_t* src = static_cast<const uint8_t*>(array);
    return fsdrv::host_call2(
        n, chunk, cap * W / 2 + (mapq_cap + 1) / 2, kWideFilterRfAlloc, out, selected, high, flags,
        [&](Engine& e) { return fsdrv::step_fits(nullptr, cap, elem_bytes, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, int sl, uint64_t pos, uint64_t c) {
            const uint32_t grid = fsint::grid_for(e);
            uint8_t* d_mapq = reinterpret_cast<uint8_t*>(e.stage[sl]) + cap * W;
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], src + pos * W, c * W, hipMemcpyHostToDevice, e.stream[sl]));
            if (min_mapq) FS_HIP_TRY(hipMemcpyAsync(d_mapq, mapq + pos, c, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_wide_filter_rf(e.stage[sl], c, elem_bytes, require, exclude, include_any, exclude_all, d_mapq, min_mapq, row.d,
                                                 row.d + 32, row.d + 33, mode, grid, e.stream[sl]));
            return 0;
        });
}

}  // extern "C"
