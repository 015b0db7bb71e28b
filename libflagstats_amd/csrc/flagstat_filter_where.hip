// flagstat_filter_where.hip -- flagstat of the elements of a uint16 FLAG array that pass samtools' view filter AND that a
// selection selects: the 32 counters of {flag[i] : pass(i) && sel(i)} and the number of such i, where pass is
// flagstat_filter.hip's predicate (-f require, -F exclude, -q min_mapq over a uint8 MAPQ column) and sel is flagstat_where.hip's
// selection (an LSB-first bitmap that may start at any bit, or one byte per element).  The case of a FLAG column with a validity
// bitmap, or of a region / read-group mask, under -F 0x904 -q 30: one pass over the array, the column and the selection, one
// kernel, nothing of the combined mask in memory.
//
// Geometry, step split, edge and fast steps, rolling schedule 71 and epilogue are the filtered kernel's (flagstat_count_filter,
// flagstat_filter.hip), which are K1's.  The MAPQ column is addressed as there, the selection as in flagstat_where.hip: the
// launcher hands the kernel `sel` such that the 8 bits of grid vector j start at bit `shift` of sel[j] (bitmap; shift == 0 takes
// one byte per vector, otherwise two are funnelled together: a template parameter, so three selection forms) or such that its 8
// bytes are sel[8 j .. 8 j + 8) (byte form, at any alignment).  On a fast step the selection of a vector is loaded right behind
// its MAPQ bytes and in front of the vector itself, and read out with it; an edge step (step 0 of an array that starts inside a
// vector, the last step) goes through the guarded loaders, which touch no byte that holds no element and hand the bitmap's bits
// back at bit 0, so an edge step runs unfunnelled.
//
// Predicate.  The filtered kernel's test ends in p = ~q & 0x80808080 (pass4, flagstat_filter_device.h): 0x80 per passing flag
// of 4.  The selection joins p in registers (counted_bits / counted_bytes of flagstat_filter_where_device.h, shared with
// flagstat_segments_filter_where.hip), in front of the popcount and of the v_perm_b32 that makes the byte masks; the
// bitmap kernel's selector table in LDS is not used (the pass word exists anyway, and the table would cost LDS traffic per
// vector on top).  Per 4 flags:
//   bitmap:  b  = v_bfe_u32(x, sh | sh + 4, 4)       the 4 selection bits (shift 0: v_and_b32 / v_lshrrev_b32)
//            e  = (b * 0x204081) << 7                v_mul_lo_u32    bit k of b on bits k, k + 7, k + 14, k + 21 (bit 8 k = bit k),
//                                                                    then to bit 7 of byte k: one multiply by 0x10204080
//            p &= e                                  v_and_b32       (p has bit 7 of every byte only)
//            = 3 VALU ops
//   bytes:   t  = (x & 0x7F..) + 0x7F..              v_and_b32, v_add_u32       bit 7 of a byte: one of its bits 0-6 is set
//            p &= t | x                              v_bitop3_b32               bit 7 of a byte of t | x: the byte is not zero
//            = 3 VALU ops
// Positions of an edge vector outside [lo, hi) come back from the guarded selection loader as not selected, so the filtered
// kernel's valid_bits are not needed: p is cleared there by the selection itself.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_filter_device.h"
#include "flagstat_filter_where.h"
#include "flagstat_filter_where_device.h"
#include "flagstat_where.h"
#include "flagstat_where_device.h"

namespace fsk {

constexpr int kFilterWhereDepth = 8;  // chain depth as K1: epochs of 255 steps

// One step: 8 vectors of 16 B per lane = 64 flags through K1's tree (tree_step, flagstat_count_core.h), predicate and selection
// applied in the per-vector front.  ROLL 0 (edge steps): the vectors are in v[], their MAPQ bytes in m[], their selection in
// x[] (bitmap: at bit 0, sh == 0).  ROLL 1, 2: K1's schedule 71 (reissue, same header); the MAPQ bytes and the selection of a
// vector are loaded right in front of it and read out with it.
template <bool MAPQ, int SEL_BITS, bool FUNNEL, int ROLL>
__device__ __forceinline__ void filter_where_step_and_count(Lane<kFilterWhereDepth>& s, const FilterArgs& f, uint4 (&v)[kUnroll],
                                                            uint2 (&m)[kUnroll], typename SelWord<SEL_BITS>::type (&x)[kUnroll],
                                                            uint32_t& blk, uint32_t sh, uint32_t& cnt,
                                                            const uint4* __restrict__ cur = nullptr, const uint4* __restrict__ next = nullptr,
                                                            const uint8_t* __restrict__ mcur = nullptr,
                                                            const uint8_t* __restrict__ mnext = nullptr,
                                                            const uint8_t* __restrict__ scur = nullptr,
                                                            const uint8_t* __restrict__ snext = nullptr)
{
    constexpr int SS = SEL_BITS == 1 ? kWaveStride : kWaveStride * 8;   // selection bytes between a lane's consecutive vectors
    blk = __builtin_amdgcn_readfirstlane(blk);
    tree_step<kFilterWhereDepth>(s, blk, [&](int uu, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        split_out(v[uu], L0, H0, L1, H1);
        uint2 w = make_uint2(0, 0);
        if constexpr (MAPQ) {
            w = m[uu];
            reissue<ROLL>(uu, m, mcur, mnext, kWaveStride * 8, load_mapq);
        }
        const typename SelWord<SEL_BITS>::type c = x[uu];
        reissue<ROLL>(uu, x, scur, snext, SS, load_sel<SEL_BITS, FUNNEL>);
        reissue<ROLL>(uu, v, cur, next, kWaveStride, load_vec<true>);
        uint32_t p0 = pass4<MAPQ>(f, L0, H0, w.x);
        uint32_t p1 = pass4<MAPQ>(f, L1, H1, w.y);
        if constexpr (SEL_BITS == 1) {
            p0 = counted_bits(p0, __builtin_amdgcn_ubfe(c, sh, 4));
            p1 = counted_bits(p1, __builtin_amdgcn_ubfe(c, sh + 4, 4));
        } else {
            p0 = counted_bytes(p0, c.x);
            p1 = counted_bytes(p1, c.y);
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
    end_step<kFilterWhereDepth>(s, blk);
}

// a0: 16-B aligned-down base; the caller's flags occupy positions [lo, hi) of its grid.  mq: the MAPQ column on the same grid
// (the byte of position q is mq[q]; not read when !MAPQ).  sel, shift: the selection on the same grid (see above; FUNNEL:
// shift != 0).  require & exclude == 0 (the launcher's business), both below 2^16, min_mapq in 1..255 when MAPQ.  mode: bit 1
// superset (bit 0, the store form, is the launcher's memset).  selected may be nullptr.
template <bool MAPQ, int SEL_BITS, bool FUNNEL>
__global__ __launch_bounds__(kThreads) void flagstat_filter_where(const uint4* __restrict__ a0, const uint8_t* __restrict__ mq,
                                                                  const uint8_t* __restrict__ sel, uint32_t shift, uint32_t require,
                                                                  uint32_t exclude, uint32_t min_mapq, uint64_t lo, uint64_t hi,
                                                                  uint64_t nsteps, uint64_t fast_begin, uint64_t fast_end,
                                                                  uint64_t* __restrict__ out, uint64_t* __restrict__ selected, int mode)
{
    static_assert(SEL_BITS == 1 || (SEL_BITS == 8 && !FUNNEL), "a bitmap (at a byte boundary of the grid or not) or bytes");
    typedef typename SelWord<SEL_BITS>::type sel_t;
    Lane<kFilterWhereDepth> s;
    lane_init(s);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    constexpr int VPS = kVecPerStep;
    constexpr int US = kWaveStride;
    constexpr int SB = SEL_BITS == 1 ? 1 : 8;   // selection bytes per vector
    const uint64_t lane_off = static_cast<uint64_t>(wave) * (US * kUnroll) + lane;
    const uint64_t G = gridDim.x;
    const FilterArgs f = filter_args_of(require, exclude, min_mapq);
    uint32_t blk = stagger_start(wave);
    uint32_t cnt = 0;                           // counted elements of this lane
    const uint32_t sh = FUNNEL ? __builtin_amdgcn_readfirstlane(shift) : 0u;

    auto edge_step = [&](uint64_t st) {
        uint4 v[kUnroll];
        uint2 m[kUnroll];
        sel_t x[kUnroll];
        const uint64_t j0 = st * VPS + lane_off;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            v[u] = load_guarded(a0, j0 + u * US, lo, hi);
            if constexpr (MAPQ)
                m[u] = load_mapq_guarded(mq, j0 + u * US, lo, hi);
            else
                m[u] = make_uint2(0, 0);
            x[u] = load_sel_guarded<SEL_BITS>(sel, shift, j0 + u * US, lo, hi);
        }
        filter_where_step_and_count<MAPQ, SEL_BITS, false, 0>(s, f, v, m, x, blk, 0u, cnt);
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
        sel_t x[kUnroll];
        const uint4* p = a0 + st * VPS + lane_off;
        const uint8_t* pm = mq + (st * VPS + lane_off) * 8;
        const uint8_t* ps = sel + (st * VPS + lane_off) * SB;
        // the first RD vectors; the rest is issued as they are consumed
#pragma unroll
        for (int u = 0; u < RD; ++u) {
            if constexpr (MAPQ) m[u] = load_mapq(pm + u * US * 8);
            x[u] = load_sel<SEL_BITS, FUNNEL>(ps + u * US * SB);
            v[u] = load_vec<true>(p + u * US);
            __builtin_amdgcn_sched_barrier(0);
        }
        for (; st + G < fast_end; st += G) {
            const uint4* pn = p + G * VPS;
            const uint8_t* pmn = pm + G * VPS * 8;
            const uint8_t* psn = ps + G * VPS * SB;
            filter_where_step_and_count<MAPQ, SEL_BITS, FUNNEL, 1>(s, f, v, m, x, blk, sh, cnt, p, pn, pm, pmn, ps, psn);
            p = pn;
            pm = pmn;
            ps = psn;
        }
        filter_where_step_and_count<MAPQ, SEL_BITS, FUNNEL, 2>(s, f, v, m, x, blk, sh, cnt, p, nullptr, pm, nullptr, ps, nullptr);
    }
    flush(s, blk);

    // wave sums on the VALU (DPP), then the 4 waves through LDS; word kInternal is the number of counted elements
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
    // counted elements into slot 9 (superset)
    finalize_slots<true>(wg_tot, out, mode, wg_selected);
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
using fsdrv::where_extent;

namespace {

template <bool MAPQ>
hipError_t launch_form(const dim3& g, hipStream_t stream, const uint4* a0, const uint8_t* mq, uintptr_t sel0, uint64_t sel_offset,
                       int sel_bits, uint32_t require, uint32_t exclude, uint32_t min_mapq, const uint64_t* geo, uint64_t* d_out32,
                       uint64_t* d_selected, int mode)
{
    const dim3 b(fsk::kThreads);
    const uint64_t lo = geo[0];
    if (sel_bits == 8) {
        // grid position q is element q - lo: its byte is d_sel[sel_offset + q - lo]
        const uint8_t* sel = reinterpret_cast<const uint8_t*>(sel0 + sel_offset - lo);
        hipLaunchKernelGGL((fsk::flagstat_filter_where<MAPQ, 8, false>), g, b, 0, stream, a0, mq, sel, 0u, require, exclude, min_mapq, geo[0],
                           geo[1], geo[2], geo[3], geo[4], d_out32, d_selected, mode);
        return hipGetLastError();
    }
    // grid position q is element q - lo: its bit is bit sel_offset + q - lo = q + (bit0 - 8), where bit0 >= 1
    const uint64_t bit0 = sel_offset + 8 - lo;
    const uint8_t* sel = reinterpret_cast<const uint8_t*>(sel0 + (bit0 >> 3) - 1);
    const uint32_t shift = static_cast<uint32_t>(bit0 & 7);
    if (shift == 0)
        hipLaunchKernelGGL((fsk::flagstat_filter_where<MAPQ, 1, false>), g, b, 0, stream, a0, mq, sel, 0u, require, exclude, min_mapq, geo[0],
                           geo[1], geo[2], geo[3], geo[4], d_out32, d_selected, mode);
    else
        hipLaunchKernelGGL((fsk::flagstat_filter_where<MAPQ, 1, true>), g, b, 0, stream, a0, mq, sel, shift, require, exclude, min_mapq,
                           geo[0], geo[1], geo[2], geo[3], geo[4], d_out32, d_selected, mode);
    return hipGetLastError();
}

}  // namespace

extern "C" hipError_t fsk_launch_filter_where(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                              uint32_t min_mapq, const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* d_out32,
                                              uint64_t* d_selected, int mode, uint32_t grid, hipStream_t stream)
{
    if ((sel_bits != 1 && sel_bits != 8) || (mode & ~3) || grid == 0 || d_out32 == nullptr || require > 0xFFFFu || exclude > 0xFFFFu ||
        min_mapq > 255u || (n && (d_array == nullptr || d_sel == nullptr || (min_mapq && d_mapq == nullptr))))
        return hipErrorInvalidValue;
    uint64_t geo[8];
    hipError_t e = fsk_where_geometry(reinterpret_cast<uintptr_t>(d_array), n, sel_offset, sel_bits, grid, geo);
    if (e != hipSuccess) return e;
    if ((mode & 1) && (e = fsdrv::zero_counters(d_out32, d_selected, stream)) != hipSuccess) return e;
    // a bit both required and excluded: no flag passes (samtools accepts the pair); the kernel's test assumes a disjoint pair
    if (n == 0 || (require & exclude)) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(reinterpret_cast<uintptr_t>(d_array) & ~static_cast<uintptr_t>(15));
    const dim3 g(static_cast<uint32_t>(geo[5]));
    const uintptr_t sel0 = reinterpret_cast<uintptr_t>(d_sel);
    if (min_mapq) {
        // grid position q is element q - lo: its byte is d_mapq[q - lo]
        const uint8_t* mq = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_mapq) - geo[0]);
        return launch_form<true>(g, stream, a0, mq, sel0, sel_offset, sel_bits, require, exclude, min_mapq, geo, d_out32, d_selected, mode & 2);
    }
    return launch_form<false>(g, stream, a0, nullptr, sel0, sel_offset, sel_bits, require, exclude, 0u, geo, d_out32, d_selected, mode & 2);
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The three forms are the shared bodies of flagstat_derived_host.h; the 33rd word is the number of counted elements.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU: the filtered entries' refusals, then the `where` entries', in their texts
int filter_where_args(const uint16_t* array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* mapq, uint32_t min_mapq,
                      const void* sel, uint64_t sel_offset, int sel_bits, const void* out, int flags)
{
    using namespace fsdrv;
    return refused(check_predicate(require, exclude, min_mapq) || check_sel_bits(sel_bits) || check_flags(flags) ||
                   check_array_given(array, n) || check_mapq_given(mapq, n, min_mapq) || check_sel_given(sel, n) ||
                   check_array_layout(array, n, 2) || check_sel_range(sel_offset, n) || check_counters(out, n, flags));
}

constexpr const char* kFilterWhereAlloc = "hipMalloc(filter_where counters)";

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_u16_filter_where(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                          uint32_t min_mapq, const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* d_out,
                                          uint64_t* d_selected, int flags, void* stream)
{
    FS_ENTRY();
    int rc = filter_where_args(d_array, n, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits, d_out, flags);
    if (rc) return rc;
    if (n == 0 && !(flags & 1)) return 0;
    const fsdrv::DeviceWord word{d_selected, "d_selected", "the count is added with a device atomic"};
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, d_sel, sel_offset, sel_bits, d_mapq, min_mapq);
    fsdrv::DeviceCall call;
    if ((rc = call.open(d_out, word, in.in, in.count, stream))) return rc;
    Engine* e = call.e;
    hipStream_t s = call.s;
    if ((rc = fsdrv::step_fits(d_array, n, 2, fsint::grid_for(*e)))) return rc;
    if ((rc = fsdrv::check_extents(d_out, word, in.in, in.count))) return rc;
    FS_HIP_TRY(fsk_launch_filter_where(d_array, n, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits, d_out, d_selected,
                                       flags & 3, fsint::grid_for(*e), s));
    return 0;
}

int FLAGSTATS_hip_device_u16_filter_where_sync(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude,
                                               const uint8_t* d_mapq, uint32_t min_mapq, const void* d_sel, uint64_t sel_offset,
                                               int sel_bits, uint64_t* out, uint64_t* selected, int flags)
{
    FS_ENTRY();
    int rc = filter_where_args(d_array, n, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, flags);
        return 0;
    }
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, d_sel, sel_offset, sel_bits, d_mapq, min_mapq);
    return fsdrv::sync_call(
        in.in, in.count, kFilterWhereAlloc, out, selected, flags, fsdrv::kWordAdd,
        [&](Engine& e) { return fsdrv::step_fits(d_array, n, 2, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_filter_where(d_array, n, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits, row.d, row.d + 32,
                                               1 | (flags & 2), fsint::grid_for(e), s));
            return 0;
        });
}

int FLAGSTATS_hip_u16_x64_filter_where(const uint16_t* array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* mapq,
                                       uint32_t min_mapq, const void* sel, uint64_t sel_offset, int sel_bits, uint64_t* out,
                                       uint64_t* selected, int flags)
{
    FS_ENTRY();
    int rc = filter_where_args(array, n, require, exclude, mapq, min_mapq, sel, sel_offset, sel_bits, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, flags);
        return 0;
    }
    // a chunk's slices of the MAPQ column and of the selection ride in the same staging buffer, behind the flags: the column's
    // first, then the selection's -- a bitmap slice from the byte that holds the chunk's first bit (the launch then starts
    // (sel_offset + pos) & 7 bits into it)
    const uint64_t chunk = fsdrv::chunk_flags();
    const uint64_t cap = n < chunk ? n : chunk;                         // flags of the largest chunk
    const uint64_t mapq_slot = min_mapq ? (cap + 1) / 2 : 0;            // its MAPQ slice, in uint16
    const uint64_t sel_cap = sel_bits == 1 ? (cap + 7) / 8 + 1 : cap;   // bytes of its selection slice
    const int mode = flags & 2;
    const uint8_t* sel_src = static_cast<const uint8_t*>(sel);
    return fsdrv::host_call(
        n, chunk, cap + mapq_slot + (sel_cap + 1) / 2, kFilterWhereAlloc, out, selected, flags, fsdrv::kWordAdd,
        [&](Engine& e) { return fsdrv::step_fits(nullptr, cap, 2, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, int sl, uint64_t pos, uint64_t c) {
            const uint32_t grid = fsint::grid_for(e);
            uint64_t first, bytes;
            where_extent(c, sel_offset + pos, sel_bits, &first, &bytes);
            uint8_t* d_mapq = reinterpret_cast<uint8_t*>(e.stage[sl] + cap);
            uint8_t* d_sel = reinterpret_cast<uint8_t*>(e.stage[sl] + cap + mapq_slot);
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], array + pos, c * 2, hipMemcpyHostToDevice, e.stream[sl]));
            if (min_mapq) FS_HIP_TRY(hipMemcpyAsync(d_mapq, mapq + pos, c, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(hipMemcpyAsync(d_sel, sel_src + first, bytes, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_filter_where(e.stage[sl], c, require, exclude, d_mapq, min_mapq, d_sel,
                                               sel_bits == 1 ? (sel_offset + pos) & 7 : 0, sel_bits, row.d, row.d + 32, mode, grid,
                                               e.stream[sl]));
            return 0;
        });
}

}  // extern "C"
