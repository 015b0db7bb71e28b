// flagstat_wide_filter_where.hip -- flagstat of the elements of a FLAG array held as 4-byte or 8-byte little-endian integers
// (int32 / int64 columns, read in place) that pass samtools' view filter AND that a selection selects.  With
//   f(i)    = element[i] & 0xFFFF
//   pass(i) = fsk_launch_wide_filter's predicate (flagstat_wide_filter.hip)
//   sel(i)  = fsk_launch_wide_where's selection  (flagstat_wide_where.hip: an LSB-first bitmap at any bit offset, or bytes)
// one kernel gives the 32 counters of {f(i) : pass(i) && sel(i)}, the number of such i, and the OR of element[i] & ~0xFFFF over
// the elements with sel(i) -- passing or not.  That is both parents' rules for the mask at once: the filter never restricts it
// (the predicate sees the low 16 bits only), the selection always does (a null slot's value is unspecified).  With an all-ones
// selection the triple is the filtered wide kernel's, with the empty predicate it is the selected wide kernel's.
//
// The kernel is flagstat_count_wide_filter (geometry, edge and fast steps, schedule 71 through reissue, epochs of 255 steps, the
// direct atomic epilogue) with a third stream beside a vector and its MAPQ bytes: the vector's selection word, addressed exactly
// as flagstat_count_wide_where addresses it (the derivation -- which byte, which shift, which two bytes of a funnelled lane, and
// why step 0 of a funnelled launch goes through the guarded path -- is written out at the top of flagstat_wide_where.hip and is
// not repeated here; the byte form uses load_mapq_wide<W>).  The selection of a vector is issued with the vector, behind its MAPQ
// bytes, and re-issued with it.
//
// Per vector:
//   1. `high` sees selected elements only: every dword of an element that is not selected is zeroed in the vector's registers in
//      front of narrow_out (select_elements of flagstat_wide_where_device.h; its count is not used).
//   2. A zeroed element still passes a predicate without `require` bits, and an unselected element may pass any: the selection's
//      EPV bits are ANDed into the pass word in front of the popcount and of the plane masks (counted_bits / counted_bytes of
//      flagstat_filter_where_device.h).  W = 4: the vector's 4 bits or bytes.  W = 8: a group is the even dwords of vectors u and
//      u + 1, so the even vector's 2 bits (bytes) are held until the odd one's arrive, like its MAPQ bytes.
// Edge steps read the selection element by element, only at positions in [lo, hi), and hand it on from bit 0: a position that
// is no element reads as not selected, so the valid bits of the filtered kernel and the selection bits are one AND here.
// No LDS table, no scratch.
//
// Epilogue.  The parents': finalize_slots<true> with the workgroup's count entering slot 9 (superset), one relaxed agent-scope
// atomic add for the count and one atomic OR for the mask.  No workspace, no second kernel; the store form zeroes counters,
// count and mask in front (one memset when they are one allocation's 34 words).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_filter_device.h"
#include "flagstat_filter_where_device.h"
#include "flagstat_where.h"
#include "flagstat_where_device.h"
#include "flagstat_wide_device.h"
#include "flagstat_wide_filter_device.h"
#include "flagstat_wide_filter_where.h"
#include "flagstat_wide_where.h"
#include "flagstat_wide_where_device.h"

namespace fsk {

constexpr int kWideFilterWhereDepth = 8;   // chain depth as K1: epochs of 255 steps

// One step: the filtered wide step (wide_filter_step_with) with the selection x[u] of vector u applied twice -- to the vector in
// front of its read-out, and to the group's pass word.
// ROLL 0 (edge steps): the vectors are in v[], their MAPQ bytes in m[], their selection in x[] from bit 0 on (sh == 0).
// ROLL 1, 2: K1's schedule 71 as the wide kernel runs it; the MAPQ bytes and the selection of a vector are re-issued right in
// front of it (load_sel).
template <int W, bool MAPQ, int SEL_BITS, int ROLL, typename LoadSel>
__device__ __forceinline__ void wide_filter_where_step_and_count(Lane<kWideFilterWhereDepth>& s, const FilterArgs& f, uint4 (&v)[kUnroll],
                                                                 uint32_t (&m)[kUnroll], uint32_t (&x)[kUnroll], uint32_t& blk, uint32_t sh,
                                                                 uint32_t& cnt, uint32_t& or_even, uint32_t& or_odd, LoadSel&& load_sel,
                                                                 const uint4* __restrict__ cur = nullptr, const uint4* __restrict__ next = nullptr,
                                                                 const uint8_t* __restrict__ mcur = nullptr,
                                                                 const uint8_t* __restrict__ mnext = nullptr,
                                                                 const uint8_t* __restrict__ scur = nullptr,
                                                                 const uint8_t* __restrict__ snext = nullptr)
{
    constexpr int NIN = 32 / W;
    constexpr int EPV = 16 / W;
    constexpr int SS = kWaveStride * EPV / (SEL_BITS == 1 ? 8 : 1);   // selection bytes between a lane's consecutive vectors
    blk = __builtin_amdgcn_readfirstlane(blk);
    uint32_t T[NIN], F[NIN], S[NIN];
    uint32_t held = 0, held_mq = 0, held_sel = 0;   // W = 8: the even vector's P, MAPQ bytes and selection until the odd one's arrive
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        uint32_t p0, p1 = 0, w = 0, unused = 0;
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t xs = x[u];
        select_elements<W, SEL_BITS>(v[u], xs, sh, unused);
        narrow_out<W>(v[u], p0, p1, or_even, or_odd);
        if constexpr (MAPQ) {
            w = m[u];
            reissue<ROLL>(u, m, mcur, mnext, kWaveStride * EPV, load_mapq_wide<W>);
        }
        reissue<ROLL>(u, x, scur, snext, SS, load_sel);
        reissue<ROLL>(u, v, cur, next, kWaveStride, load_vec<true>);
        __builtin_amdgcn_sched_barrier(0);
        // the vector's selection as the pass word takes it: EPV bits from bit 0 on, or EPV bytes
        uint32_t sb = SEL_BITS == 1 ? __builtin_amdgcn_ubfe(xs, sh, EPV) : xs;
        if (W == 8 && (u & 1) == 0) {
            held = p0;
            held_mq = w;
            held_sel = sb;
            continue;
        }
        const uint32_t a = W == 4 ? p0 : held, b = W == 4 ? p1 : p0;   // flags 0,1 and 2,3
        uint32_t L = perm(b, a, 0x05040100u), H = perm(b, a, 0x07060302u);
        if (W == 8) {
            w = held_mq | (w << 16);
            sb = held_sel | (sb << (SEL_BITS == 1 ? EPV : 16));
        }
        uint32_t p = pass4<MAPQ>(f, L, H, w);
        p = SEL_BITS == 1 ? counted_bits(p, sb) : counted_bytes(p, sb);
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
    chain_push<0, kWideFilterWhereDepth>(s, blk, ct, cf, cs);
    end_step<kWideFilterWhereDepth>(s, blk);
}

// a0: 16-B aligned-down base; the caller's elements occupy positions [lo, hi) of its grid of W-byte elements.  mq: the MAPQ
// column on the same grid (the byte of position q is mq[q]; not read when !MAPQ).  sel, shift: the selection on the same grid
// (flagstat_wide_where.hip; FUNNEL: shift != 0 and fast_begin >= 1; byte form: shift unused).  require & exclude == 0 (the
// launcher's business), both below 2^16, min_mapq in 1..255 when MAPQ.  mode: bit 1 superset (bit 0, the store form, is the
// launcher's memset).  selected and high may each be nullptr.
template <int W, bool MAPQ, int SEL_BITS, bool FUNNEL>
__global__ __launch_bounds__(kThreads) void flagstat_count_wide_filter_where(const uint4* __restrict__ a0, const uint8_t* __restrict__ mq,
                                                                             const uint8_t* __restrict__ sel, uint32_t shift, uint32_t require,
                                                                             uint32_t exclude, uint32_t min_mapq, uint64_t lo, uint64_t hi,
                                                                             uint64_t nsteps, uint64_t fast_begin, uint64_t fast_end,
                                                                             uint64_t* __restrict__ out, uint64_t* __restrict__ selected,
                                                                             uint64_t* __restrict__ high, int mode)
{
    static_assert(W == 4 || W == 8, "4-byte or 8-byte elements");
    static_assert(SEL_BITS == 1 || (SEL_BITS == 8 && !FUNNEL), "a bitmap (at a byte boundary of the grid or not) or bytes");
    Lane<kWideFilterWhereDepth> s;
    lane_init(s);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    constexpr int VPS = kVecPerStep;
    constexpr int US = kWaveStride;
    constexpr int EPV = 16 / W;
    constexpr int SDIV = SEL_BITS == 1 ? 8 : 1;   // elements per selection byte
    static_assert(US * EPV % 8 == 0 && VPS * EPV % 8 == 0, "every stride of the walk is a whole number of bitmap bytes");
    const uint32_t lane_vec = wave * (US * kUnroll) + lane;
    const uint64_t lane_off = lane_vec;
    const uint64_t G = gridDim.x;
    const FilterArgs f = filter_args_of(require, exclude, min_mapq);
    uint32_t blk = stagger_start(wave);
    uint32_t cnt = 0;                           // counted elements of this lane
    uint32_t or_even = 0, or_odd = 0;
    // bitmap form: where this lane's bits lie in its byte k and whether they reach into byte k + 1 -- for the whole launch.  The
    // funnelled form loads the two bytes [k + d - 1, k + d] at once and finds its bits 8 (1 - d) places further up.
    const uint32_t lane_bit = lane_vec * EPV + (SEL_BITS == 1 ? shift : 0u);
    const uint32_t d = FUNNEL && (lane_bit & 7u) + EPV > 8u ? 1u : 0u;
    const uint32_t sh = SEL_BITS == 1 ? (lane_bit & 7u) + (FUNNEL ? 8u * (1u - d) : 0u) : 0u;
    auto load_sel = [](const uint8_t* __restrict__ p) __attribute__((always_inline)) {
        if constexpr (FUNNEL) {
            return static_cast<uint32_t>(__builtin_nontemporal_load(reinterpret_cast<const u16_any*>(p)));
        } else if constexpr (SEL_BITS == 1) {
            return static_cast<uint32_t>(__builtin_nontemporal_load(p));
        } else {
            return load_mapq_wide<W>(p);
        }
    };

    auto edge_step = [&](uint64_t st) {
        uint4 v[kUnroll];
        uint32_t m[kUnroll], x[kUnroll];
        const uint64_t j0 = st * VPS + lane_off;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            v[u] = load_guarded_wide<W>(a0, j0 + u * US, lo, hi);
            if constexpr (MAPQ)
                m[u] = load_mapq_wide_guarded<W>(mq, j0 + u * US, lo, hi);
            else
                m[u] = 0;
            if constexpr (SEL_BITS == 1)
                x[u] = load_bits_wide_guarded<W>(sel, shift, j0 + u * US, lo, hi);
            else
                x[u] = load_mapq_wide_guarded<W>(sel, j0 + u * US, lo, hi);
        }
        wide_filter_where_step_and_count<W, MAPQ, SEL_BITS, 0>(s, f, v, m, x, blk, 0u, cnt, or_even, or_odd, load_sel);
    };
    // ragged edge steps (at most the first and the last of the whole array), outside the pipelined loop
    if (fast_begin != 0 && blockIdx.x == 0) edge_step(0);
    if (nsteps > fast_end && nsteps - 1 >= fast_begin && (nsteps - 1) % G == blockIdx.x) edge_step(nsteps - 1);
    // first fully in-range step of this workgroup
    uint64_t st = blockIdx.x;
    if (st < fast_begin) st += G;  // fast_begin is 0 or 1
    if (st < fast_end) {
        constexpr int RD = kRollDistance;
        constexpr int SS = US * EPV / SDIV;
        uint4 v[kUnroll];
        uint32_t m[kUnroll], x[kUnroll];
        const uint4* p = a0 + st * VPS + lane_off;
        const uint8_t* pm = mq + (st * VPS + lane_off) * EPV;
        const uint8_t* ps = sel + st * (VPS * EPV / SDIV) + (SEL_BITS == 1 ? lane_bit >> 3 : lane_bit);
        if constexpr (FUNNEL) ps = ps + d - 1;
        // the first RD vectors, each behind its MAPQ bytes and its selection; the rest is issued as they are consumed
#pragma unroll
        for (int u = 0; u < RD; ++u) {
            if constexpr (MAPQ) m[u] = load_mapq_wide<W>(pm + u * US * EPV);
            x[u] = load_sel(ps + u * SS);
            v[u] = load_vec<true>(p + u * US);
            __builtin_amdgcn_sched_barrier(0);
        }
        for (; st + G < fast_end; st += G) {
            const uint4* pn = p + G * VPS;
            const uint8_t* pmn = pm + G * VPS * EPV;
            const uint8_t* psn = ps + G * (VPS * EPV / SDIV);
            wide_filter_where_step_and_count<W, MAPQ, SEL_BITS, 1>(s, f, v, m, x, blk, sh, cnt, or_even, or_odd, load_sel, p, pn, pm, pmn, ps,
                                                                   psn);
            p = pn;
            pm = pmn;
            ps = psn;
        }
        wide_filter_where_step_and_count<W, MAPQ, SEL_BITS, 2>(s, f, v, m, x, blk, sh, cnt, or_even, or_odd, load_sel, p, nullptr, pm, nullptr,
                                                               ps, nullptr);
    }
    flush(s, blk);

    // wave sums and ORs on the VALU (DPP), then the 4 waves through LDS; word kInternal is the number of counted elements
    constexpr int kWaves = kThreads / 64;
    __shared__ uint32_t red[kWaves][kInternal + 1];
    __shared__ uint32_t hred[kWaves][2];
    __shared__ uint64_t wg_tot[32];
    uint32_t wsum[kInternal + 1];
#pragma unroll
    for (int c = 0; c < kInternal; ++c) wsum[c] = wave_sum_lane63(s.acc[c]);
    wsum[kInternal] = wave_sum_lane63(cnt);
    const uint32_t we = wave_or_lane63(or_even & 0xFFFF0000u);   // the even-dword stream: bits 16-31 of every selected element
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
    // counted elements into slot 9 (superset)
    finalize_slots<true>(wg_tot, out, mode, wg_selected);
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
using fsdrv::where_extent;

namespace {

// the selection forms of one (W, MAPQ): bytes, a bitmap at a byte boundary of the grid, a bitmap funnelled
template <int W, bool MAPQ>
hipError_t launch_form(dim3 g, hipStream_t stream, const uint4* a0, const uint8_t* mq, uintptr_t sel0, uint64_t sel_offset, int sel_bits,
                       uint32_t require, uint32_t exclude, uint32_t min_mapq, uint64_t (&geo)[8], uint64_t* d_out32, uint64_t* d_selected,
                       uint64_t* d_high, int mode)
{
    const dim3 b(fsk::kThreads);
    const uint64_t lo = geo[0];
    const uint8_t* sel;
    uint32_t shift = 0;
#define FSK_WFW_LAUNCH(BITS, FUNNEL)                                                                                                       \
    hipLaunchKernelGGL((fsk::flagstat_count_wide_filter_where<W, MAPQ, BITS, FUNNEL>), g, b, 0, stream, a0, mq, sel, shift, require, exclude, \
                       min_mapq, geo[0], geo[1], geo[2], geo[3], geo[4], d_out32, d_selected, d_high, mode)
    if (sel_bits == 8) {
        // grid position q is element q - lo: its byte is d_sel[sel_offset + q - lo]
        sel = reinterpret_cast<const uint8_t*>(sel0 + sel_offset - lo);
        FSK_WFW_LAUNCH(8, false);
    } else {
        // grid position q is element q - lo: its bit is bit sel_offset + q - lo = q + (bit0 - 8), where bit0 >= 1
        const uint64_t bit0 = sel_offset + 8 - lo;
        sel = reinterpret_cast<const uint8_t*>(sel0 + (bit0 >> 3) - 1);
        shift = static_cast<uint32_t>(bit0 & 7);
        if (shift == 0) {
            FSK_WFW_LAUNCH(1, false);
        } else {
            // the funnelled form reaches one selection byte in front of a fast vector's: step 0 goes through the guarded path
            geo[3] = 1;
            if (geo[4] < 1) geo[4] = 1;
            FSK_WFW_LAUNCH(1, true);
        }
    }
#undef FSK_WFW_LAUNCH
    return hipGetLastError();
}

}  // namespace

extern "C" hipError_t fsk_launch_wide_filter_where(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                                   const uint8_t* d_mapq, uint32_t min_mapq, const void* d_sel, uint64_t sel_offset,
                                                   int sel_bits, uint64_t* d_out32, uint64_t* d_selected, uint64_t* d_high, int mode,
                                                   uint32_t grid, hipStream_t stream)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || (sel_bits != 1 && sel_bits != 8) || (mode & ~3) || grid == 0 || d_out32 == nullptr ||
        require > 0xFFFFu || exclude > 0xFFFFu || min_mapq > 255u ||
        (n && (d_array == nullptr || d_sel == nullptr || (min_mapq && d_mapq == nullptr))))
        return hipErrorInvalidValue;
    uint64_t geo[8];
    hipError_t e = fsk_wide_where_geometry(reinterpret_cast<uintptr_t>(d_array), n, elem_bytes, sel_offset, sel_bits, grid, geo);
    if (e != hipSuccess) return e;
    if ((mode & 1) && (e = fsdrv::zero_counters(d_out32, d_selected, d_high, stream)) != hipSuccess) return e;
    // a bit both required and excluded: no flag passes (samtools accepts the pair); the kernel's test assumes a disjoint pair.
    // Nothing is launched, so nothing is read and the mask stays what the store form's memset or the caller left there.
    if (n == 0 || (require & exclude)) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(reinterpret_cast<uintptr_t>(d_array) & ~static_cast<uintptr_t>(15));
    // grid position q is element q - lo: its byte is d_mapq[q - lo]
    const uint8_t* mq = min_mapq ? reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_mapq) - geo[0]) : nullptr;
    const dim3 g(static_cast<uint32_t>(geo[5]));
    const uintptr_t sel0 = reinterpret_cast<uintptr_t>(d_sel);
    const int m = mode & 2;
    if (elem_bytes == 4) {
        if (min_mapq) return launch_form<4, true>(g, stream, a0, mq, sel0, sel_offset, sel_bits, require, exclude, min_mapq, geo, d_out32, d_selected, d_high, m);
        return launch_form<4, false>(g, stream, a0, mq, sel0, sel_offset, sel_bits, require, exclude, 0u, geo, d_out32, d_selected, d_high, m);
    }
    if (min_mapq) return launch_form<8, true>(g, stream, a0, mq, sel0, sel_offset, sel_bits, require, exclude, min_mapq, geo, d_out32, d_selected, d_high, m);
    return launch_form<8, false>(g, stream, a0, mq, sel0, sel_offset, sel_bits, require, exclude, 0u, geo, d_out32, d_selected, d_high, m);
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The three forms are the shared bodies of flagstat_derived_host.h with two trailing words: the 33rd is the number of counted
// elements (added in the accumulate form), the 34th the mask of the selected elements (ORed).
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU: the union of what the filtered and the selected wide entries refuse, in
// their words
int wide_filter_where_args(const void* array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude, const uint8_t* mapq,
                           uint32_t min_mapq, const void* sel, uint64_t sel_offset, int sel_bits, const void* out, int flags)
{
    using namespace fsdrv;
    return refused(check_elem_bytes(elem_bytes, "elem_bytes 2: 16-bit arrays go to the u16 filter_where entries "
                                                "(FLAGSTATS_hip_u16_x64_filter_where, FLAGSTATS_hip_device_u16_filter_where)") ||
                   check_predicate(require, exclude, min_mapq) || check_sel_bits(sel_bits) || check_flags(flags) ||
                   check_array_given(array, n) || check_mapq_given(mapq, n, min_mapq) ||
                   check_sel_given(sel, n, "NULL selection with n > 0 (no selection: the filtered wide entries FLAGSTATS_hip_wide_x64_filter, "
                                           "FLAGSTATS_hip_device_wide_filter)") ||
                   check_array_layout(array, n, elem_bytes) || check_sel_range(sel_offset, n) || check_counters(out, n, flags));
}

constexpr const char* kWideFilterWhereAlloc = "hipMalloc(wide filter_where counters)";

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_wide_filter_where(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                           const uint8_t* d_mapq, uint32_t min_mapq, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                           uint64_t* d_out, uint64_t* d_selected, uint64_t* d_high, int flags, void* stream)
{
    FS_ENTRY();
    int rc = wide_filter_where_args(d_array, n, elem_bytes, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits, d_out, flags);
    if (rc) return rc;
    if (n == 0 && !(flags & 1)) return 0;
    const fsdrv::DeviceWord words[] = {{d_selected, "d_selected", "the count is added with a device atomic"},
                                       {d_high, "d_high", "the mask is ORed with a device atomic"}};
    fsdrv::Inputs in;
    in.add_columns(d_array, n, elem_bytes, d_sel, sel_offset, sel_bits, d_mapq, min_mapq);
    fsdrv::DeviceCall call;
    if ((rc = call.open(d_out, words, 2, in.in, in.count, stream))) return rc;
    Engine* e = call.e;
    hipStream_t s = call.s;
    if ((rc = fsdrv::step_fits(d_array, n, elem_bytes, fsint::grid_for(*e)))) return rc;
    if ((rc = fsdrv::check_extents(d_out, words, 2, in.in, in.count))) return rc;
    FS_HIP_TRY(fsk_launch_wide_filter_where(d_array, n, elem_bytes, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits, d_out,
                                            d_selected, d_high, flags & 3, fsint::grid_for(*e), s));
    return 0;
}

int FLAGSTATS_hip_device_wide_filter_where_sync(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                                const uint8_t* d_mapq, uint32_t min_mapq, const void* d_sel, uint64_t sel_offset,
                                                int sel_bits, uint64_t* out, uint64_t* selected, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = wide_filter_where_args(d_array, n, elem_bytes, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, high, flags);
        return 0;
    }
    fsdrv::Inputs in;
    in.add_columns(d_array, n, elem_bytes, d_sel, sel_offset, sel_bits, d_mapq, min_mapq);
    return fsdrv::sync_call2(
        in.in, in.count, kWideFilterWhereAlloc, out, selected, high, flags,
        [&](Engine& e) { return fsdrv::step_fits(d_array, n, elem_bytes, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_wide_filter_where(d_array, n, elem_bytes, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits,
                                                    row.d, row.d + 32, row.d + 33, 1 | (flags & 2), fsint::grid_for(e), s));
            return 0;
        });
}

int FLAGSTATS_hip_wide_x64_filter_where(const void* array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                        const uint8_t* mapq, uint32_t min_mapq, const void* sel, uint64_t sel_offset, int sel_bits,
                                        uint64_t* out, uint64_t* selected, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = wide_filter_where_args(array, n, elem_bytes, require, exclude, mapq, min_mapq, sel, sel_offset, sel_bits, out, flags);
    if (rc) return rc;
    // an overlapping pair passes nothing and reads nothing: nothing crosses the bus
    if (n == 0 || (require & exclude)) {
        fsdrv::store_nothing(out, selected, high, flags);
        return 0;
    }
    // the array crosses the bus as it is, in chunks of "chunk_flags" * 2 bytes (as FLAGSTATS_hip_wide_x64); a chunk's slices of the
    // MAPQ column and of the selection ride in the same staging buffer, behind its elements: the column's first, then the
    // selection's -- a bitmap slice from the byte that holds the chunk's first bit (the launch then starts (sel_offset + pos) & 7
    // bits into it)
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const uint64_t chunk = fsdrv::chunk_flags() * 2 / W;               // elements per chunk
    const uint64_t cap = n < chunk ? n : chunk;                         // elements of the largest chunk
    const uint64_t mapq_slot = min_mapq ? (cap + 1) / 2 : 0;            // its MAPQ slice, in uint16
    const uint64_t sel_cap = sel_bits == 1 ? (cap + 7) / 8 + 1 : cap;   // bytes of its selection slice
    const int mode = flags & 2;
    const uint8_t* src = static_cast<const uint8_t*>(array);
    const uint8_t* sel_src = static_cast<const uint8_t*>(sel);
    return fsdrv::host_call2(
        n, chunk, cap * W / 2 + mapq_slot + (sel_cap + 1) / 2, kWideFilterWhereAlloc, out, selected, high, flags,
        [&](Engine& e) { return fsdrv::step_fits(nullptr, cap, elem_bytes, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, int sl, uint64_t pos, uint64_t c) {
            const uint32_t grid = fsint::grid_for(e);
            uint64_t first, bytes;
            where_extent(c, sel_offset + pos, sel_bits, &first, &bytes);
            uint8_t* d_mapq = reinterpret_cast<uint8_t*>(e.stage[sl]) + cap * W;
            uint8_t* d_sel = d_mapq + mapq_slot * 2;
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], src + pos * W, c * W, hipMemcpyHostToDevice, e.stream[sl]));
            if (min_mapq) FS_HIP_TRY(hipMemcpyAsync(d_mapq, mapq + pos, c, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(hipMemcpyAsync(d_sel, sel_src + first, bytes, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_wide_filter_where(e.stage[sl], c, elem_bytes, require, exclude, d_mapq, min_mapq, d_sel,
                                                    sel_bits == 1 ? (sel_offset + pos) & 7 : 0, sel_bits, row.d, row.d + 32, row.d + 33, mode,
                                                    grid, e.stream[sl]));
            return 0;
        });
}

}  // extern "C"
