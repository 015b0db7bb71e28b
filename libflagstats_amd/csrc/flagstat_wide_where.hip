// flagstat_wide_where.hip -- flagstat of the SELECTED elements of a FLAG array held as 4-byte or 8-byte little-endian integers
// (int32 / int64 columns, read in place): the 32 counters of {element[i] & 0xFFFF : sel(i)}, the number of selected elements and
// the OR of element[i] & ~0xFFFF over the SELECTED elements only, in one pass over the array and its selection.  The selection
// is an LSB-first bitmap (Arrow's validity layout) that may start at any bit, or one byte per element (numpy / torch bool).
//
// `high` covers the selected elements only -- unlike the filtered kernel (flagstat_wide_filter.hip), whose mask covers every
// element read.  A selection is typically a validity bitmap, and the value of a null slot is unspecified: whatever lies there
// must neither count nor set a mask bit.
//
// It is the wide kernel's walk (flagstat_wide.hip: geometry, 32 KiB steps, guarded loaders on the edge steps, schedule 71
// through reissue, wide_step_with, epochs of 255 steps, the direct atomic epilogue) with ONE thing in front of narrow_out: every
// dword of an element that is not selected is zeroed in the vector's registers.  A zero element counts nothing in any slot and
// sets no bit in the v_or3_b32 mask stream, so counters and mask both see the selected elements only.
//
// Selection, bitmap form.  The selection is addressed on the array's 16-byte grid.  A vector holds EPV = 16 / W elements (4 or
// 2).  With bit0 = sel_offset + 8 - lo (>= 1: lo < EPV) the bit of grid position q is bit q + bit0 - 8 of d_sel; the launcher
// hands the kernel sel = d_sel + (bit0 >> 3) - 1 and shift = bit0 & 7, so that it is bit q + shift of `sel`, and the EPV bits of
// grid vector j start at bit j * EPV + shift.  A lane's vectors are j = step * 2048 + wave * 512 + u * 64 + lane: everything but
// `lane` is a multiple of 8 / EPV vectors = 8 bits, so with b = lane * EPV + shift
//     byte index   k  = (j - lane) * EPV / 8 + (b >> 3)
//     shift        sh = b & 7                    -- constant for the lane over the whole launch
//     straddle     d  = sh + EPV > 8 ? 1 : 0     -- constant too: whether the lane's bits reach into byte k + 1
// At shift == 0, sh is lane * EPV & 7 <= 8 - EPV: no lane straddles, and a lane loads the one byte sel[k] (FUNNEL false).
// Otherwise (FUNNEL) a lane loads TWO ADJACENT bytes with one unaligned 16-bit load -- which two depends on the lane:
//     d == 1:  [k, k + 1], its bits from bit sh on          d == 0:  [k - 1, k], its bits from bit sh + 8 on
// No over-read, by construction.  Unlike the uint16 kernel's 8 bits, 4 bits at sh <= 4 lie in one byte, so a blind load of
// [k, k + 1] would read one byte past the bitmap where the last fast vector ends the array, and a blind [k - 1, k] one byte in
// front of it where the first fast vector begins it.  On a fast step every position of a vector is an element, so sel[k] holds
// an element's bit; sel[k + 1] is addressed only where the vector's own last bit lies in it; sel[k - 1] holds the bits of the 8
// grid positions in front of the vector's, and the launcher makes those elements: it runs step 0 of a funnelled launch through
// the guarded path whatever the step split says (fast_begin = 1), so a fast vector is never among the first 2,048 of the grid
// and the positions in front of it are at least lo (< EPV) and below hi.  tests/test_wide_where_host.py models exactly these
// addresses.  (Two byte loads, sel[k] and sel[k + d], need no such step but cost a third vector-memory instruction per vector:
// 1.17-1.21 of the wide kernel's time where this form takes what the plain form takes; joined at the place of the load, so
// that every re-issue waited for itself, 1.57-1.66.)
// Selection, byte form.  sel is such that the byte of grid position q is sel[q]; the EPV bytes of a vector come with one
// unaligned load of 4 or 2 bytes (the filtered kernel's MAPQ loaders: the layout is the same), and a byte selects if it is not
// zero (bytes_mask's test, flagstat_where_device.h).
// The selection of a vector is issued right in front of the vector itself (reissue), so it has arrived when the vector has.
// Per vector the keep masks cost v_bfe_u32 (bitmap) or four ops of bytes_mask (bytes), v_bcnt_u32_b32 for the number selected
// (the lane's 22nd counter), then v_bfe_i32 per element and v_and_b32 per dword.  No LDS table, no scratch.
// Edge steps read the selection element by element, only at positions in [lo, hi), and hand it on as EPV bits / bytes from bit 0.
//
// Epilogue.  The filtered wide kernel's: finalize_slots<true> with the workgroup's `selected` entering slot 9 (superset), one
// relaxed agent-scope atomic add for `selected` and one atomic OR for the mask.  No workspace, no second kernel; the store form
// zeroes counters, count and mask in front (one memset when they are one allocation's 34 words).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_where.h"
#include "flagstat_where_device.h"
#include "flagstat_wide_device.h"
#include "flagstat_wide_filter_device.h"
#include "flagstat_wide_where.h"
#include "flagstat_wide_where_device.h"

namespace fsk {

constexpr int kWideWhereDepth = 8;   // chain depth as K1: epochs of 255 steps

// (load_bits_wide_guarded, the bitmap loader of the edge steps, and select_elements, the zeroing of the elements a selection word
// leaves out, are flagstat_wide_where_device.h's: flagstat_segments_wide_where.hip runs them too.)

// One step (wide_step_with) with the selection m[u] of vector u applied in front of its read-out.
// ROLL 0 (edge steps): the vectors are in v[], their selection in m[] from bit 0 on (sh == 0).  ROLL 1, 2: K1's schedule 71 as
// the wide kernel runs it; the selection of a vector is re-issued right in front of it (load_sel).
template <int W, int SEL_BITS, int ROLL, typename LoadSel>
__device__ __forceinline__ void wide_where_step_and_count(Lane<kWideWhereDepth>& s, uint4 (&v)[kUnroll], uint32_t (&m)[kUnroll], uint32_t& blk,
                                                          uint32_t sh, uint32_t& cnt, uint32_t& or_even, uint32_t& or_odd, LoadSel&& load_sel,
                                                          const uint4* __restrict__ cur = nullptr, const uint4* __restrict__ next = nullptr,
                                                          const uint8_t* __restrict__ scur = nullptr, const uint8_t* __restrict__ snext = nullptr)
{
    constexpr int SS = kWaveStride * (16 / W) / (SEL_BITS == 1 ? 8 : 1);   // selection bytes between a lane's consecutive vectors
    blk = __builtin_amdgcn_readfirstlane(blk);
    wide_step_with<W>(
        s, v, blk, or_even, or_odd,
        [&](int u) __attribute__((always_inline)) {
            reissue<ROLL>(u, m, scur, snext, SS, load_sel);
            reissue<ROLL>(u, v, cur, next, kWaveStride, load_vec<true>);
        },
        [&](int u) __attribute__((always_inline)) { select_elements<W, SEL_BITS>(v[u], m[u], sh, cnt); });
    end_step<kWideWhereDepth>(s, blk);
}

// a0: 16-B aligned-down base; the caller's elements occupy positions [lo, hi) of its grid of W-byte elements.  sel, shift: the
// selection on the same grid (see above; FUNNEL: shift != 0; byte form: shift unused).  mode: bit 1 superset (bit 0, the store
// form, is the launcher's memset).  selected and high may each be nullptr.
template <int W, int SEL_BITS, bool FUNNEL>
__global__ __launch_bounds__(kThreads) void flagstat_count_wide_where(const uint4* __restrict__ a0, const uint8_t* __restrict__ sel, uint32_t shift,
                                                                      uint64_t lo, uint64_t hi, uint64_t nsteps, uint64_t fast_begin,
                                                                      uint64_t fast_end, uint64_t* __restrict__ out,
                                                                      uint64_t* __restrict__ selected, uint64_t* __restrict__ high, int mode)
{
    static_assert(W == 4 || W == 8, "4-byte or 8-byte elements");
    static_assert(SEL_BITS == 1 || (SEL_BITS == 8 && !FUNNEL), "a bitmap (at a byte boundary of the grid or not) or bytes");
    Lane<kWideWhereDepth> s;
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
    uint32_t blk = stagger_start(wave);
    uint32_t cnt = 0;                           // selected elements of this lane
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
        uint32_t m[kUnroll];
        const uint64_t j0 = st * VPS + lane_off;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            v[u] = load_guarded_wide<W>(a0, j0 + u * US, lo, hi);
            if constexpr (SEL_BITS == 1)
                m[u] = load_bits_wide_guarded<W>(sel, shift, j0 + u * US, lo, hi);
            else
                m[u] = load_mapq_wide_guarded<W>(sel, j0 + u * US, lo, hi);
        }
        wide_where_step_and_count<W, SEL_BITS, 0>(s, v, m, blk, 0u, cnt, or_even, or_odd, load_sel);
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
        uint32_t m[kUnroll];
        const uint4* p = a0 + st * VPS + lane_off;
        const uint8_t* ps = sel + st * (VPS * EPV / SDIV) + (SEL_BITS == 1 ? lane_bit >> 3 : lane_bit);
        if constexpr (FUNNEL) ps = ps + d - 1;
        // the first RD vectors, each behind its selection; the rest is issued as they are consumed
#pragma unroll
        for (int u = 0; u < RD; ++u) {
            m[u] = load_sel(ps + u * SS);
            v[u] = load_vec<true>(p + u * US);
            __builtin_amdgcn_sched_barrier(0);
        }
        for (; st + G < fast_end; st += G) {
            const uint4* pn = p + G * VPS;
            const uint8_t* psn = ps + G * (VPS * EPV / SDIV);
            wide_where_step_and_count<W, SEL_BITS, 1>(s, v, m, blk, sh, cnt, or_even, or_odd, load_sel, p, pn, ps, psn);
            p = pn;
            ps = psn;
        }
        wide_where_step_and_count<W, SEL_BITS, 2>(s, v, m, blk, sh, cnt, or_even, or_odd, load_sel, p, nullptr, ps, nullptr);
    }
    flush(s, blk);

    // wave sums and ORs on the VALU (DPP), then the 4 waves through LDS; word kInternal is the number of selected elements
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
    // selected elements into slot 9 (superset)
    finalize_slots<true>(wg_tot, out, mode, wg_selected);
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
using fsdrv::where_extent;

// Host-side geometry: the shared step split (flagstat_derived_host.h) at W = 4 or 8; geo[6], geo[7]: the selection bytes
// [geo[6], geo[7]) hold the bit or byte of an element.
extern "C" hipError_t fsk_wide_where_geometry(uint64_t address, uint64_t n, int elem_bytes, uint64_t sel_offset, int sel_bits, uint32_t grid,
                                              uint64_t* geo)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || (sel_bits != 1 && sel_bits != 8) || geo == nullptr) return hipErrorInvalidValue;
    geo[6] = geo[7] = 0;
    const hipError_t e = fsdrv::step_split(address, n, elem_bytes, grid, geo);
    if (e != hipSuccess || n == 0) return e;
    if (sel_offset > ~0ull - 64 - n) {  // sel_offset + n must be an index
        for (int i = 0; i < 6; ++i) geo[i] = 0;
        return hipErrorInvalidValue;
    }
    uint64_t first, bytes;
    where_extent(n, sel_offset, sel_bits, &first, &bytes);
    geo[6] = first;
    geo[7] = first + bytes;
    return hipSuccess;
}

extern "C" hipError_t fsk_launch_wide_where(const void* d_array, uint64_t n, int elem_bytes, const void* d_sel, uint64_t sel_offset,
                                            int sel_bits, uint64_t* d_out32, uint64_t* d_selected, uint64_t* d_high, int mode, uint32_t grid,
                                            hipStream_t stream)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || (sel_bits != 1 && sel_bits != 8) || (mode & ~3) || grid == 0 || d_out32 == nullptr ||
        (n && (d_array == nullptr || d_sel == nullptr)))
        return hipErrorInvalidValue;
    uint64_t geo[8];
    hipError_t e = fsk_wide_where_geometry(reinterpret_cast<uintptr_t>(d_array), n, elem_bytes, sel_offset, sel_bits, grid, geo);
    if (e != hipSuccess) return e;
    if ((mode & 1) && (e = fsdrv::zero_counters(d_out32, d_selected, d_high, stream)) != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(reinterpret_cast<uintptr_t>(d_array) & ~static_cast<uintptr_t>(15));
    const dim3 g(static_cast<uint32_t>(geo[5])), b(fsk::kThreads);
    const uintptr_t sel0 = reinterpret_cast<uintptr_t>(d_sel);
    const uint64_t lo = geo[0];
    const uint8_t* sel;
    uint32_t shift = 0;
#define FSK_WW_LAUNCH(W, BITS, FUNNEL)                                                                                                   \
    hipLaunchKernelGGL((fsk::flagstat_count_wide_where<W, BITS, FUNNEL>), g, b, 0, stream, a0, sel, shift, geo[0], geo[1], geo[2], geo[3], \
                       geo[4], d_out32, d_selected, d_high, mode & 2)
    if (sel_bits == 8) {
        // grid position q is element q - lo: its byte is d_sel[sel_offset + q - lo]
        sel = reinterpret_cast<const uint8_t*>(sel0 + sel_offset - lo);
        if (elem_bytes == 4)
            FSK_WW_LAUNCH(4, 8, false);
        else
            FSK_WW_LAUNCH(8, 8, false);
    } else {
        // grid position q is element q - lo: its bit is bit sel_offset + q - lo = q + (bit0 - 8), where bit0 >= 1
        const uint64_t bit0 = sel_offset + 8 - lo;
        sel = reinterpret_cast<const uint8_t*>(sel0 + (bit0 >> 3) - 1);
        shift = static_cast<uint32_t>(bit0 & 7);
        if (shift != 0) {
            // the funnelled form reaches one selection byte in front of a fast vector's: step 0 goes through the guarded path
            geo[3] = 1;
            if (geo[4] < 1) geo[4] = 1;
        }
        if (elem_bytes == 4) {
            if (shift == 0)
                FSK_WW_LAUNCH(4, 1, false);
            else
                FSK_WW_LAUNCH(4, 1, true);
        } else {
            if (shift == 0)
                FSK_WW_LAUNCH(8, 1, false);
            else
                FSK_WW_LAUNCH(8, 1, true);
        }
    }
#undef FSK_WW_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The three forms are the shared bodies of flagstat_derived_host.h with two trailing words: the 33rd is the number of selected
// elements (added in the accumulate form), the 34th the mask of the selected elements (ORed).
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU: the wide entries' list, then the where entries', in their words
int wide_where_args(const void* array, uint64_t n, int elem_bytes, const void* sel, uint64_t sel_offset, int sel_bits, const void* out,
                    int flags)
{
    using namespace fsdrv;
    return refused(check_elem_bytes(elem_bytes, "elem_bytes 2: 16-bit arrays go to the u16 where entries (FLAGSTATS_hip_u16_x64_where, "
                                                "FLAGSTATS_hip_device_u16_where)") ||
                   check_sel_bits(sel_bits) || check_flags(flags) || check_array_given(array, n) || check_sel_given(sel, n) ||
                   check_array_layout(array, n, elem_bytes) || check_sel_range(sel_offset, n) || check_counters(out, n, flags));
}

constexpr const char* kWideWhereAlloc = "hipMalloc(wide where counters)";

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_wide_where(const void* d_array, uint64_t n, int elem_bytes, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                    uint64_t* d_out, uint64_t* d_selected, uint64_t* d_high, int flags, void* stream)
{
    FS_ENTRY();
    int rc = wide_where_args(d_array, n, elem_bytes, d_sel, sel_offset, sel_bits, d_out, flags);
    if (rc) return rc;
    if (n == 0 && !(flags & 1)) return 0;
    const fsdrv::DeviceWord words[] = {{d_selected, "d_selected", "the count is added with a device atomic"},
                                       {d_high, "d_high", "the mask is ORed with a device atomic"}};
    fsdrv::Inputs in;
    in.add_columns(d_array, n, elem_bytes, d_sel, sel_offset, sel_bits, nullptr, 0);
    fsdrv::DeviceCall call;
    if ((rc = call.open(d_out, words, 2, in.in, in.count, stream))) return rc;
    Engine* e = call.e;
    hipStream_t s = call.s;
    if ((rc = fsdrv::step_fits(d_array, n, elem_bytes, fsint::grid_for(*e)))) return rc;
    if ((rc = fsdrv::check_extents(d_out, words, 2, in.in, in.count))) return rc;
    FS_HIP_TRY(fsk_launch_wide_where(d_array, n, elem_bytes, d_sel, sel_offset, sel_bits, d_out, d_selected, d_high, flags & 3,
                                     fsint::grid_for(*e), s));
    return 0;
}

int FLAGSTATS_hip_device_wide_where_sync(const void* d_array, uint64_t n, int elem_bytes, const void* d_sel, uint64_t sel_offset,
                                         int sel_bits, uint64_t* out, uint64_t* selected, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = wide_where_args(d_array, n, elem_bytes, d_sel, sel_offset, sel_bits, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, high, flags);
        return 0;
    }
    fsdrv::Inputs in;
    in.add_columns(d_array, n, elem_bytes, d_sel, sel_offset, sel_bits, nullptr, 0);
    return fsdrv::sync_call2(
        in.in, in.count, kWideWhereAlloc, out, selected, high, flags,
        [&](Engine& e) { return fsdrv::step_fits(d_array, n, elem_bytes, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_wide_where(d_array, n, elem_bytes, d_sel, sel_offset, sel_bits, row.d, row.d + 32, row.d + 33,
                                             1 | (flags & 2), fsint::grid_for(e), s));
            return 0;
        });
}

int FLAGSTATS_hip_wide_x64_where(const void* array, uint64_t n, int elem_bytes, const void* sel, uint64_t sel_offset, int sel_bits,
                                 uint64_t* out, uint64_t* selected, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = wide_where_args(array, n, elem_bytes, sel, sel_offset, sel_bits, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, high, flags);
        return 0;
    }
    // the array crosses the bus as it is, in chunks of "chunk_flags" * 2 bytes (as FLAGSTATS_hip_wide_x64); a chunk's slice of the
    // selection rides in the same staging buffer, behind its elements: a bitmap slice from the byte that holds the chunk's first
    // bit (the launch then starts (sel_offset + pos) & 7 bits into it)
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const uint64_t chunk = fsdrv::chunk_flags() * 2 / W;               // elements per chunk
    const uint64_t cap = n < chunk ? n : chunk;                         // elements of the largest chunk
    const uint64_t sel_cap = sel_bits == 1 ? (cap + 7) / 8 + 1 : cap;   // bytes of its selection slice
    const int mode = flags & 2;
    const uint8_t* src = static_cast<const uint8_t*>(array);
    const uint8_t* sel_src = static_cast<const uint8_t*>(sel);
    return fsdrv::host_call2(
        n, chunk, cap * W / 2 + (sel_cap + 1) / 2, kWideWhereAlloc, out, selected, high, flags,
        [&](Engine& e) { return fsdrv::step_fits(nullptr, cap, elem_bytes, fsint::grid_for(e)); },
        [&](Engine& e, fsdrv::Row& row, int sl, uint64_t pos, uint64_t c) {
            const uint32_t grid = fsint::grid_for(e);
            uint64_t first, bytes;
            where_extent(c, sel_offset + pos, sel_bits, &first, &bytes);
            uint8_t* d_sel = reinterpret_cast<uint8_t*>(e.stage[sl]) + cap * W;
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], src + pos * W, c * W, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(hipMemcpyAsync(d_sel, sel_src + first, bytes, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_wide_where(e.stage[sl], c, elem_bytes, d_sel, sel_bits == 1 ? (sel_offset + pos) & 7 : 0, sel_bits, row.d,
                                             row.d + 32, row.d + 33, mode, grid, e.stream[sl]));
            return 0;
        });
}

}  // extern "C"
