// flagstat_where.hip -- flagstat of the SELECTED elements of a uint16 FLAG array: the 32 counters of {array[i] : sel(i)} and the
// number of selected elements, in one pass over the array and its selection.  The selection is an LSB-first bitmap (Arrow's
// validity layout, np.packbits(bitorder="little")) that may start at any bit, or one byte per element (numpy / torch bool).
//
// Geometry.  K1's: the array is addressed on the 16-byte grid of its aligned-down base, the caller's flags occupy positions
// [lo, hi) of it, and it is cut into steps of 32 KiB = 16,384 flags (256 lanes x 8 vectors of 16 B); workgroup b takes the head
// edge step (b == 0), the tail edge step, then the fully covered steps b, b + G, ...; each wave owns a contiguous 8 KiB of a
// step and lane l takes vectors u * 64 + l.  Edge steps go through guarded, zero-filling loaders; fast steps through K1's
// rolling load schedule (schedule 71: a vector's registers are re-issued for the vector six places on as soon as it has been
// read out: reissue, flagstat_count_core.h).  tests/steps_oracle.StepSplit(addr % 16, n, grid) is the step split.
//
// Selection.  The selection is addressed on the array's grid as well: the launcher hands the kernel a base pointer `sel` such
// that the 8 bits of grid vector j start at bit `sh` of sel[j] (bitmap: sh == 0 takes one byte per vector, otherwise two are
// funnelled together), or such that its 8 bytes are sel[8 j .. 8 j + 8) (byte form, at any alignment).  A wave's 64 lanes thus
// read 64 consecutive selection bytes (bitmap) or 512 (bytes) per vector.
// A zero flag counts nothing in any slot, so selecting is zeroing the flags that are not selected, in front of front4:
//   bitmap:  in the split itself.  split_out's four v_perm_b32 take their byte selectors from registers, and a selector byte
//            of 0x0C writes 0x00: a 256-entry table in LDS (4 KiB, built by the workgroup's 256 threads) maps a selection
//            byte to the four selectors with 0x0C for every flag that is not selected.  Per vector of 8 flags: v_lshlrev_b32
//            (the table offset; v_bfe_u32 in front when the bits are funnelled), ds_read_b128, v_bcnt_u32_b32 for the number
//            selected -- 1 to 1.5 VALU ops per 4 flags.  The selection byte of a vector is loaded one vector ahead of it, so
//            the table read of vector u + 1 is in flight while vector u is counted.
//   bytes:   on the byte planes L and H.  Per 4 flags v_and_b32, v_add_u32, v_bitop3_b32 (bit 7 of a byte = byte != 0),
//            v_lshrrev_b32, v_perm_b32 (0x01 -> 0xFF), 2 x v_and_b32 (some fused by the compiler with front4's first ops),
//            v_bcnt_u32_b32: 8 VALU ops.  This form moves 3 B per flag and runs at 0.955-0.962 of K1's byte rate
//            (profiles/r10/where_sweep.log); whether these ops or its loads cost the 4 % has not been determined.
// Only selection bytes that hold the bit or byte of an element in [0, n) are read: on fast steps every position of a vector
// is an element; the edge loaders look at [lo, hi) for every byte.
//
// Epilogue.  K1's direct one: every workgroup maps its 21 totals to the 32 slots and adds them to out[32] with relaxed
// agent-scope atomics; its number of selected elements goes to *selected the same way and is what the superset slot 9 takes for
// the flag count (the per-workgroup partial sums wrap modulo 2^64: slot_value, flagstat_count_core.h).  No workspace, no second
// kernel; the store form zeroes counters and `selected` in front (one memset).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_where.h"
#include "flagstat_where_device.h"

namespace fsk {

constexpr int kWhereDepth = 8;        // chain depth as K1: epochs of 255 steps

// the byte masks of a vector's flags 0-3 and 4-7 in the byte form; the number selected is added to cnt
__device__ __forceinline__ void bytes_masks(const uint2& w, uint32_t& M0, uint32_t& M1, uint32_t& cnt)
{
    uint32_t s0, s1;
    M0 = bytes_mask(w.x, s0);
    M1 = bytes_mask(w.y, s1);
    cnt += __builtin_popcount(s0);
    cnt += __builtin_popcount(s1);
}

// One step: 8 vectors of 16 B per lane = 64 flags through K1's tree (tree_step, flagstat_count_core.h), the selection applied in
// the per-vector front.  ROLL 0: the vectors are in v[], their selection in m[].  ROLL 1, 2: K1's schedule 71 (reissue, same
// header).  Byte form: the selection of a vector is loaded right in front of it and read out with it.  Bitmap form: the
// selection byte of a vector is loaded in front of the vector BEFORE it, so that it has arrived when that one has; its table
// entry is fetched while that one is being counted and handed on in `entry` (on entry: vector 0's; on exit, ROLL 1: the next
// step's vector 0's).
template <int SEL_BITS, bool FUNNEL, int ROLL>
__device__ __forceinline__ void where_step_and_count(Lane<kWhereDepth>& s, uint4 (&v)[kUnroll], typename SelWord<SEL_BITS>::type (&m)[kUnroll],
                                                     uint4& entry, const uint4* __restrict__ lut, uint32_t& blk, uint32_t sh, uint32_t& cnt,
                                                     const uint4* __restrict__ cur = nullptr, const uint4* __restrict__ next = nullptr,
                                                     const uint8_t* __restrict__ scur = nullptr, const uint8_t* __restrict__ snext = nullptr)
{
    constexpr int SS = SEL_BITS == 1 ? kWaveStride : kWaveStride * 8;   // selection bytes between a lane's consecutive vectors
    blk = __builtin_amdgcn_readfirstlane(blk);
    tree_step<kWhereDepth>(s, blk, [&](int uu, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (SEL_BITS == 1) {
            split_out_selected(v[uu], entry, L0, H0, L1, H1);
            if (uu + 1 < kUnroll || ROLL == 1) entry = lookup(lut, m[(uu + 1) % kUnroll], sh, cnt);
            reissue<ROLL, 1>(uu, m, scur, snext, SS, load_sel<SEL_BITS, FUNNEL>);
        } else {
            split_out(v[uu], L0, H0, L1, H1);
            const uint2 w = m[uu];
            reissue<ROLL>(uu, m, scur, snext, SS, load_sel<SEL_BITS, FUNNEL>);
            uint32_t M0, M1;
            bytes_masks(w, M0, M1, cnt);
            L0 &= M0;
            H0 &= M0;
            L1 &= M1;
            H1 &= M1;
        }
        reissue<ROLL>(uu, v, cur, next, kWaveStride, load_vec<true>);
        __builtin_amdgcn_sched_barrier(0);
    });
    end_step<kWhereDepth>(s, blk);
}

// a0: 16-B aligned-down base; the caller's flags occupy positions [lo, hi) of its grid.  sel, shift: the selection on the same
// grid (see above; FUNNEL: shift != 0).  mode: bit 1 superset (bit 0, the store form, is the launcher's memset).  selected may
// be nullptr.
template <int SEL_BITS, bool FUNNEL = false>
__global__ __launch_bounds__(kThreads) void flagstat_count_where(const uint4* __restrict__ a0, const uint8_t* __restrict__ sel, uint32_t shift,
                                                                 uint64_t lo, uint64_t hi, uint64_t nsteps, uint64_t fast_begin,
                                                                 uint64_t fast_end, uint64_t* __restrict__ out,
                                                                 uint64_t* __restrict__ selected, int mode)
{
    static_assert(SEL_BITS == 1 || (SEL_BITS == 8 && !FUNNEL), "a bitmap (at a byte boundary of the grid or not) or bytes");
    static_assert(kThreads == 256, "one thread per table entry");
    typedef typename SelWord<SEL_BITS>::type sel_t;
    __shared__ uint4 lut[SEL_BITS == 1 ? 256 : 1];
    if constexpr (SEL_BITS == 1) {
        lut[threadIdx.x] = selector_entry(threadIdx.x);
        __syncthreads();
    }
    Lane<kWhereDepth> s;
    lane_init(s);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    constexpr int VPS = kVecPerStep;
    constexpr int US = kWaveStride;
    constexpr int SB = SEL_BITS == 1 ? 1 : 8;   // selection bytes per vector
    const uint64_t lane_off = static_cast<uint64_t>(wave) * (US * kUnroll) + lane;
    const uint64_t G = gridDim.x;
    uint32_t blk = stagger_start(wave);
    uint32_t cnt = 0;                           // selected elements of this lane
    const uint32_t sh = FUNNEL ? __builtin_amdgcn_readfirstlane(shift) : 0u;
    uint4 entry = make_uint4(0, 0, 0, 0);       // bitmap form: the table entry of the vector that is counted next

    auto edge_step = [&](uint64_t st) {
        uint4 v[kUnroll];
        sel_t m[kUnroll];
        const uint64_t j0 = st * VPS + lane_off;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            v[u] = load_guarded(a0, j0 + u * US, lo, hi);
            m[u] = load_sel_guarded<SEL_BITS>(sel, shift, j0 + u * US, lo, hi);
        }
        if constexpr (SEL_BITS == 1) entry = lookup(lut, m[0], 0u, cnt);
        where_step_and_count<SEL_BITS, false, 0>(s, v, m, entry, lut, blk, 0u, cnt);
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
        sel_t m[kUnroll];
        const uint4* p = a0 + st * VPS + lane_off;
        const uint8_t* ps = sel + (st * VPS + lane_off) * SB;
        // the first RD vectors; the rest is issued as they are consumed.  The bitmap's bytes run one vector ahead.
        if constexpr (SEL_BITS == 1) m[0] = load_sel<SEL_BITS, FUNNEL>(ps);
#pragma unroll
        for (int u = 0; u < RD; ++u) {
            if constexpr (SEL_BITS == 1)
                m[u + 1] = load_sel<SEL_BITS, FUNNEL>(ps + (u + 1) * US * SB);
            else
                m[u] = load_sel<SEL_BITS, FUNNEL>(ps + u * US * SB);
            v[u] = load_vec<true>(p + u * US);
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (SEL_BITS == 1) entry = lookup(lut, m[0], sh, cnt);
        for (; st + G < fast_end; st += G) {
            const uint4* pn = p + G * VPS;
            const uint8_t* psn = ps + G * VPS * SB;
            where_step_and_count<SEL_BITS, FUNNEL, 1>(s, v, m, entry, lut, blk, sh, cnt, p, pn, ps, psn);
            p = pn;
            ps = psn;
        }
        where_step_and_count<SEL_BITS, FUNNEL, 2>(s, v, m, entry, lut, blk, sh, cnt, p, nullptr, ps, nullptr);
    }
    flush(s, blk);

    // wave sums on the VALU (DPP), then the 4 waves through LDS; word kInternal is the number of selected elements
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
    // selected elements into slot 9 (superset)
    finalize_slots<true>(wg_tot, out, mode, wg_selected);
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
using fsdrv::where_extent;

// Host-side geometry: the shared step split (flagstat_derived_host.h) at W = 2; geo[6], geo[7]: the selection bytes
// [geo[6], geo[7]) hold the bit or byte of an element.
extern "C" hipError_t fsk_where_geometry(uint64_t address, uint64_t n, uint64_t sel_offset, int sel_bits, uint32_t grid, uint64_t* geo)
{
    if ((sel_bits != 1 && sel_bits != 8) || geo == nullptr) return hipErrorInvalidValue;
    geo[6] = geo[7] = 0;
    const hipError_t e = fsdrv::step_split(address, n, 2, grid, geo);
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

extern "C" hipError_t fsk_launch_where(const uint16_t* d_array, uint64_t n, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                       uint64_t* d_out32, uint64_t* d_selected, int mode, uint32_t grid, hipStream_t stream)
{
    if ((sel_bits != 1 && sel_bits != 8) || (mode & ~3) || grid == 0 || d_out32 == nullptr || (n && (d_array == nullptr || d_sel == nullptr)))
        return hipErrorInvalidValue;
    uint64_t geo[8];
    hipError_t e = fsk_where_geometry(reinterpret_cast<uintptr_t>(d_array), n, sel_offset, sel_bits, grid, geo);
    if (e != hipSuccess) return e;
    if ((mode & 1) && (e = fsdrv::zero_counters(d_out32, d_selected, stream)) != hipSuccess) return e;
    if (n == 0) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(reinterpret_cast<uintptr_t>(d_array) & ~static_cast<uintptr_t>(15));
    const dim3 g(static_cast<uint32_t>(geo[5])), b(fsk::kThreads);
    const uintptr_t sel0 = reinterpret_cast<uintptr_t>(d_sel);
    const uint64_t lo = geo[0];
    if (sel_bits == 8) {
        // grid position q is element q - lo: its byte is d_sel[sel_offset + q - lo]
        const uint8_t* sel = reinterpret_cast<const uint8_t*>(sel0 + sel_offset - lo);
        hipLaunchKernelGGL((fsk::flagstat_count_where<8>), g, b, 0, stream, a0, sel, 0u, geo[0], geo[1], geo[2], geo[3], geo[4], d_out32,
                           d_selected, mode & 2);
        return hipGetLastError();
    }
    // grid position q is element q - lo: its bit is bit sel_offset + q - lo = q + (bit0 - 8), where bit0 >= 1
    const uint64_t bit0 = sel_offset + 8 - lo;
    const uint8_t* sel = reinterpret_cast<const uint8_t*>(sel0 + (bit0 >> 3) - 1);
    const uint32_t shift = static_cast<uint32_t>(bit0 & 7);
    if (shift == 0)
        hipLaunchKernelGGL((fsk::flagstat_count_where<1, false>), g, b, 0, stream, a0, sel, 0u, geo[0], geo[1], geo[2], geo[3], geo[4],
                           d_out32, d_selected, mode & 2);
    else
        hipLaunchKernelGGL((fsk::flagstat_count_where<1, true>), g, b, 0, stream, a0, sel, shift, geo[0], geo[1], geo[2], geo[3], geo[4],
                           d_out32, d_selected, mode & 2);
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The three forms are the shared bodies of flagstat_derived_host.h; the 33rd word is the number of selected elements.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU
int where_args(const uint16_t* array, uint64_t n, const void* sel, uint64_t sel_offset, int sel_bits, const void* out, int flags)
{
    using namespace fsdrv;
    return refused(check_sel_bits(sel_bits) || check_flags(flags) || check_array_given(array, n) || check_sel_given(sel, n) ||
                   check_array_layout(array, n, 2) || check_sel_range(sel_offset, n) || check_counters(out, n, flags));
}

constexpr const char* kWhereAlloc = "hipMalloc(where counters)";

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_u16_where(const uint16_t* d_array, uint64_t n, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                   uint64_t* d_out, uint64_t* d_selected, int flags, void* stream)
{
    FS_ENTRY();
    int rc = where_args(d_array, n, d_sel, sel_offset, sel_bits, d_out, flags);
    if (rc) return rc;
    if (n == 0 && !(flags & 1)) return 0;
    const fsdrv::DeviceWord word{d_selected, "d_selected", "the count is added with a device atomic"};
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, d_sel, sel_offset, sel_bits, nullptr, 0);
    fsdrv::DeviceCall call;
    if ((rc = call.open(d_out, word, in.in, in.count, stream))) return rc;
    if ((rc = fsdrv::check_extents(d_out, word, in.in, in.count))) return rc;
    Engine* e = call.e;
    hipStream_t s = call.s;
    FS_HIP_TRY(fsk_launch_where(d_array, n, d_sel, sel_offset, sel_bits, d_out, d_selected, flags & 3, fsint::grid_for(*e), s));
    return 0;
}

int FLAGSTATS_hip_device_u16_where_sync(const uint16_t* d_array, uint64_t n, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                        uint64_t* out, uint64_t* selected, int flags)
{
    FS_ENTRY();
    int rc = where_args(d_array, n, d_sel, sel_offset, sel_bits, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, flags);
        return 0;
    }
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, d_sel, sel_offset, sel_bits, nullptr, 0);
    return fsdrv::sync_call(in.in, in.count, kWhereAlloc, out, selected, flags, fsdrv::kWordAdd, fsdrv::fits_always,
                            [&](Engine& e, fsdrv::Row& row, hipStream_t s) {
                                FS_HIP_TRY(fsk_launch_where(d_array, n, d_sel, sel_offset, sel_bits, row.d, row.d + 32, 1 | (flags & 2), fsint::grid_for(e), s));
                                return 0;
                            });
}

int FLAGSTATS_hip_u16_x64_where(const uint16_t* array, uint64_t n, const void* sel, uint64_t sel_offset, int sel_bits, uint64_t* out,
                                uint64_t* selected, int flags)
{
    FS_ENTRY();
    int rc = where_args(array, n, sel, sel_offset, sel_bits, out, flags);
    if (rc) return rc;
    if (n == 0) {
        fsdrv::store_nothing(out, selected, flags);
        return 0;
    }
    // a chunk's slice of the selection rides in the same staging buffer, behind the flags: a bitmap slice from the byte that
    // holds the chunk's first bit (the launch then starts (sel_offset + pos) & 7 bits into it)
    const uint64_t chunk = fsdrv::chunk_flags();
    const uint64_t cap = n < chunk ? n : chunk;                         // flags of the largest chunk
    const uint64_t sel_cap = sel_bits == 1 ? (cap + 7) / 8 + 1 : cap;   // bytes of its slice
    const int mode = flags & 2;
    const uint8_t* sel_src = static_cast<const uint8_t*>(sel);
    return fsdrv::host_call(n, chunk, cap + (sel_cap + 1) / 2, kWhereAlloc, out, selected, flags, fsdrv::kWordAdd, fsdrv::fits_always,
                            [&](Engine& e, fsdrv::Row& row, int sl, uint64_t pos, uint64_t c) {
                                const uint32_t grid = fsint::grid_for(e);
                                uint64_t first, bytes;
                                where_extent(c, sel_offset + pos, sel_bits, &first, &bytes);
                                uint8_t* d_sel = reinterpret_cast<uint8_t*>(e.stage[sl] + cap);
                                FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], array + pos, c * 2, hipMemcpyHostToDevice, e.stream[sl]));
                                FS_HIP_TRY(hipMemcpyAsync(d_sel, sel_src + first, bytes, hipMemcpyHostToDevice, e.stream[sl]));
                                FS_HIP_TRY(fsk_launch_where(e.stage[sl], c, d_sel, sel_bits == 1 ? (sel_offset + pos) & 7 : 0, sel_bits, row.d, row.d + 32, mode,
                                                            grid, e.stream[sl]));
                                return 0;
                            });
}

}  // extern "C"
