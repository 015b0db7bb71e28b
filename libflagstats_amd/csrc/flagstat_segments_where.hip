// flagstat_segments_where.hip -- selected-elements segmented flagstat: per CSR segment of a uint16 FLAG array, the 32 counters of
// the flags that a selection picks and how many it picks, in one launch.  The selection is indexed by ARRAY ELEMENT, under the two
// encodings of the `where` entries: an LSB-first bitmap (Arrow's validity layout) that may start at any bit, or one byte per
// element (any non-zero byte selects).
// The segmented kernel (flagstat_segments.hip) with the `where` kernel's bitmap selection (flagstat_where.hip) in front of the
// count.
//
// Byte form: no kernel of its own.  pass4<true> (flagstat_filter_device.h) with require == exclude == 0 and min_mapq == 1 is
// exactly "any non-zero byte selects": the FLAG test passes every flag (x1 == x2 == 0, bit 7 of q stays clear), and of the MAPQ
// test bit 7 of a byte is w7 | t2_7 (k == 0x80808080 turns the majority into an OR) with t2 = (w | 0x80) - 1: byte 0 gives 0x7F
// and has bit 7 clear in both; bytes 1..127 set bit 7 of t2; bytes 128..255 set bit 7 of w.  So the launcher hands the mask,
// from the byte of the chunk's element 0 on, to fsk::flagstat_segments_filter<true> as its MAPQ column
// (fsk_launch_segments_filter), whose loaders touch only bytes of elements.
//
// Work split, walk, window and emission.  The segmented kernels' shared ones (tests/segments_oracle.WriterSplit mirrors them):
// units of 4096 flags on the 16-byte grid of the array's aligned-down base, every wave a writer over a contiguous run of units,
// lane l of a row takes vector row * 64 + l, the 64-ary search for a writer's first segment, the window of 64 offsets, plain
// stores in the store form for rows that lie inside one writer (seg_walk<kSegWaveFlags> and seg_emit<true, false> of
// flagstat_segments_shared.h).
//
// Selection.  Addressed like the `where` kernel's: the launcher hands over a base `sel` such that the 8 bits of grid vector j
// start at bit `sh` of sel[j] (sh == 0: one byte per vector; otherwise two bytes funnelled together: FUNNEL).  A zero flag
// counts in no slot, so selecting is zeroing the flags that are not selected: the 256-entry table in LDS maps 8 selection bits
// to the four v_perm_b32 selectors of the split with 0x0C (-> 0x00) for every flag not selected (flagstat_where_device.h).
//   * chain regime (a run of at least `min_units` whole units in one segment): K1's tree_step / end_step with the `where`
//     kernel's front: split_out_selected under the table entry, the entry of the next vector looked up (and its popcount added
//     to the 22nd lane counter) while this one is counted, the selection byte of a vector issued one vector ahead of it through
//     reissue.  Every position of such a unit is an element of the segment.  The entry carried between steps is primed from the
//     run's first vector every time the walk enters a chain run: after a per-flag unit or a skipped stretch nothing is carried.
//   * per-flag regime: the unit's 8 rows and their 8 selection bytes are loaded at once (through guarded loaders that read only
//     bytes holding a bit of [lo0, hi0) when the unit is the array's ragged first or last) and brought to bit 0.  Per piece and
//     row the selection bits are ANDed with the piece's valid_bits; the result is the table index (one ds_read_b128 and no VALU
//     op, against 10 VALU ops for two nibble_mask and four ANDs) that zeroes the flags in front of count_planes, and its
//     popcount is the selected count.  A selected element of a neighbouring segment, of a gap or of the bytes around the array
//     is cleared there and counts nowhere.
// The table is built by the workgroup's 256 threads and the barrier behind it is passed before any wave returns early.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_engine.h"
#include "flagstat_filter_device.h"
#include "flagstat_segments.h"
#include "flagstat_segments_filter.h"
#include "flagstat_segments_shared.h"
#include "flagstat_segments_where.h"
#include "flagstat_where.h"
#include "flagstat_where_device.h"

namespace fsk {

// K1's step at the default schedule over one unit, the bitmap's selection applied in the split: `entry` is the table entry of
// the vector counted next (on entry: vector 0's; on exit, HAS_NEXT: the next unit's vector 0's).  Vector u's registers are
// re-issued for vector u + 6 of the same unit (`cur`) or u - 2 of the next (`next`), its selection byte one vector further on.
template <bool FUNNEL, bool HAS_NEXT>
__device__ __forceinline__ void segw_step_and_count(Lane<kSegFilterDepth>& s, uint4 (&v)[kUnroll], uint32_t (&m)[kUnroll], uint4& entry,
                                                    const uint4* __restrict__ lut, uint32_t& blk, uint32_t sh, uint32_t& cnt,
                                                    const uint4* cur, const uint4* next, const uint8_t* scur, const uint8_t* snext)
{
    constexpr int ROLL = HAS_NEXT ? 1 : 2;
    blk = __builtin_amdgcn_readfirstlane(blk);
    tree_step<kSegFilterDepth>(s, blk, [&](int uu, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        split_out_selected(v[uu], entry, L0, H0, L1, H1);
        if (uu + 1 < kUnroll || HAS_NEXT) entry = lookup(lut, m[(uu + 1) % kUnroll], sh, cnt);
        reissue<ROLL, 1>(uu, m, scur, snext, kSegRowVecs, load_sel<1, FUNNEL>);
        reissue<ROLL>(uu, v, cur, next, kSegRowVecs, load_vec<true>);
        __builtin_amdgcn_sched_barrier(0);
    });
    end_step<kSegFilterDepth>(s, blk);
}

// the selected flags of the piece [b, e), out of the unit starting at grid position w0 (its 8 rows in v[], their selection bits
// at bit 0 of m[]), into the lane counters and the lane's selected count
__device__ __forceinline__ void count_piece_where(uint32_t (&acc)[kInternal], uint32_t& cnt, const uint4* __restrict__ lut,
                                                  const uint4 (&v)[kUnroll], const uint32_t (&m)[kUnroll], uint64_t w0, uint64_t b,
                                                  uint64_t e, uint32_t lane)
{
#pragma unroll
    for (int r = 0; r < kUnroll; ++r) {
        const uint64_t r0 = w0 + static_cast<uint64_t>(r) * 512u;
        if (r0 + 512u <= b || r0 >= e) continue;  // wave-uniform
        uint32_t vb = 0xFFu;                      // bit k: flag k of this lane's vector lies in the piece
        if (r0 < b || r0 + 512u > e) vb = valid_bits(r0 / 8u + lane, b, e);
        const uint32_t bits = m[r] & vb;          // ... and is selected
        cnt += __builtin_popcount(bits);
        const uint4 entry = lut[bits];
        uint32_t L0, H0, L1, H1;
        split_out_selected(v[r], entry, L0, H0, L1, H1);
        count_planes(acc, L0, H0, L1, H1);
    }
}

// a0: 16-B aligned-down base; the chunk's flags occupy grid positions [lo0, hi0) and are global flags [base, base + hi0 - lo0).
// sel, shift: the chunk's selection on the same grid (the 8 bits of grid vector j start at bit `shift` of sel[j]; FUNNEL:
// shift != 0).  nunits = ceil(hi0 / 4096).  mode: bit 0 store form (out[] and selected[] zeroed in front), bit 1 superset.
// selected may be nullptr.
template <bool FUNNEL>
__global__ __launch_bounds__(kThreads) void flagstat_segments_where(const uint4* __restrict__ a0, const uint8_t* __restrict__ sel,
                                                                    uint32_t shift, uint64_t lo0, uint64_t hi0, uint64_t base,
                                                                    const uint64_t* __restrict__ off, uint64_t nseg,
                                                                    uint64_t* __restrict__ out, uint64_t* __restrict__ selected, int mode,
                                                                    uint64_t nunits, uint32_t min_units)
{
    static_assert(kThreads == 256, "one thread per table entry");
    __shared__ uint4 lut[256];
    __shared__ uint32_t red_all[kThreads / 64][24];
    lut[threadIdx.x] = selector_entry(threadIdx.x);
    __syncthreads();  // the only workgroup barrier: behind it waves return and walk on their own
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* red = red_all[threadIdx.x >> 6];
    const uint32_t sh = FUNNEL ? __builtin_amdgcn_readfirstlane(shift) : 0u;
    Lane<kSegFilterDepth> st;
    lane_init(st);
    uint32_t blk = 0;
    uint32_t cnt = 0;   // selected flags of this lane in the open segment
    uint32_t none = 0;  // no mask
    uint4 v[kUnroll];
    uint32_t m[kUnroll];
    seg_walk<kSegWaveFlags>(
        lo0, hi0, base, off, nseg, mode, nunits, min_units,
        [&](uint64_t u, uint64_t k) __attribute__((always_inline)) {
            const uint4* p = a0 + u * kSegUnitVecs + lane;
            const uint8_t* ps = sel + u * kSegUnitVecs + lane;
            // the first kRollDistance vectors, the selection bytes one vector ahead of them
            m[0] = load_sel<1, FUNNEL>(ps);
#pragma unroll
            for (int r = 0; r < kRollDistance; ++r) {
                m[r + 1] = load_sel<1, FUNNEL>(ps + (r + 1) * kSegRowVecs);
                v[r] = load_vec<true>(p + r * kSegRowVecs);
                __builtin_amdgcn_sched_barrier(0);
            }
            // entering a chain run: whatever came before (a per-flag unit, a skipped stretch, another run) left no entry
            uint4 entry = lookup(lut, m[0], sh, cnt);
            for (uint64_t i = 1; i < k; ++i) {
                const uint4* pn = p + kSegUnitVecs;
                const uint8_t* psn = ps + kSegUnitVecs;
                segw_step_and_count<FUNNEL, true>(st, v, m, entry, lut, blk, sh, cnt, p, pn, ps, psn);
                p = pn;
                ps = psn;
            }
            segw_step_and_count<FUNNEL, false>(st, v, m, entry, lut, blk, sh, cnt, p, nullptr, ps, nullptr);
        },
        [&](uint64_t u, bool whole) __attribute__((always_inline)) {
            const uint64_t j0 = u * kSegUnitVecs + lane;
            if (whole) {
#pragma unroll
                for (int r = 0; r < kUnroll; ++r) {
                    v[r] = load_vec<true>(a0 + j0 + r * kSegRowVecs);
                    m[r] = __builtin_amdgcn_ubfe(load_sel<1, FUNNEL>(sel + j0 + r * kSegRowVecs), sh, 8);
                }
            } else {
#pragma unroll
                for (int r = 0; r < kUnroll; ++r) {
                    v[r] = load_guarded(a0, j0 + r * kSegRowVecs, lo0, hi0);
                    m[r] = load_sel_guarded<1>(sel, sh, j0 + r * kSegRowVecs, lo0, hi0);
                }
            }
        },
        [&](uint64_t w0, uint64_t b, uint64_t e) __attribute__((always_inline)) {
            count_piece_where(st.acc, cnt, lut, v, m, w0, b, e, lane);
        },
        [&](uint64_t s, uint64_t len, bool plain) __attribute__((always_inline)) {
            seg_emit<true, false>(st, blk, cnt, none, none, red, out, selected, nullptr, s, len, plain, mode, lane);
        });
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
using fsdrv::where_extent;

// Host-side geometry.  Grid position q is element q - lo0 of the chunk and so bit or byte sel_offset + q - lo0 of d_sel.
// Bytes: that is base[q] with base = d_sel + sel_offset - lo0.  Bitmap: bit q + (bit0 - 8) with bit0 = sel_offset + 8 - lo0 >= 1,
// so the 8 bits of grid vector j start at bit bit0 & 7 of byte j of base = d_sel + (bit0 >> 3) - 1 (fsk_launch_where's
// arithmetic with lo0 for lo; the chunk's position in the array is folded into sel_offset by the caller).
extern "C" hipError_t fsk_segments_where_geometry(uint64_t address, uint64_t m, uint64_t sel_offset, int sel_bits, uint32_t grid,
                                                  uint64_t* geo)
{
    if ((sel_bits != 1 && sel_bits != 8) || grid == 0 || geo == nullptr) return hipErrorInvalidValue;
    for (int i = 0; i < 7; ++i) geo[i] = 0;
    if ((address & 1u) || m > (~0ull - 64) / 2) return hipErrorInvalidValue;
    if (m == 0) return hipSuccess;
    if (sel_offset > ~0ull - 64 - m) return hipErrorInvalidValue;  // sel_offset + m must be an index
    uint64_t lo0 = 0, nunits = 0;
    uint32_t g = 0;
    fsseg::launch_shape(static_cast<uintptr_t>(address), m, fsk::kSegWaveFlags, grid, &lo0, &nunits, &g);
    if (!fsseg::wave_totals_fit(nunits, g, fsk::kSegWaveFlags)) return hipErrorInvalidValue;
    uint64_t first, bytes;
    where_extent(m, sel_offset, sel_bits, &first, &bytes);
    geo[0] = lo0;
    geo[1] = nunits;
    geo[2] = g;
    if (sel_bits == 8) {
        geo[3] = sel_offset - lo0;
        geo[4] = 0;
    } else {
        const uint64_t bit0 = sel_offset + 8 - lo0;
        geo[3] = (bit0 >> 3) - 1;
        geo[4] = bit0 & 7;
    }
    geo[5] = first;
    geo[6] = first + bytes;
    return hipSuccess;
}

extern "C" hipError_t fsk_launch_segments_where(const uint16_t* d_chunk, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                                uint64_t base, uint64_t m, const uint64_t* d_offsets, uint64_t nseg, uint64_t* d_out,
                                                uint64_t* d_selected, int mode, uint32_t grid, hipStream_t stream)
{
    if ((sel_bits != 1 && sel_bits != 8) || (mode & ~3) || grid == 0) return hipErrorInvalidValue;
    if (nseg == 0) return hipSuccess;
    if (d_out == nullptr || d_offsets == nullptr || (m && (d_chunk == nullptr || d_sel == nullptr))) return hipErrorInvalidValue;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_chunk);
    uint64_t geo[7];
    hipError_t e = fsk_segments_where_geometry(addr, m, sel_offset, sel_bits, grid, geo);
    if (e != hipSuccess) return e;
    if (sel_bits == 8)  // the mask is the filtered kernel's MAPQ column (see the top), which that launcher takes from element 0 on
        return fsk_launch_segments_filter(d_chunk, static_cast<const uint8_t*>(d_sel) + sel_offset, base, m, d_offsets, nseg, 0u, 0u, 1u,
                                          d_out, d_selected, mode, grid, stream);
    const uint8_t* sel = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_sel) + geo[3]);
    if (mode & 1) {
        e = fsk_zero_words(d_out, nseg * 32, stream);
        if (e == hipSuccess && d_selected) e = fsk_zero_words(d_selected, nseg, stream);
        if (e != hipSuccess) return e;
    }
    if (m == 0) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(addr & ~static_cast<uintptr_t>(15));
    const uint64_t lo0 = geo[0], hi0 = lo0 + m, nunits = geo[1];
    const uint32_t shift = static_cast<uint32_t>(geo[4]);
    uint32_t min_units = 0, blocks_per_cu = 0;
    fsk_segments_policy(&min_units, &blocks_per_cu);
    const dim3 gd(static_cast<uint32_t>(geo[2])), bd(fsk::kThreads);
    if (shift == 0)
        hipLaunchKernelGGL((fsk::flagstat_segments_where<false>), gd, bd, 0, stream, a0, sel, 0u, lo0, hi0, base, d_offsets, nseg, d_out,
                           d_selected, mode & 3, nunits, min_units);
    else
        hipLaunchKernelGGL((fsk::flagstat_segments_where<true>), gd, bd, 0, stream, a0, sel, shift, lo0, hi0, base, d_offsets, nseg, d_out,
                           d_selected, mode & 3, nunits, min_units);
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The bodies of the three forms are fsseg's (flagstat_segments_shared.h): 33 words per segment, the rows, then the selected counts.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU (nseg > 0 from the NULL checks on): segf_args' and where_args' refusals
int segw_args(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg, const void* sel, uint64_t sel_offset, int sel_bits,
              const void* out, int flags, const char* null_text)
{
    using namespace fsdrv;
    if (check_sel_bits(sel_bits) || check_flags(flags)) return -1;
    if (nseg == 0) return 0;
    return refused(fsseg::check_segments(offsets, out, nseg, null_text, fsseg::kMaxSegments / 2) || check_array_given(array, n) ||
                   check_sel_given(sel, n) || check_array_layout(array, n, 2) || check_sel_range(sel_offset, n));
}

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_u16_segments_where(const uint16_t* d_array, uint64_t n, const uint64_t* d_offsets, uint64_t nseg,
                                            const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* d_out, uint64_t* d_selected,
                                            int flags, void* stream)
{
    FS_ENTRY();
    int rc = segw_args(d_array, n, d_offsets, nseg, d_sel, sel_offset, sel_bits, d_out, flags, fsseg::kNullDevice);
    if (rc || nseg == 0) return rc;
    const fsdrv::DeviceWord word{d_selected, "d_selected", "the counts are added with device atomics"};
    fsdrv::Inputs in = fsseg::offsets_input(d_offsets, nseg);
    in.add_columns(d_array, n, 2, d_sel, sel_offset, sel_bits, nullptr, 0);
    return fsseg::device_call(
        d_out, &word, 1, in.in, in.count, nseg, stream, [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWaveFlags, grid); },
        [&](uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_where(d_array, d_sel, sel_offset, sel_bits, 0, n, d_offsets, nseg, d_out, d_selected, flags & 3,
                                                 grid, s));
            return 0;
        });
}

int FLAGSTATS_hip_device_u16_segments_where_sync(const uint16_t* d_array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                                 const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* out, uint64_t* selected,
                                                 int flags)
{
    FS_ENTRY();
    int rc = segw_args(d_array, n, offsets, nseg, d_sel, sel_offset, sel_bits, out, flags, fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, d_sel, sel_offset, sel_bits, nullptr, 0);
    return fsseg::sync_call(
        in.in, in.count, n, offsets, nseg, 33, [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWaveFlags, grid); },
        [&](fsseg::SegBuffers& buf, uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_where(d_array, d_sel, sel_offset, sel_bits, 0, n, buf.off, nseg, buf.cnt, buf.cnt + nseg * 32,
                                                 1 | (flags & 2), grid, s));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_both(out, selected, got, nseg, flags); });
}

int FLAGSTATS_hip_u16_x64_segments_where(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg, const void* sel,
                                         uint64_t sel_offset, int sel_bits, uint64_t* out, uint64_t* selected, int flags)
{
    FS_ENTRY();
    int rc = segw_args(array, n, offsets, nseg, sel, sel_offset, sel_bits, out, flags, fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    // a chunk's slice of the selection rides in the same staging buffer, behind the flags -- a bitmap slice from the byte that
    // holds the chunk's first bit (the launch then starts (sel_offset + pos) & 7 bits into it)
    const int mode = flags & 2;
    const uint8_t* sel_src = static_cast<const uint8_t*>(sel);
    return fsseg::host_call(
        n, offsets, nseg, 33, fsdrv::chunk_flags(), [&] { return offsets[nseg]; },
        [&](uint64_t cap) { return cap + ((sel_bits == 1 ? (cap + 7) / 8 + 1 : cap) + 1) / 2; },
        [&](Engine& e, fsseg::SegBuffers& buf, int sl, uint64_t pos, uint64_t c, uint64_t cap, uint32_t grid) {
            uint64_t sel_first, sel_len;
            where_extent(c, sel_offset + pos, sel_bits, &sel_first, &sel_len);
            uint8_t* d_sel = reinterpret_cast<uint8_t*>(e.stage[sl] + cap);
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], array + pos, c * sizeof(uint16_t), hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(hipMemcpyAsync(d_sel, sel_src + sel_first, sel_len, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_segments_where(e.stage[sl], d_sel, sel_bits == 1 ? (sel_offset + pos) & 7 : 0, sel_bits, pos, c, buf.off,
                                                 nseg, buf.cnt, buf.cnt + nseg * 32, mode, grid, e.stream[sl]));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_both(out, selected, got, nseg, flags); });
}

}  // extern "C"
