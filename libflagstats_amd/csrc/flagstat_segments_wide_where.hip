// flagstat_segments_wide_where.hip -- selected-elements segmented flagstat of a FLAG array held as 4-byte or 8-byte little-endian
// integers (int32 / int64 columns), read in place: per CSR segment the 32 counters of {element[j] & 0xFFFF : sel(j)}, the number of
// selected elements and the OR of element[j] & ~0xFFFF over the SELECTED elements of THAT segment only, in one launch.  The
// selection is indexed by ARRAY ELEMENT under the two encodings of the `where` entries: an LSB-first bitmap (Arrow's validity
// layout) that may start at any bit, or one byte per element (any non-zero byte selects).  The last corner of the grid {uint16,
// wide} x {whole array, per segment} x {no predicate, -f / -F / -q, mask}: flagstat_segments_wide.hip's geometry, work split, walk
// and window (SegWalk, fsk_segments_policy) and seg_emit<true, true> of flagstat_segments_shared.h, over flagstat_wide_where.hip's
// selection (select_elements of flagstat_wide_where_device.h).
//
// The walk is this kernel's own copy of seg_walk<UE> (flagstat_segments_shared.h), as flagstat_segments_wide_filter.hip keeps one
// and for its reason: under the shared form (with the unit-0 rule below as a template flag of seg_walk) four of the six
// instantiations need 254-256 VGPRs and 4 AGPRs and fall from 2 waves per SIMD to 1; with the walk written out, v[] and the
// selection words local to the regime that uses them, all six fit in 251-256 VGPRs at 2 waves per SIMD without scratch
// (profiles/r19/resource_usage.log).  A change to the walk is made there and here; tests/test_segments_wide_where_host.py holds
// the two together rule by rule.
//
// `high` is the wide_where rule, not the filtered kernels': garbage in a null slot, an unselected element, an element of a
// neighbouring segment or of a gap, and the bytes around the array enter no counter, no count and no mask.  Selecting is zeroing,
// in registers, every dword of an element that is not selected, in front of both the read-out and the mask OR.  No LDS table, no
// scratch.
//
// Geometry.  Units of 8 KiB on the 16-byte grid of the aligned-down base (2048 elements at W = 4, 1024 at W = 8), 8 rows of 64
// lanes x 16 B; every wave of the grid is a writer over a contiguous run of units (tests/segments_wide_oracle.WideWriterSplit).
// A vector holds EPV = 16 / W elements.
//
// Selection, bitmap form.  As in flagstat_wide_where.hip: with bit0 = sel_offset + 8 - lo0 (>= 1) the launcher hands over
// sel = d_sel + (bit0 >> 3) - 1 and shift = bit0 & 7, so that bit q + shift of `sel` belongs to grid position q.  A lane's vectors
// are j = unit * 512 + row * 64 + lane: everything but `lane` is a multiple of 8 / EPV vectors = 8 bits -- every stride of the
// walk (lane -> row -> unit) is a whole number of bitmap bytes -- so with b = lane * EPV + shift
//     byte index   k  = (j - lane) * EPV / 8 + (b >> 3)
//     shift        sh = b & 7                    -- constant for the lane over the whole launch
//     straddle     d  = sh + EPV > 8 ? 1 : 0     -- constant too
// At shift == 0 no lane straddles and a lane loads the one byte sel[k] (FUNNEL false).  Otherwise (FUNNEL) a lane loads two
// adjacent bytes with one unaligned 16-bit load: [k, k + 1] where its bits straddle, [k - 1, k] where they do not.
// No over-read, by construction.  On an unguarded vector every position is an element, so sel[k] holds an element's bit;
// sel[k + 1] is addressed only where the vector's own last bit lies in it; sel[k - 1] holds bits of grid positions between 15 and
// 1 in front of the vector's first.  The uint16 segmented kernel does not have this case (8 bits at sh != 0 always straddle); here,
// at EPV = 4 or 2, a non-straddling lane of grid unit 0 would read a byte in front of the first one that holds an element's bit
// (an aligned array with sel_offset & 7 != 0; every chunk of the host form).  So in a funnelled launch GRID UNIT 0 IS LOADED
// THROUGH THE GUARDED LOADERS ONLY and is never chained (`guard0` of the walk; the segmented counterpart of
// flagstat_wide_where.hip's fast_begin = 1): it is a per-piece unit, loaded guarded whether or not it lies wholly inside the array,
// and a chain run of the segment that covers it begins at unit 1.  From unit 1 on the positions in front of a vector's first are
// at least 8192 / W - 15 > lo0 and below hi0: elements.  tests/segments_wide_where_oracle.py models exactly
// these addresses and tests/test_segments_wide_where_host.py holds them inside the bytes that hold an element's bit.
// Selection, byte form.  SEL_BITS = 8 of the same template: sel is such that the byte of grid position q is sel[q]; the EPV bytes
// of a vector come with one unaligned load of 4 or 2 bytes (load_mapq_wide / load_mapq_wide_guarded: the layout is the MAPQ
// column's) and a byte selects if it is not zero (bytes_mask).  It cannot be routed through flagstat_segments_wide_filter<W, true>
// with min_mapq = 1, as the uint16 byte form is routed through its filtered kernel: that kernel's `high` covers every element
// read, this one's the selected elements only.
//
// Two regimes, chosen per stretch as in flagstat_segments_wide.hip (the same policy: fsk_segments_policy):
//   * chain regime (a run of at least `min_units` whole units inside one segment): wide_step_with under the segmented kernel's
//     per-wave stride (kSegRowVecs), the selection of a vector re-issued right in front of the vector and applied by
//     select_elements as the step's select_vec hook; epochs of 255 units, flushed exactly when the segment ends.  Nothing about
//     the selection is carried from unit to unit except the pointers (there is no table entry and no look-ahead word), so
//     entering a chain run after a per-piece unit or a skipped stretch needs no priming.
//   * per-piece regime: the unit's 8 rows and their selection are loaded once (guarded where the unit is not wholly inside
//     [lo0, hi0), and for unit 0 of a funnelled launch), the selection brought to EPV bits from bit 0.  The selection does not
//     depend on the piece, so the unselected elements of v[] are zeroed once per unit; every piece is then counted with
//     count_piece_wide_with, whose mask_vec_wide keeps neighbours out of counters and mask, and per piece
//     cnt += popcount(selection bits & valid_bits_wide): a selected element outside the piece enters no `selected`.
//
// Emission (seg_emit<true, true>): lanes 0-31 of one instruction write the row (superset slot 9 from the selected count), lane 32
// selected[s], lane 33 high[s]: plain stores where the row is stored plainly, else relaxed agent-scope atomics (add, add, OR)
// issued only for non-zero values.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_engine.h"
#include "flagstat_segments.h"
#include "flagstat_segments_shared.h"
#include "flagstat_segments_wide.h"
#include "flagstat_segments_wide_device.h"
#include "flagstat_segments_wide_where.h"
#include "flagstat_where.h"
#include "flagstat_where_device.h"
#include "flagstat_wide_device.h"
#include "flagstat_wide_filter_device.h"
#include "flagstat_wide_where_device.h"

namespace fsk {

constexpr int kSegWideWhereDepth = 8;   // chain depth as K1: epochs of 255 units

// One unit through wide_step_with, the selection m[u] of vector u applied in front of its read-out.  ROLL 1, 2: vector u's
// selection and registers are re-issued for vector u + 6 of the same unit (`cur`) or u - 2 of the next (`next`, ROLL 1 only).
template <int W, int SEL_BITS, int ROLL, typename LoadSel>
__device__ __forceinline__ void segww_step_and_count(Lane<kSegWideWhereDepth>& s, uint4 (&v)[kUnroll], uint32_t (&m)[kUnroll], uint32_t& blk,
                                                     uint32_t sh, uint32_t& cnt, uint32_t& or_even, uint32_t& or_odd, LoadSel&& load_sel,
                                                     const uint4* __restrict__ cur, const uint4* __restrict__ next,
                                                     const uint8_t* __restrict__ scur, const uint8_t* __restrict__ snext)
{
    constexpr int SS = kSegRowVecs * (16 / W) / (SEL_BITS == 1 ? 8 : 1);   // selection bytes between a lane's consecutive vectors
    blk = __builtin_amdgcn_readfirstlane(blk);
    wide_step_with<W>(
        s, v, blk, or_even, or_odd,
        [&](int u) __attribute__((always_inline)) {
            reissue<ROLL>(u, m, scur, snext, SS, load_sel);
            reissue<ROLL>(u, v, cur, next, kSegRowVecs, load_vec<true>);
        },
        [&](int u) __attribute__((always_inline)) { select_elements<W, SEL_BITS>(v[u], m[u], sh, cnt); });
    end_step<kSegWideWhereDepth>(s, blk);
}

// the EPV selection bits, from bit 0 on, of a vector's selection word as the unguarded loaders deliver it
template <int W, int SEL_BITS>
__device__ __forceinline__ uint32_t selection_bits(uint32_t w, uint32_t sh)
{
    if constexpr (SEL_BITS == 1) {
        return __builtin_amdgcn_ubfe(w, sh, 16 / W);
    } else {
        uint32_t s;
        (void)bytes_mask(w, s);            // 0x01 per selected byte
        return (s * 0x01020408u) >> 24;    // bit 8 e -> bit 24 + e; the 16 partial products fall on 16 different bits
    }
}

// a0: 16-B aligned-down base; the chunk's elements occupy grid positions [lo0, hi0) (elements of W bytes) and are global elements
// [base, base + hi0 - lo0).  sel, shift: the chunk's selection on the same grid (see above; FUNNEL: shift != 0; byte form: shift
// unused).  nunits = ceil(hi0 / (8192 / W)).  mode: bit 0 store form (out[], selected[] and high[] zeroed in front), bit 1
// superset.  selected and high may each be nullptr.
template <int W, int SEL_BITS, bool FUNNEL>
__global__ __launch_bounds__(kThreads) void flagstat_segments_wide_where(const uint4* __restrict__ a0, const uint8_t* __restrict__ sel,
                                                                         uint32_t shift, uint64_t lo0, uint64_t hi0, uint64_t base,
                                                                         const uint64_t* __restrict__ off, uint64_t nseg,
                                                                         uint64_t* __restrict__ out, uint64_t* __restrict__ selected,
                                                                         uint64_t* __restrict__ high, int mode, uint64_t nunits,
                                                                         uint32_t min_units)
{
    static_assert(W == 4 || W == 8, "4-byte or 8-byte elements");
    static_assert(SEL_BITS == 1 || (SEL_BITS == 8 && !FUNNEL), "a bitmap (at a byte boundary of the grid or not) or bytes");
    constexpr uint64_t UE = kSegWideUnitBytes / W;   // elements per unit
    constexpr int EPV = 16 / W;
    constexpr uint64_t RE = 1024 / W;                 // elements per row
    constexpr int SDIV = SEL_BITS == 1 ? 8 : 1;       // elements per selection byte
    constexpr int SS = kSegRowVecs * EPV / SDIV;      // selection bytes of a row
    constexpr int SU = kSegUnitVecs * EPV / SDIV;     // ... of a unit
    static_assert(kSegRowVecs * EPV % 8 == 0, "every stride of the walk is a whole number of bitmap bytes");
    __shared__ uint32_t red_all[kThreads / 64][24];
    const uint32_t lane = threadIdx.x & 63u;
    // bitmap form: where this lane's bits lie in its byte k and whether they reach into byte k + 1 -- for the whole launch.  The
    // funnelled form loads the two bytes [k + d - 1, k + d] at once and finds its bits 8 (1 - d) places further up.
    const uint32_t lane_bit = lane * EPV + (SEL_BITS == 1 ? shift : 0u);
    const uint32_t d = FUNNEL && (lane_bit & 7u) + EPV > 8u ? 1u : 0u;
    const uint32_t sh = SEL_BITS == 1 ? (lane_bit & 7u) + (FUNNEL ? 8u * (1u - d) : 0u) : 0u;
    // this lane's selection byte for vector 0 of grid unit 0, as an offset from `sel` (funnelled: -1 in a lane 0 that does not
    // straddle -- the byte no unguarded load ever takes, see the top)
    const int32_t lane_sel = static_cast<int32_t>(SEL_BITS == 1 ? lane_bit >> 3 : lane_bit) + (FUNNEL ? static_cast<int32_t>(d) - 1 : 0);
    auto load_sel = [](const uint8_t* __restrict__ p) __attribute__((always_inline)) {
        // bitmap: plain loads, not non-temporal ones -- the 8 rows of a unit take 32 or 16 bytes each out of one or two cache
        // lines of the wave's own stretch of the bitmap, and no other wave is near: the line has to stay for the next row
        if constexpr (FUNNEL) {
            return static_cast<uint32_t>(*reinterpret_cast<const u16_any*>(p));
        } else if constexpr (SEL_BITS == 1) {
            return static_cast<uint32_t>(*p);
        } else {
            return load_mapq_wide<W>(p);
        }
    };
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kThreads / 64);
    const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * (kThreads / 64) + wave;
    const uint64_t u_begin = gw * nunits / waves, u_end = (gw + 1) * nunits / waves;
    const uint64_t p0 = u_begin * UE > lo0 ? u_begin * UE : lo0;  // this writer: grid positions [p0, E)
    const uint64_t E = u_end * UE < hi0 ? u_end * UE : hi0;
    if (p0 >= E) return;
    uint32_t* red = red_all[wave];

    SegWalk sw{off, nseg, base, hi0 - lo0, lo0, lane, 0, 0, 0};
    uint64_t s = sw.first_segment(p0);
    if (s >= nseg) return;
    sw.load_window(s);

    Lane<kSegWideWhereDepth> st;
    lane_init(st);
    uint32_t blk = 0;
    uint32_t cnt = 0;                   // selected elements of this lane in segment s not yet emitted
    uint32_t or_even = 0, or_odd = 0;   // dwords of segment s's selected elements not yet emitted
    bool open = false;                  // st, cnt and the mask accumulators hold segment s's, not yet emitted
    uint64_t sb = 0, se = 0;
    auto emit = [&](uint64_t seg, uint64_t b_, uint64_t e_) {
        seg_emit<true, true>(st, blk, cnt, or_even, or_odd, red, out, selected, high, seg, 0, (mode & 1) && b_ >= p0 && e_ <= E, mode, lane);
    };

    uint64_t u = p0 / UE;
    while (s < nseg && u < u_end) {
        sw.bounds(s, sb, se);
        const uint64_t w0 = u * UE;
        const uint64_t x = w0 > p0 ? w0 : p0;
        // (the order of these tests is seg_walk's in flagstat_segments_shared.h, for its reasons)
        if (sb >= E) break;
        if (se <= sb || se <= x) {  // empty (or, with malformed offsets, reversed or behind)
            ++s;
            continue;
        }
        if (sb >= w0 + UE) {  // elements before the segment belong to none: skip whole units unread
            u = sb / UE;
            continue;
        }
        const uint64_t seg_e = se < E ? se : E;
        const bool guard0 = FUNNEL && u == 0;  // the one rule seg_walk does not have: grid unit 0 of a funnelled launch (see the top)
        if (sb <= w0 && w0 >= lo0) {
            const uint64_t k = (seg_e - w0) / UE;  // whole units of segment s from here on
            if (k >= min_units && k > 0) {
                if (!guard0) {
                    const uint4* p = a0 + u * kSegUnitVecs + lane;
                    const uint8_t* ps = sel + u * SU + lane_sel;
                    uint4 v[kUnroll];
                    uint32_t m[kUnroll];
                    // the first kRollDistance vectors, each behind its selection; the rest is issued as they are consumed
#pragma unroll
                    for (int r = 0; r < kRollDistance; ++r) {
                        m[r] = load_sel(ps + r * SS);
                        v[r] = load_vec<true>(p + r * kSegRowVecs);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    for (uint64_t i = 1; i < k; ++i) {
                        const uint4* pn = p + kSegUnitVecs;
                        const uint8_t* psn = ps + SU;
                        segww_step_and_count<W, SEL_BITS, 1>(st, v, m, blk, sh, cnt, or_even, or_odd, load_sel, p, pn, ps, psn);
                        p = pn;
                        ps = psn;
                    }
                    segww_step_and_count<W, SEL_BITS, 2>(st, v, m, blk, sh, cnt, or_even, or_odd, load_sel, p, nullptr, ps, nullptr);
                    u += k;
                    open = true;
                    if (u * UE >= se) {
                        emit(s, sb, se);
                        open = false;
                        ++s;
                    }
                    continue;
                }
            }
        }
        // per-piece unit: its 8 rows and their selection loaded at once, the selection as EPV bits a row from bit 0 on in mp;
        // the selection does not depend on the piece, so the unselected elements are zeroed once per unit
        uint4 v[kUnroll];
        uint32_t mp = 0, unused = 0;
        const uint64_t j0 = u * kSegUnitVecs + lane;
        if (w0 >= lo0 && w0 + UE <= hi0 && !guard0) {
            const uint8_t* ps = sel + u * SU + lane_sel;
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                v[r] = load_vec<true>(a0 + j0 + r * kSegRowVecs);
                const uint32_t bits = selection_bits<W, SEL_BITS>(load_sel(ps + r * SS), sh);
                select_elements<W, 1>(v[r], bits, 0u, unused);
                mp |= bits << (r * EPV);
            }
        } else {
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                v[r] = load_guarded_wide<W>(a0, j0 + r * kSegRowVecs, lo0, hi0);
                uint32_t bits;
                if constexpr (SEL_BITS == 1)
                    bits = load_bits_wide_guarded<W>(sel, shift, j0 + r * kSegRowVecs, lo0, hi0);
                else
                    bits = selection_bits<W, 8>(load_mapq_wide_guarded<W>(sel, j0 + r * kSegRowVecs, lo0, hi0), 0u);
                select_elements<W, 1>(v[r], bits, 0u, unused);
                mp |= bits << (r * EPV);
            }
        }
        const uint64_t w1 = w0 + UE;
        uint64_t xx = x;
        for (;;) {
            // s < nseg, sb < se, se > xx, sb < w1; the piece [b, e) lies inside [p0, E) and so inside [lo0, hi0)
            const uint64_t b = sb > xx ? sb : xx, e = se < w1 ? se : w1;
            uint32_t in_piece = 0;   // bit r * EPV + k: element k of this lane's vector in row r lies in the piece
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                const uint64_t r0 = w0 + static_cast<uint64_t>(r) * RE;
                if (r0 + RE <= b || r0 >= e) continue;   // wave-uniform
                uint32_t vb = (1u << EPV) - 1u;
                if (r0 < b || r0 + RE > e) vb = valid_bits_wide<W>(r0 / EPV + lane, b, e);
                in_piece |= vb << (r * EPV);
            }
            cnt += __builtin_popcount(mp & in_piece);   // a selected element outside the piece enters no `selected`
            count_piece_wide_with<W>(st.acc, or_even, or_odd, v, w0, b, e, lane,
                                     [](int, uint32_t&, uint32_t&, uint32_t&, uint32_t&) __attribute__((always_inline)) {});
            open = true;
            if (e < se) break;  // segment s goes on in the next unit
            emit(s, sb, se);
            open = false;
            ++s;
            xx = e;
            bool more = false;
            while (s < nseg) {
                sw.bounds(s, sb, se);
                if (sb >= E) break;  // (as in the outer walk: before the empty test)
                if (se <= sb || se <= xx) {
                    ++s;
                    continue;
                }
                more = sb < w1;
                break;
            }
            if (!more) break;
        }
        ++u;
    }
    if (open) emit(s, sb, se);  // this writer's range ends inside segment s
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
using fsdrv::where_extent;

// Host-side geometry.  Grid position q is element q - lo0 of the chunk and so bit or byte sel_offset + q - lo0 of d_sel.
// Bytes: that is base[q] with base = d_sel + sel_offset - lo0.  Bitmap: bit q + (bit0 - 8) with bit0 = sel_offset + 8 - lo0 >= 1
// (lo0 < 16 / W), so it is bit q + (bit0 & 7) of base = d_sel + (bit0 >> 3) - 1 (fsk_launch_wide_where's arithmetic with lo0 for
// lo; the chunk's position in the array is folded into sel_offset by the caller).
extern "C" hipError_t fsk_segments_wide_where_geometry(uint64_t address, uint64_t m, int elem_bytes, uint64_t sel_offset, int sel_bits,
                                                       uint32_t grid, uint64_t* geo)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || (sel_bits != 1 && sel_bits != 8) || grid == 0 || geo == nullptr) return hipErrorInvalidValue;
    for (int i = 0; i < 8; ++i) geo[i] = 0;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    if ((address & (W - 1)) || m > (~0ull - 64) / W) return hipErrorInvalidValue;
    if (m == 0) return hipSuccess;
    if (sel_offset > ~0ull - 64 - m) return hipErrorInvalidValue;  // sel_offset + m must be an index
    uint64_t lo0 = 0, nunits = 0;
    uint32_t g = 0;
    fsseg::launch_shape(static_cast<uintptr_t>(address), m, fsk::kSegWideUnitBytes / W, grid, &lo0, &nunits, &g);
    if (!fsseg::wave_totals_fit(nunits, g, fsk::kSegWideUnitBytes / W)) return hipErrorInvalidValue;
    uint64_t first, bytes;
    where_extent(m, sel_offset, sel_bits, &first, &bytes);
    geo[0] = lo0;
    geo[1] = nunits;
    geo[2] = g;
    if (sel_bits == 8) {
        geo[3] = sel_offset - lo0;
    } else {
        const uint64_t bit0 = sel_offset + 8 - lo0;
        geo[3] = (bit0 >> 3) - 1;
        geo[4] = bit0 & 7;
        geo[5] = geo[4] != 0;
    }
    geo[6] = first;
    geo[7] = first + bytes;
    return hipSuccess;
}

extern "C" hipError_t fsk_launch_segments_wide_where(const void* d_chunk, int elem_bytes, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                                     uint64_t base, uint64_t m, const uint64_t* d_offsets, uint64_t nseg, uint64_t* d_out,
                                                     uint64_t* d_selected, uint64_t* d_high, int mode, uint32_t grid, hipStream_t stream)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || (sel_bits != 1 && sel_bits != 8) || (mode & ~3) || grid == 0) return hipErrorInvalidValue;
    if (nseg == 0) return hipSuccess;
    if (d_out == nullptr || d_offsets == nullptr || (m && (d_chunk == nullptr || d_sel == nullptr))) return hipErrorInvalidValue;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_chunk);
    uint64_t geo[8];
    hipError_t e = fsk_segments_wide_where_geometry(addr, m, elem_bytes, sel_offset, sel_bits, grid, geo);
    if (e != hipSuccess) return e;
    if (mode & 1) {
        if (d_selected == d_out + nseg * 32 && d_high == d_selected + nseg) {
            e = fsk_zero_words(d_out, nseg * 34, stream);
        } else {
            e = fsk_zero_words(d_out, nseg * 32, stream);
            if (e == hipSuccess && d_selected) e = fsk_zero_words(d_selected, nseg, stream);
            if (e == hipSuccess && d_high) e = fsk_zero_words(d_high, nseg, stream);
        }
        if (e != hipSuccess) return e;
    }
    if (m == 0) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(addr & ~static_cast<uintptr_t>(15));
    const uint8_t* sel = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_sel) + geo[3]);
    const uint64_t lo0 = geo[0], hi0 = lo0 + m, nunits = geo[1];
    const uint32_t shift = static_cast<uint32_t>(geo[4]);
    uint32_t min_units = 0, blocks_per_cu = 0;
    fsk_segments_policy(&min_units, &blocks_per_cu);
    const dim3 gd(static_cast<uint32_t>(geo[2])), bd(fsk::kThreads);
#define FSK_SWW_LAUNCH(W_, BITS_, FUNNEL_)                                                                                                \
    hipLaunchKernelGGL((fsk::flagstat_segments_wide_where<W_, BITS_, FUNNEL_>), gd, bd, 0, stream, a0, sel, shift, lo0, hi0, base, d_offsets, \
                       nseg, d_out, d_selected, d_high, mode & 3, nunits, min_units)
    if (elem_bytes == 4) {
        if (sel_bits == 8)
            FSK_SWW_LAUNCH(4, 8, false);
        else if (geo[5])
            FSK_SWW_LAUNCH(4, 1, true);
        else
            FSK_SWW_LAUNCH(4, 1, false);
    } else {
        if (sel_bits == 8)
            FSK_SWW_LAUNCH(8, 8, false);
        else if (geo[5])
            FSK_SWW_LAUNCH(8, 1, true);
        else
            FSK_SWW_LAUNCH(8, 1, false);
    }
#undef FSK_SWW_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The bodies of the three forms are fsseg's (flagstat_segments_shared.h): 34 words per segment, the rows, then the selected
// counts, then the masks.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU (nseg > 0 from the NULL checks on): the wide segmented entries' list, then
// the u16 segments_where entries', in their words
int segww_args(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg, const void* sel, uint64_t sel_offset,
               int sel_bits, const void* out, int flags, const char* null_text)
{
    using namespace fsdrv;
    if (check_elem_bytes(elem_bytes, "elem_bytes 2: 16-bit arrays go to the u16 segments_where entries "
                                     "(FLAGSTATS_hip_u16_x64_segments_where, FLAGSTATS_hip_device_u16_segments_where)") ||
        check_sel_bits(sel_bits) || check_flags(flags))
        return -1;
    if (nseg == 0) return 0;
    return refused(fsseg::check_segments(offsets, out, nseg, null_text, fsseg::kMaxSegments / 2) || check_array_given(array, n) ||
                   check_sel_given(sel, n) || check_array_layout(array, n, elem_bytes) || check_sel_range(sel_offset, n));
}

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_wide_segments_where(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* d_offsets, uint64_t nseg,
                                             const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* d_out, uint64_t* d_selected,
                                             uint64_t* d_high, int flags, void* stream)
{
    FS_ENTRY();
    int rc = segww_args(d_array, n, elem_bytes, d_offsets, nseg, d_sel, sel_offset, sel_bits, d_out, flags,
                        fsseg::kNullDevice);
    if (rc || nseg == 0) return rc;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const fsdrv::DeviceWord words[] = {{d_selected, "d_selected", "the counts are added with device atomics"},
                                       {d_high, "d_high", "the masks are ORed with device atomics"}};
    fsdrv::Inputs in = fsseg::offsets_input(d_offsets, nseg);
    in.add_columns(d_array, n, W, d_sel, sel_offset, sel_bits, nullptr, 0);
    return fsseg::device_call(
        d_out, words, 2, in.in, in.count, nseg, stream,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWideUnitBytes / W, grid); },
        [&](uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_wide_where(d_array, elem_bytes, d_sel, sel_offset, sel_bits, 0, n, d_offsets, nseg, d_out,
                                                      d_selected, d_high, flags & 3, grid, s));
            return 0;
        });
}

int FLAGSTATS_hip_device_wide_segments_where_sync(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg,
                                                  const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* out, uint64_t* selected,
                                                  uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = segww_args(d_array, n, elem_bytes, offsets, nseg, d_sel, sel_offset, sel_bits, out, flags, fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    fsdrv::Inputs in;
    in.add_columns(d_array, n, W, d_sel, sel_offset, sel_bits, nullptr, 0);
    return fsseg::sync_call(
        in.in, in.count, n, offsets, nseg, 34, [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWideUnitBytes / W, grid); },
        [&](fsseg::SegBuffers& buf, uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_wide_where(d_array, elem_bytes, d_sel, sel_offset, sel_bits, 0, n, buf.off, nseg, buf.cnt,
                                                      buf.cnt + nseg * 32, buf.cnt + nseg * 33, 1 | (flags & 2), grid, s));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_all(out, selected, high, got, nseg, flags); });
}

int FLAGSTATS_hip_wide_x64_segments_where(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg,
                                          const void* sel, uint64_t sel_offset, int sel_bits, uint64_t* out, uint64_t* selected,
                                          uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = segww_args(array, n, elem_bytes, offsets, nseg, sel, sel_offset, sel_bits, out, flags, fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    // the elements cross the bus as they are, in chunks of "chunk_flags" * 2 bytes (the wide host entries'); a chunk's slice of the
    // selection rides in the same staging buffer, behind its elements -- a bitmap slice from the byte that holds the chunk's first
    // bit (the launch then starts (sel_offset + pos) & 7 bits into it), as FLAGSTATS_hip_wide_x64_where stages it; every chunk's
    // launch adds to the same device rows and counts and ORs into the same device masks
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const int mode = flags & 2;
    const uint8_t* src = static_cast<const uint8_t*>(array);
    const uint8_t* sel_src = static_cast<const uint8_t*>(sel);
    return fsseg::host_call(
        n, offsets, nseg, 34, fsdrv::chunk_flags() * 2 / W, [&] { return offsets[nseg]; },
        [&](uint64_t cap) { return cap * W / 2 + ((sel_bits == 1 ? (cap + 7) / 8 + 1 : cap) + 1) / 2; },
        [&](Engine& e, fsseg::SegBuffers& buf, int sl, uint64_t pos, uint64_t c, uint64_t cap, uint32_t grid) {
            uint64_t sel_first, sel_len;
            where_extent(c, sel_offset + pos, sel_bits, &sel_first, &sel_len);
            uint8_t* d_sel = reinterpret_cast<uint8_t*>(e.stage[sl]) + cap * W;
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], src + pos * W, c * W, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(hipMemcpyAsync(d_sel, sel_src + sel_first, sel_len, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_segments_wide_where(e.stage[sl], elem_bytes, d_sel, sel_bits == 1 ? (sel_offset + pos) & 7 : 0, sel_bits,
                                                      pos, c, buf.off, nseg, buf.cnt, buf.cnt + nseg * 32, buf.cnt + nseg * 33, mode, grid,
                                                      e.stream[sl]));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_all(out, selected, high, got, nseg, flags); });
}

}  // extern "C"
