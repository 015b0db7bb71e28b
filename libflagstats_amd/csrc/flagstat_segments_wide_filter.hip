// flagstat_segments_wide_filter.hip -- filtered segmented flagstat of a FLAG array held as 4-byte or 8-byte little-endian integers
// (int32 / int64 columns), read in place: per CSR segment the 32 counters of the elements whose low 16 bits pass samtools' view
// filter, how many pass, and the OR of every bit above bit 15 that one of the segment's elements carries -- passing or not --, in
// one launch.  With f(j) = element[j] & 0xFFFF,
//   pass(j) = (f(j) & require) == require && (f(j) & exclude) == 0 && (min_mapq == 0 || mapq[j] >= min_mapq).
// It is flagstat_segments_wide.hip with the filter in front of the count; the last corner of the grid {uint16, wide} x {whole
// array, per segment} x {no predicate, -f / -F / -q}.
//
// Geometry, work split and walk.  flagstat_segments_wide.hip's -- but this kernel keeps its own copy of the walk that the other
// four take from flagstat_segments_shared.h (seg_walk<UE>): under the shared form the two MAPQ instantiations need 262 and 260
// VGPRs against 255 and 253 and fall from 2 waves per SIMD to 1 (profiles/r18/).  A change to the walk is made there and here;
// tests/test_segments_wide_filter_host.py holds the two together rule by rule.  The 16-byte grid of the aligned-down base, positions
// are elements of W bytes, units of 8 KiB (2048 elements at W = 4, 1024 at W = 8), every wave of the grid a writer over a
// contiguous run of units, SegWalk / seg_slot_value (flagstat_segments_shared.h), the policy of fsk_segments_policy.
// tests/segments_wide_oracle.WideWriterSplit mirrors the split of both kernels.
//
// Predicate.  A zero flag counts in no slot, so filtering is zeroing the flags that fail on their byte planes in front of front4 /
// count_planes (pass4 and the v_perm_b32 mask of flagstat_filter_device.h).  The MAPQ column is addressed like
// flagstat_wide_filter.hip's: `mq` is such that the byte of grid position q is mq[q], at any alignment; one unaligned dword per
// vector at W = 4, one unaligned 16-bit load per vector at W = 8.  The kernel is a template on whether the column is read at all.
//   * chain regime (a run of at least `min_units` whole units inside one segment): the filtered wide step (wide_filter_step_with
//     of flagstat_wide_filter_device.h) under the segmented kernel's per-wave stride, a vector's MAPQ bytes re-issued with it;
//     epochs of 255 units, flushed exactly when the segment ends.  Every position of such a unit is an element of the segment, so
//     no position needs masking.
//   * per-piece regime: the unit's 8 rows and their MAPQ bytes are loaded once (through the guarded loaders where the unit is not
//     wholly inside the array) and counted per piece with count_piece_wide_with (flagstat_segments_wide_device.h).  Two maskings,
//     which are not the same thing: the dwords of elements outside the piece are zeroed (mask_vec_wide), which keeps them out of
//     `high` and out of the counters; and the pass bits of positions outside the piece are cleared (valid_bits_wide spread with
//     nibble_to_bit7), because a zeroed element passes every predicate without `require` bits and would enter `selected`.
//     At W = 8 a count_planes call takes four rows of the unit: the MAPQ dword of its first plane pair is the 16-bit halves of
//     rows 4 g and 4 g + 1 (low, high), that of the second those of rows 4 g + 2 and 4 g + 3; the valid bits pair up the same way.
//
// Emission (seg_emit<true, true> of flagstat_segments_shared.h): the lane's 21 counters, its passing count and its two mask accumulators are reduced and
// reset at a segment's end; lanes 0-31 of one instruction write the row (superset slot 9 from the passing count), lane 32
// selected[s], lane 33 high[s]: plain stores where the row is stored plainly, else relaxed agent-scope atomics (add, add, OR),
// issued only for non-zero values.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_engine.h"
#include "flagstat_filter_device.h"
#include "flagstat_segments.h"
#include "flagstat_segments_shared.h"
#include "flagstat_segments_wide.h"
#include "flagstat_segments_wide_device.h"
#include "flagstat_segments_wide_filter.h"
#include "flagstat_wide_device.h"
#include "flagstat_wide_filter_device.h"

namespace fsk {

constexpr int kSegWideFilterDepth = 8;   // chain depth as K1: epochs of 255 units

// the filtered wide step over one unit: vector u's MAPQ bytes and registers are re-issued for vector u + 6 of the same unit
// (`cur`) or u - 2 of the next (`next`, if HAS_NEXT)
template <int W, bool MAPQ, bool HAS_NEXT>
__device__ __forceinline__ void segwf_step_and_count(Lane<kSegWideFilterDepth>& s, const FilterArgs& f, uint4 (&v)[kUnroll],
                                                     uint32_t (&m)[kUnroll], uint32_t& blk, uint32_t& cnt, uint32_t& or_even,
                                                     uint32_t& or_odd, const uint4* cur, const uint4* next, const uint8_t* mcur,
                                                     const uint8_t* mnext)
{
    const uint32_t vb[kUnroll] = {};   // not looked at: every position of a chain unit is an element of the segment
    blk = __builtin_amdgcn_readfirstlane(blk);
    wide_filter_step_with<W, MAPQ, HAS_NEXT ? 1 : 2, kSegRowVecs>(s, f, v, m, vb, blk, cnt, or_even, or_odd, cur, next, mcur, mnext);
    end_step<kSegWideFilterDepth>(s, blk);
}

// the elements of the piece [b, e) that pass, out of the unit starting at grid position w0 (its 8 rows in v[], their MAPQ bytes
// in m[]), into the lane counters and the lane's passing count; the dwords of every element of the piece into the lane's mask
// accumulators
template <int W, bool MAPQ>
__device__ __forceinline__ void count_piece_wide_filter(uint32_t (&acc)[kInternal], uint32_t& cnt, uint32_t& or_even, uint32_t& or_odd,
                                                        const FilterArgs& f, const uint4 (&v)[kUnroll], const uint32_t (&m)[kUnroll],
                                                        uint64_t w0, uint64_t b, uint64_t e, uint32_t lane)
{
    constexpr uint64_t RE = 1024 / W;   // elements per row
    constexpr uint32_t EPV = 16 / W;
    // bit k: element k of this lane's vector in row r of the unit lies in the piece
    auto row_bits = [&](int r) __attribute__((always_inline)) -> uint32_t {
        const uint64_t r0 = w0 + static_cast<uint64_t>(r) * RE;
        if (r0 + RE <= b || r0 >= e) return 0u;  // wave-uniform
        if (r0 >= b && r0 + RE <= e) return (1u << EPV) - 1u;
        return valid_bits_wide<W>(r0 / EPV + lane, b, e);
    };
    count_piece_wide_with<W>(acc, or_even, or_odd, v, w0, b, e, lane,
                             [&](int g, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1) __attribute__((always_inline)) {
        uint32_t n0, n1, q0, q1;   // valid bits and MAPQ bytes of the 4 elements of (L0, H0) and of (L1, H1)
        if constexpr (W == 4) {
            n0 = row_bits(2 * g);
            n1 = row_bits(2 * g + 1);
            q0 = m[2 * g];
            q1 = m[2 * g + 1];
        } else {
            n0 = row_bits(4 * g) | (row_bits(4 * g + 1) << 2);
            n1 = row_bits(4 * g + 2) | (row_bits(4 * g + 3) << 2);
            q0 = m[4 * g] | (m[4 * g + 1] << 16);
            q1 = m[4 * g + 2] | (m[4 * g + 3] << 16);
        }
        const uint32_t p0 = pass4<MAPQ>(f, L0, H0, q0) & nibble_to_bit7(n0);
        const uint32_t p1 = pass4<MAPQ>(f, L1, H1, q1) & nibble_to_bit7(n1);
        cnt += __builtin_popcount(p0);
        cnt += __builtin_popcount(p1);
        const uint32_t M0 = perm(0u, 0u, p0), M1 = perm(0u, 0u, p1);   // selector 0x80 -> 0xFF, 0x00 -> source byte 0 = 0x00
        L0 &= M0;
        H0 &= M0;
        L1 &= M1;
        H1 &= M1;
    });
}

// a0: 16-B aligned-down base; the chunk's elements occupy grid positions [lo0, hi0) (elements of W bytes) and are global elements
// [base, base + hi0 - lo0).  mq: the chunk's MAPQ column on the same grid (the byte of position q is mq[q]; not read when !MAPQ).
// require & exclude == 0 (the launcher's business), both below 2^16, min_mapq in 1..255 when MAPQ.  nunits = ceil(hi0 / (8192 /
// W)).  mode: bit 0 store form (out[], selected[] and high[] zeroed in front), bit 1 superset.  selected and high may each be
// nullptr.
template <int W, bool MAPQ>
__global__ __launch_bounds__(kThreads) void flagstat_segments_wide_filter(const uint4* __restrict__ a0, const uint8_t* __restrict__ mq,
                                                                          uint32_t require, uint32_t exclude, uint32_t min_mapq,
                                                                          uint64_t lo0, uint64_t hi0, uint64_t base,
                                                                          const uint64_t* __restrict__ off, uint64_t nseg,
                                                                          uint64_t* __restrict__ out, uint64_t* __restrict__ selected,
                                                                          uint64_t* __restrict__ high, int mode, uint64_t nunits,
                                                                          uint32_t min_units)
{
    static_assert(W == 4 || W == 8, "4-byte or 8-byte elements");
    constexpr uint64_t UE = kSegWideUnitBytes / W;   // elements per unit
    constexpr int EPV = 16 / W;                       // elements, and MAPQ bytes, per vector
    constexpr int kRowMapq = kSegRowVecs * EPV;       // MAPQ bytes of a row
    __shared__ uint32_t red_all[kThreads / 64][24];
    const uint32_t lane = threadIdx.x & 63u;
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

    const FilterArgs f = filter_args_of(require, exclude, min_mapq);
    Lane<kSegWideFilterDepth> st;
    lane_init(st);
    uint32_t blk = 0;
    uint32_t cnt = 0;                   // passing elements of this lane in segment s not yet emitted
    uint32_t or_even = 0, or_odd = 0;   // dwords of segment s's elements, passing or not, not yet emitted
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
        if (sb <= w0 && w0 >= lo0) {
            const uint64_t k = (seg_e - w0) / UE;  // whole units of segment s from here on
            if (k >= min_units && k > 0) {
                const uint4* p = a0 + u * kSegUnitVecs + lane;
                const uint8_t* pm = mq + (u * kSegUnitVecs + lane) * EPV;
                uint4 v[kUnroll];
                uint32_t m[kUnroll];
#pragma unroll
                for (int r = 0; r < kRollDistance; ++r) {
                    if constexpr (MAPQ) m[r] = load_mapq_wide<W>(pm + r * kRowMapq);
                    v[r] = load_vec<true>(p + r * kSegRowVecs);
                    __builtin_amdgcn_sched_barrier(0);
                }
                for (uint64_t i = 1; i < k; ++i) {
                    const uint4* pn = p + kSegUnitVecs;
                    const uint8_t* pmn = pm + UE;
                    segwf_step_and_count<W, MAPQ, true>(st, f, v, m, blk, cnt, or_even, or_odd, p, pn, pm, pmn);
                    p = pn;
                    pm = pmn;
                }
                segwf_step_and_count<W, MAPQ, false>(st, f, v, m, blk, cnt, or_even, or_odd, p, nullptr, pm, nullptr);
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
        // per-piece unit: its 8 rows and their MAPQ bytes loaded at once, then every segment piece in it
        uint4 v[kUnroll];
        uint32_t m[kUnroll];
        const uint64_t j0 = u * kSegUnitVecs + lane;
        if (w0 >= lo0 && w0 + UE <= hi0) {
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                v[r] = load_vec<true>(a0 + j0 + r * kSegRowVecs);
                if constexpr (MAPQ)
                    m[r] = load_mapq_wide<W>(mq + (j0 + r * kSegRowVecs) * EPV);
                else
                    m[r] = 0;
            }
        } else {
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                v[r] = load_guarded_wide<W>(a0, j0 + r * kSegRowVecs, lo0, hi0);
                if constexpr (MAPQ)
                    m[r] = load_mapq_wide_guarded<W>(mq, j0 + r * kSegRowVecs, lo0, hi0);
                else
                    m[r] = 0;
            }
        }
        const uint64_t w1 = w0 + UE;
        uint64_t xx = x;
        for (;;) {
            // s < nseg, sb < se, se > xx, sb < w1; the piece [b, e) lies inside [p0, E) and so inside [lo0, hi0)
            const uint64_t b = sb > xx ? sb : xx, e = se < w1 ? se : w1;
            count_piece_wide_filter<W, MAPQ>(st.acc, cnt, or_even, or_odd, f, v, m, w0, b, e, lane);
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
extern "C" hipError_t fsk_launch_segments_wide_filter(const void* d_chunk, int elem_bytes, const uint8_t* d_mapq_chunk, uint64_t base,
                                                      uint64_t m, const uint64_t* d_offsets, uint64_t nseg, uint32_t require,
                                                      uint32_t exclude, uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected,
                                                      uint64_t* d_high, int mode, uint32_t grid, hipStream_t stream)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || (mode & ~3) || grid == 0 || require > 0xFFFFu || exclude > 0xFFFFu || min_mapq > 255u)
        return hipErrorInvalidValue;
    if (nseg == 0) return hipSuccess;
    if (d_out == nullptr || d_offsets == nullptr || (m && (d_chunk == nullptr || (min_mapq && d_mapq_chunk == nullptr))))
        return hipErrorInvalidValue;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_chunk);
    if ((addr & (W - 1)) || m > (~0ull - 64) / W) return hipErrorInvalidValue;
    uint64_t lo0 = 0, nunits = 0;
    uint32_t g = 0;
    if (m) {
        fsseg::launch_shape(addr, m, fsk::kSegWideUnitBytes / W, grid, &lo0, &nunits, &g);
        if (!fsseg::wave_totals_fit(nunits, g, fsk::kSegWideUnitBytes / W)) return hipErrorInvalidValue;
    }
    if (mode & 1) {
        hipError_t e;
        if (d_selected == d_out + nseg * 32 && d_high == d_selected + nseg) {
            e = fsk_zero_words(d_out, nseg * 34, stream);
        } else {
            e = fsk_zero_words(d_out, nseg * 32, stream);
            if (e == hipSuccess && d_selected) e = fsk_zero_words(d_selected, nseg, stream);
            if (e == hipSuccess && d_high) e = fsk_zero_words(d_high, nseg, stream);
        }
        if (e != hipSuccess) return e;
    }
    // a bit both required and excluded: no element passes (samtools accepts the pair); the kernel's test assumes a disjoint pair.
    // Nothing is launched, so no element is read and the masks stay what the store form's zeroing or the caller left there.
    if (m == 0 || (require & exclude)) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(addr & ~static_cast<uintptr_t>(15));
    const uint64_t hi0 = lo0 + m;
    uint32_t min_units = 0, blocks_per_cu = 0;
    fsk_segments_policy(&min_units, &blocks_per_cu);
    // grid position q is element q - lo0 of the chunk: its byte is d_mapq_chunk[q - lo0]
    const uint8_t* mq = min_mapq ? reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_mapq_chunk) - lo0) : nullptr;
    const dim3 gd(g), bd(fsk::kThreads);
#define FSK_SWF_LAUNCH(W_, Q_)                                                                                                       \
    hipLaunchKernelGGL((fsk::flagstat_segments_wide_filter<W_, Q_>), gd, bd, 0, stream, a0, mq, require, exclude, min_mapq, lo0, hi0, \
                       base, d_offsets, nseg, d_out, d_selected, d_high, mode & 3, nunits, min_units)
    if (elem_bytes == 4) {
        if (min_mapq)
            FSK_SWF_LAUNCH(4, true);
        else
            FSK_SWF_LAUNCH(4, false);
    } else {
        if (min_mapq)
            FSK_SWF_LAUNCH(8, true);
        else
            FSK_SWF_LAUNCH(8, false);
    }
#undef FSK_SWF_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The bodies of the three forms are fsseg's (flagstat_segments_shared.h): 34 words per segment, the rows, then the selected
// counts, then the masks.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU (nseg > 0 from the NULL checks on): the wide segmented entries' list, then
// the filtered segmented entries', in their words
int segwf_args(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg, uint32_t require, uint32_t exclude,
               const uint8_t* mapq, uint32_t min_mapq, const void* out, int flags, const char* null_text)
{
    using namespace fsdrv;
    if (check_elem_bytes(elem_bytes, "elem_bytes 2: 16-bit arrays go to the u16 segmented filter entries "
                                     "(FLAGSTATS_hip_u16_x64_segments_filter, FLAGSTATS_hip_device_u16_segments_filter)") ||
        check_predicate(require, exclude, min_mapq) || check_flags(flags))
        return -1;
    if (nseg == 0) return 0;
    return refused(fsseg::check_segments(offsets, out, nseg, null_text, fsseg::kMaxSegments / 2) || check_array_given(array, n) ||
                   check_mapq_given(mapq, n, min_mapq) || check_array_layout(array, n, elem_bytes));
}

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_wide_segments_filter(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* d_offsets, uint64_t nseg,
                                              uint32_t require, uint32_t exclude, const uint8_t* d_mapq, uint32_t min_mapq,
                                              uint64_t* d_out, uint64_t* d_selected, uint64_t* d_high, int flags, void* stream)
{
    FS_ENTRY();
    int rc = segwf_args(d_array, n, elem_bytes, d_offsets, nseg, require, exclude, d_mapq, min_mapq, d_out, flags,
                        fsseg::kNullDevice);
    if (rc || nseg == 0) return rc;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const fsdrv::DeviceWord words[] = {{d_selected, "d_selected", "the counts are added with device atomics"},
                                       {d_high, "d_high", "the masks are ORed with device atomics"}};
    fsdrv::Inputs in = fsseg::offsets_input(d_offsets, nseg);
    in.add_columns(d_array, n, W, nullptr, 0, 0, d_mapq, min_mapq);
    return fsseg::device_call(
        d_out, words, 2, in.in, in.count, nseg, stream,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWideUnitBytes / W, grid); },
        [&](uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_wide_filter(d_array, elem_bytes, d_mapq, 0, n, d_offsets, nseg, require, exclude, min_mapq, d_out,
                                                       d_selected, d_high, flags & 3, grid, s));
            return 0;
        });
}

int FLAGSTATS_hip_device_wide_segments_filter_sync(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg,
                                                   uint32_t require, uint32_t exclude, const uint8_t* d_mapq, uint32_t min_mapq,
                                                   uint64_t* out, uint64_t* selected, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = segwf_args(d_array, n, elem_bytes, offsets, nseg, require, exclude, d_mapq, min_mapq, out, flags,
                        fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    fsdrv::Inputs in;
    in.add_columns(d_array, n, W, nullptr, 0, 0, d_mapq, min_mapq);
    return fsseg::sync_call(
        in.in, in.count, n, offsets, nseg, 34,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWideUnitBytes / W, grid); },
        [&](fsseg::SegBuffers& buf, uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_wide_filter(d_array, elem_bytes, d_mapq, 0, n, buf.off, nseg, require, exclude, min_mapq, buf.cnt,
                                                       buf.cnt + nseg * 32, buf.cnt + nseg * 33, 1 | (flags & 2), grid, s));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_all(out, selected, high, got, nseg, flags); });
}

int FLAGSTATS_hip_wide_x64_segments_filter(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg,
                                           uint32_t require, uint32_t exclude, const uint8_t* mapq, uint32_t min_mapq, uint64_t* out,
                                           uint64_t* selected, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = segwf_args(array, n, elem_bytes, offsets, nseg, require, exclude, mapq, min_mapq, out, flags,
                        fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    // the elements cross the bus as they are, in chunks of "chunk_flags" * 2 bytes (the wide host entries'); a chunk's slice of the
    // MAPQ column rides in the same staging buffer, behind its elements (as FLAGSTATS_hip_wide_x64_filter stages it); every
    // chunk's launch adds to the same device rows and counts and ORs into the same device masks.  An overlapping pair selects
    // nothing and reads no element: nothing is moved.
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const int mode = flags & 2;
    const uint8_t* src = static_cast<const uint8_t*>(array);
    return fsseg::host_call(
        n, offsets, nseg, 34, fsdrv::chunk_flags() * 2 / W, [&] { return (require & exclude) ? offsets[0] : offsets[nseg]; },
        [&](uint64_t cap) { return cap * W / 2 + ((min_mapq ? cap : 0) + 1) / 2; },
        [&](Engine& e, fsseg::SegBuffers& buf, int sl, uint64_t pos, uint64_t c, uint64_t cap, uint32_t grid) {
            uint8_t* d_mapq = reinterpret_cast<uint8_t*>(e.stage[sl]) + cap * W;
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], src + pos * W, c * W, hipMemcpyHostToDevice, e.stream[sl]));
            if (min_mapq) FS_HIP_TRY(hipMemcpyAsync(d_mapq, mapq + pos, c, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_segments_wide_filter(e.stage[sl], elem_bytes, d_mapq, pos, c, buf.off, nseg, require, exclude, min_mapq,
                                                       buf.cnt, buf.cnt + nseg * 32, buf.cnt + nseg * 33, mode, grid, e.stream[sl]));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_all(out, selected, high, got, nseg, flags); });
}

}  // extern "C"
