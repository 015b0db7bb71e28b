// flagstat_segments_filter_where.hip -- filtered AND selected segmented flagstat: per CSR segment of a uint16 FLAG array, the 32
// counters of the flags that pass samtools' view filter and that a selection selects, and how many those are, in one launch:
//   counted(j) = pass(j) && sel(j)
// with pass flagstat_segments_filter.hip's predicate (-f require, -F exclude, -q min_mapq over a uint8 MAPQ column) and sel
// flagstat_segments_where.hip's selection, indexed by ARRAY ELEMENT (an LSB-first bitmap that may start at any bit, or one byte per
// element, any non-zero byte selects).  The case of a FLAG column with a validity bitmap under -F 0x904 -q 30 per row group,
// contig, sample or block.  The cross of the two segmented parents, with flagstat_filter_where.hip's way of joining the two
// tests: the selection is ANDed into pass4's word in registers (counted_bits / counted_bytes, flagstat_filter_where_device.h); no
// selector table in LDS, no combined mask in memory.
//
// Forms.  The kernel is a template on <MAPQ, SEL_BITS, FUNNEL>; five instantiations exist: the bitmap with and without the
// column, each at a byte boundary of the grid (one selection byte per vector) and off it (FUNNEL: two bytes funnelled together),
// and the byte mask with the column.  The sixth form, a byte mask without -q, has no kernel: flagstat_segments_filter<true> with
// the caller's require / exclude, the mask as its MAPQ column and min_mapq == 1 is exactly "passes the FLAG test and the byte is
// not zero" (the derivation stands at the top of flagstat_segments_where.hip; there with require == exclude == 0, but the MAPQ
// half of pass4 does not depend on the FLAG half).  The launcher hands that form to fsk_launch_segments_filter.
//
// Work split, walk, window and emission.  The segmented kernels' shared ones (tests/segments_oracle.WriterSplit mirrors them):
// units of 4096 flags on the 16-byte grid of the array's aligned-down base, every wave a writer over a contiguous run of units,
// lane l of a row takes vector row * 64 + l, the 64-ary search for a writer's first segment, the window of 64 offsets, plain
// stores in the store form for rows that lie inside one writer: seg_walk<kSegWaveFlags> and seg_emit<true, false> of
// flagstat_segments_shared.h, taken as they are -- with the shared walk every instantiation keeps the parents' 2 waves per SIMD
// and no scratch (profiles/r21/resource_usage.log), so this unit has no copy of the walk.  The number of counted flags is the
// 22nd lane counter; it is the `len` of the superset slot 9 and lane 32 writes it to selected[s].
//
// Addresses.  The array and the MAPQ column as in flagstat_segments_filter.hip (`mq` such that the byte of grid position q is
// mq[q]), the selection as in flagstat_segments_where.hip (`sel` such that the 8 bits of grid vector j start at bit `shift` of
// sel[j], or such that the byte of grid position q is sel[q]; the launcher takes both from fsk_segments_where_geometry).
//   * chain regime (a run of at least `min_units` whole units in one segment): K1's tree_step / end_step with the filtered
//     segmented kernel's front and, as in filter_where_step_and_count, the selection of a vector re-issued next to its MAPQ bytes
//     and in front of the vector itself, read out with it; after pass4 the selection clears the pass bits of the flags it does
//     not select, then the popcount into the lane's count, the v_perm_b32 masks and the AND onto the planes.  Every position of
//     such a unit is an element of the segment.  Nothing is carried between units, so a run needs no priming.
//   * per-flag regime: the unit's 8 rows, their MAPQ bytes and their selection are loaded at once -- through the guarded loaders,
//     which touch only bytes that hold an element (its flag, its MAPQ byte, its bit or byte), when the unit is the array's ragged
//     first or last -- with the bitmap's bits brought to bit 0.  Per piece and row: the bitmap's bits are ANDed with the piece's
//     valid_bits and their two nibbles go through counted_bits onto pass4's word, so piece bounds and selection cost one AND
//     together (the filtered parent's nibble_to_bit7 is not needed); the byte form goes through counted_bytes and then the
//     parent's nibble_to_bit7(valid_bits).  A selected, passing flag of a neighbouring segment, of a gap or of the bytes around
//     the array has its pass bit cleared there and counts nowhere.
//
// What a funnelled launch reads of the selection.  A funnelled 16-bit load for grid vector j reads sel[j] and sel[j + 1].  Plain
// loads are issued only for units that lie wholly inside [lo0, hi0) (the walk chains only such units, and hands `whole` to the
// per-flag load).  If lo0 > 0 the array starts inside unit 0, which is then ragged: it is never chained and goes through
// load_sel_guarded, which reads sel[j] only if it holds the bit of an element.  So a plain load of vector 0 of unit 0 happens
// only with lo0 == 0, where sel[0] is the byte of element 0's bit (shift = sel_offset & 7).  The last vector of a whole unit ends
// at a position <= hi0, its 8 bits are bits [shift, shift + 8) of the pair, and shift >= 1 puts its last element's bit into
// sel[j + 1]: the second byte of every plain load holds an element's bit, none lies past the byte of the last element's bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_engine.h"
#include "flagstat_filter_device.h"
#include "flagstat_filter_where_device.h"
#include "flagstat_segments.h"
#include "flagstat_segments_filter.h"
#include "flagstat_segments_filter_where.h"
#include "flagstat_segments_shared.h"
#include "flagstat_segments_where.h"
#include "flagstat_where.h"
#include "flagstat_where_device.h"

namespace fsk {

constexpr int kSegfwRowBytes = kSegRowVecs * 8;   // MAPQ bytes, or selection bytes of the byte form, of a row

// K1's step at the default schedule over one unit, predicate and selection applied in the per-vector front: vector u's
// registers, its MAPQ bytes and its selection are re-issued for vector u + 6 of the same unit (`cur`) or u - 2 of the next
// (`next`, if HAS_NEXT).  sh: the bit of x[] at which a vector's 8 selection bits start (bitmap).
template <bool MAPQ, int SEL_BITS, bool FUNNEL, bool HAS_NEXT>
__device__ __forceinline__ void segfw_step_and_count(Lane<kSegFilterDepth>& s, const FilterArgs& f, uint4 (&v)[kUnroll], uint2 (&m)[kUnroll],
                                                     typename SelWord<SEL_BITS>::type (&x)[kUnroll], uint32_t& blk, uint32_t sh,
                                                     uint32_t& cnt, const uint4* cur, const uint4* next, const uint8_t* mcur,
                                                     const uint8_t* mnext, const uint8_t* scur, const uint8_t* snext)
{
    constexpr int ROLL = HAS_NEXT ? 1 : 2;
    constexpr int SS = SEL_BITS == 1 ? kSegRowVecs : kSegfwRowBytes;   // selection bytes between a lane's consecutive vectors
    blk = __builtin_amdgcn_readfirstlane(blk);
    tree_step<kSegFilterDepth>(s, blk, [&](int uu, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        split_out(v[uu], L0, H0, L1, H1);
        uint2 w = make_uint2(0, 0);
        if constexpr (MAPQ) {
            w = m[uu];
            reissue<ROLL>(uu, m, mcur, mnext, kSegfwRowBytes, load_mapq);
        }
        const typename SelWord<SEL_BITS>::type c = x[uu];
        reissue<ROLL>(uu, x, scur, snext, SS, load_sel<SEL_BITS, FUNNEL>);
        reissue<ROLL>(uu, v, cur, next, kSegRowVecs, load_vec<true>);
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
    end_step<kSegFilterDepth>(s, blk);
}

// the flags of the piece [b, e) that pass and are selected, out of the unit starting at grid position w0 (its 8 rows in v[],
// their MAPQ bytes in m[], their selection in x[]: the bitmap's bits at bit 0), into the lane counters and the lane's count
template <bool MAPQ, int SEL_BITS>
__device__ __forceinline__ void count_piece_filter_where(uint32_t (&acc)[kInternal], uint32_t& cnt, const FilterArgs& f,
                                                         const uint4 (&v)[kUnroll], const uint2 (&m)[kUnroll],
                                                         const typename SelWord<SEL_BITS>::type (&x)[kUnroll], uint64_t w0, uint64_t b,
                                                         uint64_t e, uint32_t lane)
{
#pragma unroll
    for (int r = 0; r < kUnroll; ++r) {
        const uint64_t r0 = w0 + static_cast<uint64_t>(r) * 512u;
        if (r0 + 512u <= b || r0 >= e) continue;  // wave-uniform
        uint32_t vb = 0xFFu;                      // bit k: flag k of this lane's vector lies in the piece
        if (r0 < b || r0 + 512u > e) vb = valid_bits(r0 / 8u + lane, b, e);
        const uint4& y = v[r];
        uint32_t L0 = perm(y.y, y.x, 0x06040200u), H0 = perm(y.y, y.x, 0x07050301u);
        uint32_t L1 = perm(y.w, y.z, 0x06040200u), H1 = perm(y.w, y.z, 0x07050301u);
        uint32_t p0 = pass4<MAPQ>(f, L0, H0, m[r].x);
        uint32_t p1 = pass4<MAPQ>(f, L1, H1, m[r].y);
        if constexpr (SEL_BITS == 1) {
            const uint32_t bits = x[r] & vb;      // ... and is selected (x[r] < 256)
            p0 = counted_bits(p0, bits & 15u);
            p1 = counted_bits(p1, bits >> 4);
        } else {
            p0 = counted_bytes(p0, x[r].x) & nibble_to_bit7(vb & 15u);
            p1 = counted_bytes(p1, x[r].y) & nibble_to_bit7(vb >> 4);
        }
        cnt += __builtin_popcount(p0);
        cnt += __builtin_popcount(p1);
        const uint32_t M0 = perm(0u, 0u, p0), M1 = perm(0u, 0u, p1);
        L0 &= M0;
        H0 &= M0;
        L1 &= M1;
        H1 &= M1;
        count_planes(acc, L0, H0, L1, H1);
    }
}

// a0: 16-B aligned-down base; the chunk's flags occupy grid positions [lo0, hi0) and are global flags [base, base + hi0 - lo0).
// mq: the chunk's MAPQ column on the same grid (the byte of position q is mq[q]; not read when !MAPQ).  sel, shift: the chunk's
// selection on the same grid (bitmap: the 8 bits of grid vector j start at bit `shift` of sel[j], FUNNEL: shift != 0; bytes: the
// byte of position q is sel[q]).  require & exclude == 0 (the launcher's business), both below 2^16, min_mapq in 1..255 when
// MAPQ.  nunits = ceil(hi0 / 4096).  mode: bit 0 store form (out[] and selected[] zeroed in front), bit 1 superset.  selected may
// be nullptr.
template <bool MAPQ, int SEL_BITS, bool FUNNEL>
__global__ __launch_bounds__(kThreads) void flagstat_segments_filter_where(const uint4* __restrict__ a0, const uint8_t* __restrict__ mq,
                                                                           const uint8_t* __restrict__ sel, uint32_t shift,
                                                                           uint32_t require, uint32_t exclude, uint32_t min_mapq,
                                                                           uint64_t lo0, uint64_t hi0, uint64_t base,
                                                                           const uint64_t* __restrict__ off, uint64_t nseg,
                                                                           uint64_t* __restrict__ out, uint64_t* __restrict__ selected,
                                                                           int mode, uint64_t nunits, uint32_t min_units)
{
    static_assert(SEL_BITS == 1 || (SEL_BITS == 8 && !FUNNEL && MAPQ), "a bitmap (at a byte boundary of the grid or not), or bytes with -q");
    typedef typename SelWord<SEL_BITS>::type sel_t;
    constexpr int SB = SEL_BITS == 1 ? 1 : 8;   // selection bytes per vector
    __shared__ uint32_t red_all[kThreads / 64][24];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* red = red_all[threadIdx.x >> 6];
    const uint32_t sh = FUNNEL ? __builtin_amdgcn_readfirstlane(shift) : 0u;
    const FilterArgs f = filter_args_of(require, exclude, min_mapq);
    Lane<kSegFilterDepth> st;
    lane_init(st);
    uint32_t blk = 0;
    uint32_t cnt = 0;   // counted flags of this lane in the open segment
    uint32_t none = 0;  // no mask
    uint4 v[kUnroll];
    uint2 m[kUnroll];
    sel_t x[kUnroll];
    seg_walk<kSegWaveFlags>(
        lo0, hi0, base, off, nseg, mode, nunits, min_units,
        [&](uint64_t u, uint64_t k) __attribute__((always_inline)) {
            const uint64_t j0 = u * kSegUnitVecs + lane;
            const uint4* p = a0 + j0;
            const uint8_t* pm = mq + j0 * 8;
            const uint8_t* ps = sel + j0 * SB;
#pragma unroll
            for (int r = 0; r < kRollDistance; ++r) {
                if constexpr (MAPQ) m[r] = load_mapq(pm + r * kSegfwRowBytes);
                x[r] = load_sel<SEL_BITS, FUNNEL>(ps + r * kSegRowVecs * SB);
                v[r] = load_vec<true>(p + r * kSegRowVecs);
                __builtin_amdgcn_sched_barrier(0);
            }
            for (uint64_t i = 1; i < k; ++i) {
                const uint4* pn = p + kSegUnitVecs;
                const uint8_t* pmn = pm + kSegWaveFlags;
                const uint8_t* psn = ps + kSegUnitVecs * SB;
                segfw_step_and_count<MAPQ, SEL_BITS, FUNNEL, true>(st, f, v, m, x, blk, sh, cnt, p, pn, pm, pmn, ps, psn);
                p = pn;
                pm = pmn;
                ps = psn;
            }
            segfw_step_and_count<MAPQ, SEL_BITS, FUNNEL, false>(st, f, v, m, x, blk, sh, cnt, p, nullptr, pm, nullptr, ps, nullptr);
        },
        [&](uint64_t u, bool whole) __attribute__((always_inline)) {
            const uint64_t j0 = u * kSegUnitVecs + lane;
            if (whole) {
#pragma unroll
                for (int r = 0; r < kUnroll; ++r) {
                    const uint64_t j = j0 + r * kSegRowVecs;
                    v[r] = load_vec<true>(a0 + j);
                    if constexpr (MAPQ)
                        m[r] = load_mapq(mq + j * 8);
                    else
                        m[r] = make_uint2(0, 0);
                    if constexpr (SEL_BITS == 1)
                        x[r] = __builtin_amdgcn_ubfe(load_sel<1, FUNNEL>(sel + j), sh, 8);
                    else
                        x[r] = load_sel<8, false>(sel + j * 8);
                }
            } else {
#pragma unroll
                for (int r = 0; r < kUnroll; ++r) {
                    const uint64_t j = j0 + r * kSegRowVecs;
                    v[r] = load_guarded(a0, j, lo0, hi0);
                    if constexpr (MAPQ)
                        m[r] = load_mapq_guarded(mq, j, lo0, hi0);
                    else
                        m[r] = make_uint2(0, 0);
                    x[r] = load_sel_guarded<SEL_BITS>(sel, sh, j, lo0, hi0);
                }
            }
        },
        [&](uint64_t w0, uint64_t b, uint64_t e) __attribute__((always_inline)) {
            count_piece_filter_where<MAPQ, SEL_BITS>(st.acc, cnt, f, v, m, x, w0, b, e, lane);
        },
        [&](uint64_t s, uint64_t len, bool plain) __attribute__((always_inline)) {
            seg_emit<true, false>(st, blk, cnt, none, none, red, out, selected, nullptr, s, len, plain, mode, lane);
        });
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
using fsdrv::where_extent;

extern "C" hipError_t fsk_launch_segments_filter_where(const uint16_t* d_chunk, const uint8_t* d_mapq_chunk, const void* d_sel,
                                                       uint64_t sel_offset, int sel_bits, uint64_t base, uint64_t m,
                                                       const uint64_t* d_offsets, uint64_t nseg, uint32_t require, uint32_t exclude,
                                                       uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected, int mode, uint32_t grid,
                                                       hipStream_t stream)
{
    if ((sel_bits != 1 && sel_bits != 8) || (mode & ~3) || grid == 0 || require > 0xFFFFu || exclude > 0xFFFFu || min_mapq > 255u)
        return hipErrorInvalidValue;
    if (nseg == 0) return hipSuccess;
    if (d_out == nullptr || d_offsets == nullptr ||
        (m && (d_chunk == nullptr || d_sel == nullptr || (min_mapq && d_mapq_chunk == nullptr))))
        return hipErrorInvalidValue;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_chunk);
    uint64_t geo[7];
    hipError_t e = fsk_segments_where_geometry(addr, m, sel_offset, sel_bits, grid, geo);
    if (e != hipSuccess) return e;
    if (sel_bits == 8 && min_mapq == 0)  // the mask is the filtered kernel's MAPQ column (see the top), taken from element 0 on
        return fsk_launch_segments_filter(d_chunk, static_cast<const uint8_t*>(d_sel) + sel_offset, base, m, d_offsets, nseg, require,
                                          exclude, 1u, d_out, d_selected, mode, grid, stream);
    if (mode & 1) {
        e = fsk_zero_words(d_out, nseg * 32, stream);
        if (e == hipSuccess && d_selected) e = fsk_zero_words(d_selected, nseg, stream);
        if (e != hipSuccess) return e;
    }
    // a bit both required and excluded: no flag passes (samtools accepts the pair); the kernel's test assumes a disjoint pair
    if (m == 0 || (require & exclude)) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(addr & ~static_cast<uintptr_t>(15));
    const uint64_t lo0 = geo[0], hi0 = lo0 + m, nunits = geo[1];
    const uint8_t* sel = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_sel) + geo[3]);
    const uint32_t shift = static_cast<uint32_t>(geo[4]);
    // grid position q is element q - lo0 of the chunk: its MAPQ byte is d_mapq_chunk[q - lo0]
    const uint8_t* mq = min_mapq ? reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_mapq_chunk) - lo0) : nullptr;
    uint32_t min_units = 0, blocks_per_cu = 0;
    fsk_segments_policy(&min_units, &blocks_per_cu);
    const dim3 gd(static_cast<uint32_t>(geo[2])), bd(fsk::kThreads);
#define FSK_SFW_LAUNCH(MAPQ_, BITS_, FUNNEL_)                                                                                              \
    hipLaunchKernelGGL((fsk::flagstat_segments_filter_where<MAPQ_, BITS_, FUNNEL_>), gd, bd, 0, stream, a0, mq, sel, shift, require, exclude, \
                       min_mapq, lo0, hi0, base, d_offsets, nseg, d_out, d_selected, mode & 3, nunits, min_units)
    if (sel_bits == 8)
        FSK_SFW_LAUNCH(true, 8, false);
    else if (min_mapq && shift)
        FSK_SFW_LAUNCH(true, 1, true);
    else if (min_mapq)
        FSK_SFW_LAUNCH(true, 1, false);
    else if (shift)
        FSK_SFW_LAUNCH(false, 1, true);
    else
        FSK_SFW_LAUNCH(false, 1, false);
#undef FSK_SFW_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The bodies of the three forms are fsseg's (flagstat_segments_shared.h): 33 words per segment, the rows, then the counts.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU (nseg > 0 from the NULL checks on): segf_args' and segw_args' refusals
int segfw_args(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg, uint32_t require, uint32_t exclude,
               const uint8_t* mapq, uint32_t min_mapq, const void* sel, uint64_t sel_offset, int sel_bits, const void* out, int flags,
               const char* null_text)
{
    using namespace fsdrv;
    if (check_predicate(require, exclude, min_mapq) || check_sel_bits(sel_bits) || check_flags(flags)) return -1;
    if (nseg == 0) return 0;
    return refused(fsseg::check_segments(offsets, out, nseg, null_text, fsseg::kMaxSegments / 2) || check_array_given(array, n) ||
                   check_mapq_given(mapq, n, min_mapq) || check_sel_given(sel, n) || check_array_layout(array, n, 2) ||
                   check_sel_range(sel_offset, n));
}

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_u16_segments_filter_where(const uint16_t* d_array, uint64_t n, const uint64_t* d_offsets, uint64_t nseg,
                                                   uint32_t require, uint32_t exclude, const uint8_t* d_mapq, uint32_t min_mapq,
                                                   const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* d_out,
                                                   uint64_t* d_selected, int flags, void* stream)
{
    FS_ENTRY();
    int rc = segfw_args(d_array, n, d_offsets, nseg, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits, d_out, flags,
                        fsseg::kNullDevice);
    if (rc || nseg == 0) return rc;
    const fsdrv::DeviceWord word{d_selected, "d_selected", "the counts are added with device atomics"};
    fsdrv::Inputs in = fsseg::offsets_input(d_offsets, nseg);
    in.add_columns(d_array, n, 2, d_sel, sel_offset, sel_bits, d_mapq, min_mapq);
    return fsseg::device_call(
        d_out, &word, 1, in.in, in.count, nseg, stream,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWaveFlags, grid); },
        [&](uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_filter_where(d_array, d_mapq, d_sel, sel_offset, sel_bits, 0, n, d_offsets, nseg, require, exclude,
                                                        min_mapq, d_out, d_selected, flags & 3, grid, s));
            return 0;
        });
}

int FLAGSTATS_hip_device_u16_segments_filter_where_sync(const uint16_t* d_array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                                        uint32_t require, uint32_t exclude, const uint8_t* d_mapq, uint32_t min_mapq,
                                                        const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* out,
                                                        uint64_t* selected, int flags)
{
    FS_ENTRY();
    int rc = segfw_args(d_array, n, offsets, nseg, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits, out, flags,
                        fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, d_sel, sel_offset, sel_bits, d_mapq, min_mapq);
    return fsseg::sync_call(
        in.in, in.count, n, offsets, nseg, 33,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWaveFlags, grid); },
        [&](fsseg::SegBuffers& buf, uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_filter_where(d_array, d_mapq, d_sel, sel_offset, sel_bits, 0, n, buf.off, nseg, require, exclude,
                                                        min_mapq, buf.cnt, buf.cnt + nseg * 32, 1 | (flags & 2), grid, s));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_both(out, selected, got, nseg, flags); });
}

int FLAGSTATS_hip_u16_x64_segments_filter_where(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                                uint32_t require, uint32_t exclude, const uint8_t* mapq, uint32_t min_mapq,
                                                const void* sel, uint64_t sel_offset, int sel_bits, uint64_t* out, uint64_t* selected,
                                                int flags)
{
    FS_ENTRY();
    int rc = segfw_args(array, n, offsets, nseg, require, exclude, mapq, min_mapq, sel, sel_offset, sel_bits, out, flags,
                        fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    // a chunk's slices of the MAPQ column and of the selection ride in the same staging buffer, behind the flags: the column's
    // first, then the selection's -- a bitmap slice from the byte that holds the chunk's first bit (the launch then starts
    // (sel_offset + pos) & 7 bits into it).  An overlapping pair counts nothing: nothing is moved.
    const int mode = flags & 2;
    const uint8_t* sel_src = static_cast<const uint8_t*>(sel);
    auto mapq_slot = [&](uint64_t cap) { return min_mapq ? (cap + 1) / 2 : 0; };   // a chunk's MAPQ slice, in uint16
    return fsseg::host_call(
        n, offsets, nseg, 33, fsdrv::chunk_flags(), [&] { return (require & exclude) ? offsets[0] : offsets[nseg]; },
        [&](uint64_t cap) { return cap + mapq_slot(cap) + ((sel_bits == 1 ? (cap + 7) / 8 + 1 : cap) + 1) / 2; },
        [&](Engine& e, fsseg::SegBuffers& buf, int sl, uint64_t pos, uint64_t c, uint64_t cap, uint32_t grid) {
            uint64_t sel_first, sel_len;
            where_extent(c, sel_offset + pos, sel_bits, &sel_first, &sel_len);
            uint8_t* d_mapq = reinterpret_cast<uint8_t*>(e.stage[sl] + cap);
            uint8_t* d_sel = reinterpret_cast<uint8_t*>(e.stage[sl] + cap + mapq_slot(cap));
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], array + pos, c * sizeof(uint16_t), hipMemcpyHostToDevice, e.stream[sl]));
            if (min_mapq) FS_HIP_TRY(hipMemcpyAsync(d_mapq, mapq + pos, c, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(hipMemcpyAsync(d_sel, sel_src + sel_first, sel_len, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_segments_filter_where(e.stage[sl], d_mapq, d_sel, sel_bits == 1 ? (sel_offset + pos) & 7 : 0, sel_bits, pos,
                                                        c, buf.off, nseg, require, exclude, min_mapq, buf.cnt, buf.cnt + nseg * 32, mode, grid,
                                                        e.stream[sl]));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_both(out, selected, got, nseg, flags); });
}

}  // extern "C"
