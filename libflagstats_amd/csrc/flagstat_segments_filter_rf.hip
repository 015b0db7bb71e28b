// flagstat_segments_filter_rf.hip -- filtered segmented flagstat under samtools' whole view predicate on FLAG and MAPQ: per CSR
// segment of a uint16 FLAG array, the 32 counters of the flags that pass and how many pass, in one launch, where
//   pass(j) = (flag[j] & require) == require && (flag[j] & exclude) == 0
//             && (include_any == 0 || (flag[j] & include_any) != 0)
//             && (exclude_all == 0 || (flag[j] & exclude_all) != exclude_all)
//             && (min_mapq == 0 || mapq[j] >= min_mapq)
// (-f require, -F exclude, --rf / --incl-flags include_any, -G exclude_all, -q min_mapq).  The filtered segmented kernel
// (flagstat_segments_filter.hip) with the whole-column rf kernel's two more tests (flagstat_filter_rf.hip, where they are derived)
// ANDed into the pass word of 4 flags: pass4_rf of flagstat_filter_rf_device.h in place of pass4.
//
// Reduction.  As for whole columns: the launcher first asks the exact host reduction declared in flagstat_filter_rf.h.  A
// predicate that passes nothing launches nothing, a plain require / exclude pair is fsk_launch_segments_filter's -- the parent's
// kernel at the parent's speed -- and only a residue of at least two free bits in --rf or -G reaches the kernel of this file.  It
// is a template on the MAPQ column and on which of the two tests the residue holds, so a test that is off costs nothing: six
// instantiations, none without a test.
//
// Work split, walk, window and emission.  The segmented kernels' shared ones: seg_walk<kSegWaveFlags> and seg_emit<true, false>
// of flagstat_segments_shared.h, taken as they are.  The parent keeps a copy of the walk of its own for 7 % on ~1,000-flag
// segments; this kernel runs only when a residue is left and does not get a third copy (DESIGN.md section 4 has what that costs).
// The number of passing flags is the 22nd lane counter; it is the `len` of the superset slot 9 and lane 32 writes it to
// selected[s].
//   * chain regime: segf_step_and_count's front (flagstat_segments_filter.hip) with pass4_rf: K1's tree_step / end_step at depth
//     kSegFilterDepth, a vector and its MAPQ bytes re-issued as they are consumed.  Every position of such a unit is an element
//     of the segment.
//   * per-flag regime: count_piece_filter's body with pass4_rf.  The pass word is ANDed with nibble_to_bit7(valid_bits) as there:
//     a zero-filled or foreign position fails the any-of test but passes the all-of one, and must count nowhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_engine.h"
#include "flagstat_filter_device.h"
#include "flagstat_filter_rf.h"
#include "flagstat_filter_rf_device.h"
#include "flagstat_segments.h"
#include "flagstat_segments_filter.h"
#include "flagstat_segments_filter_rf.h"
#include "flagstat_segments_shared.h"

namespace fsk {

constexpr int kSegfrRowBytes = kSegRowVecs * 8;   // MAPQ bytes of a row

// K1's step at the default schedule over one unit, the whole predicate applied in the per-vector front: vector u's registers and
// its MAPQ bytes are re-issued for vector u + 6 of the same unit (`cur`) or u - 2 of the next (`next`, if HAS_NEXT).
template <bool MAPQ, bool ANY, bool ALL, bool HAS_NEXT>
__device__ __forceinline__ void segfr_step_and_count(Lane<kSegFilterDepth>& s, const FilterArgs& f, const FilterRfArgs& r,
                                                     uint4 (&v)[kUnroll], uint2 (&m)[kUnroll], uint32_t& blk, uint32_t& cnt,
                                                     const uint4* cur, const uint4* next, const uint8_t* mcur, const uint8_t* mnext)
{
    blk = __builtin_amdgcn_readfirstlane(blk);
    tree_step<kSegFilterDepth>(s, blk, [&](int uu, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        split_out(v[uu], L0, H0, L1, H1);
        uint2 w = make_uint2(0, 0);
        if constexpr (MAPQ) {
            w = m[uu];
            reissue<HAS_NEXT ? 1 : 2>(uu, m, mcur, mnext, kSegfrRowBytes, load_mapq);
        }
        reissue<HAS_NEXT ? 1 : 2>(uu, v, cur, next, kSegRowVecs, load_vec<true>);
        const uint32_t p0 = pass4_rf<MAPQ, ANY, ALL>(f, r, L0, H0, w.x);
        const uint32_t p1 = pass4_rf<MAPQ, ANY, ALL>(f, r, L1, H1, w.y);
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

// the flags of the piece [b, e) that pass, out of the unit starting at grid position w0 (its 8 rows in v[], their MAPQ bytes in
// m[]), into the lane counters and the lane's passing count
template <bool MAPQ, bool ANY, bool ALL>
__device__ __forceinline__ void count_piece_filter_rf(uint32_t (&acc)[kInternal], uint32_t& cnt, const FilterArgs& f, const FilterRfArgs& rf,
                                                      const uint4 (&v)[kUnroll], const uint2 (&m)[kUnroll], uint64_t w0, uint64_t b,
                                                      uint64_t e, uint32_t lane)
{
#pragma unroll
    for (int r = 0; r < kUnroll; ++r) {
        const uint64_t r0 = w0 + static_cast<uint64_t>(r) * 512u;
        if (r0 + 512u <= b || r0 >= e) continue;  // wave-uniform
        uint32_t vb = 0xFFu;                      // bit k: flag k of this lane's vector lies in the piece
        if (r0 < b || r0 + 512u > e) vb = valid_bits(r0 / 8u + lane, b, e);
        const uint4& x = v[r];
        uint32_t L0 = perm(x.y, x.x, 0x06040200u), H0 = perm(x.y, x.x, 0x07050301u);
        uint32_t L1 = perm(x.w, x.z, 0x06040200u), H1 = perm(x.w, x.z, 0x07050301u);
        // in front of the count: a position outside the piece may pass the all-of test
        const uint32_t p0 = pass4_rf<MAPQ, ANY, ALL>(f, rf, L0, H0, m[r].x) & nibble_to_bit7(vb & 15u);
        const uint32_t p1 = pass4_rf<MAPQ, ANY, ALL>(f, rf, L1, H1, m[r].y) & nibble_to_bit7(vb >> 4);
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

// flagstat_segments_filter's arguments (flagstat_segments_filter.hip) with the residue behind `exclude`: the four masks are the
// reduction's, so require & exclude == 0, include_any and exclude_all are disjoint from both, all below 2^16; include_any != 0 iff
// ANY, exclude_all != 0 iff ALL.  min_mapq in 1..255 when MAPQ.  mode: bit 0 store form (out[] and selected[] zeroed in front),
// bit 1 superset.  selected may be nullptr.
template <bool MAPQ, bool ANY, bool ALL>
__global__ __launch_bounds__(kThreads) void flagstat_segments_filter_rf(const uint4* __restrict__ a0, const uint8_t* __restrict__ mq,
                                                                        uint32_t require, uint32_t exclude, uint32_t include_any,
                                                                        uint32_t exclude_all, uint32_t min_mapq, uint64_t lo0,
                                                                        uint64_t hi0, uint64_t base, const uint64_t* __restrict__ off,
                                                                        uint64_t nseg, uint64_t* __restrict__ out,
                                                                        uint64_t* __restrict__ selected, int mode, uint64_t nunits,
                                                                        uint32_t min_units)
{
    static_assert(ANY || ALL, "a plain require / exclude pair is flagstat_segments_filter's");
    __shared__ uint32_t red_all[kThreads / 64][24];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* red = red_all[threadIdx.x >> 6];
    const FilterArgs f = filter_args_of(require, exclude, min_mapq);
    const FilterRfArgs rf = filter_rf_args_of(include_any, exclude_all);
    Lane<kSegFilterDepth> st;
    lane_init(st);
    uint32_t blk = 0;
    uint32_t cnt = 0;   // passing flags of this lane in the open segment
    uint32_t none = 0;  // no mask
    uint4 v[kUnroll];
    uint2 m[kUnroll];
    seg_walk<kSegWaveFlags>(
        lo0, hi0, base, off, nseg, mode, nunits, min_units,
        [&](uint64_t u, uint64_t k) __attribute__((always_inline)) {
            const uint64_t j0 = u * kSegUnitVecs + lane;
            const uint4* p = a0 + j0;
            const uint8_t* pm = mq + j0 * 8;
#pragma unroll
            for (int r = 0; r < kRollDistance; ++r) {
                if constexpr (MAPQ) m[r] = load_mapq(pm + r * kSegfrRowBytes);
                v[r] = load_vec<true>(p + r * kSegRowVecs);
                __builtin_amdgcn_sched_barrier(0);
            }
            for (uint64_t i = 1; i < k; ++i) {
                const uint4* pn = p + kSegUnitVecs;
                const uint8_t* pmn = pm + kSegWaveFlags;
                segfr_step_and_count<MAPQ, ANY, ALL, true>(st, f, rf, v, m, blk, cnt, p, pn, pm, pmn);
                p = pn;
                pm = pmn;
            }
            segfr_step_and_count<MAPQ, ANY, ALL, false>(st, f, rf, v, m, blk, cnt, p, nullptr, pm, nullptr);
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
                }
            }
        },
        [&](uint64_t w0, uint64_t b, uint64_t e) __attribute__((always_inline)) {
            count_piece_filter_rf<MAPQ, ANY, ALL>(st.acc, cnt, f, rf, v, m, w0, b, e, lane);
        },
        [&](uint64_t s, uint64_t len, bool plain) __attribute__((always_inline)) {
            seg_emit<true, false>(st, blk, cnt, none, none, red, out, selected, nullptr, s, len, plain, mode, lane);
        });
}

}  // namespace fsk

// ------------------------------------------------------------------ launcher
namespace {

template <bool MAPQ>
void launch_residue(bool any, bool all, dim3 g, dim3 b, hipStream_t stream, const uint4* a0, const uint8_t* mq, const uint32_t (&r)[4],
                    uint32_t min_mapq, uint64_t lo0, uint64_t hi0, uint64_t base, const uint64_t* d_offsets, uint64_t nseg,
                    uint64_t* d_out, uint64_t* d_selected, int mode, uint64_t nunits, uint32_t min_units)
{
    auto* kernel = any && all ? fsk::flagstat_segments_filter_rf<MAPQ, true, true>
                   : any      ? fsk::flagstat_segments_filter_rf<MAPQ, true, false>
                              : fsk::flagstat_segments_filter_rf<MAPQ, false, true>;
    hipLaunchKernelGGL(kernel, g, b, 0, stream, a0, mq, r[0], r[1], r[2], r[3], min_mapq, lo0, hi0, base, d_offsets, nseg, d_out,
                       d_selected, mode, nunits, min_units);
}

}  // namespace

extern "C" hipError_t fsk_launch_segments_filter_rf(const uint16_t* d_chunk, const uint8_t* d_mapq_chunk, uint64_t base, uint64_t m,
                                                    const uint64_t* d_offsets, uint64_t nseg, uint32_t require, uint32_t exclude,
                                                    uint32_t include_any, uint32_t exclude_all, uint32_t min_mapq, uint64_t* d_out,
                                                    uint64_t* d_selected, int mode, uint32_t grid, hipStream_t stream)
{
    if (require > 0xFFFFu || exclude > 0xFFFFu || include_any > 0xFFFFu || exclude_all > 0xFFFFu) return hipErrorInvalidValue;
    uint32_t r[4];
    const int kind = fsk_filter_rf_reduce(require, exclude, include_any, exclude_all, r);
    // a plain pair is the parent's kernel; so is an empty predicate, as the overlapping pair that launcher answers itself
    if (kind == 1)
        return fsk_launch_segments_filter(d_chunk, d_mapq_chunk, base, m, d_offsets, nseg, r[0], r[1], min_mapq, d_out, d_selected, mode,
                                          grid, stream);
    if (kind == 0)
        return fsk_launch_segments_filter(d_chunk, d_mapq_chunk, base, m, d_offsets, nseg, 1u, 1u, min_mapq, d_out, d_selected, mode, grid,
                                          stream);
    if ((mode & ~3) || grid == 0 || min_mapq > 255u) return hipErrorInvalidValue;
    if (nseg == 0) return hipSuccess;
    if (d_out == nullptr || d_offsets == nullptr || (m && (d_chunk == nullptr || (min_mapq && d_mapq_chunk == nullptr))))
        return hipErrorInvalidValue;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(d_chunk);
    if ((addr & 1u) || m > (~0ull - 64) / 2) return hipErrorInvalidValue;
    uint64_t lo0 = 0, nunits = 0;
    uint32_t g = 0;
    if (m) {
        fsseg::launch_shape(addr, m, fsk::kSegWaveFlags, grid, &lo0, &nunits, &g);
        if (!fsseg::wave_totals_fit(nunits, g, fsk::kSegWaveFlags)) return hipErrorInvalidValue;
    }
    if (mode & 1) {
        hipError_t e = fsk_zero_words(d_out, nseg * 32, stream);
        if (e == hipSuccess && d_selected) e = fsk_zero_words(d_selected, nseg, stream);
        if (e != hipSuccess) return e;
    }
    if (m == 0) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(addr & ~static_cast<uintptr_t>(15));
    const uint64_t hi0 = lo0 + m;
    uint32_t min_units = 0, blocks_per_cu = 0;
    fsk_segments_policy(&min_units, &blocks_per_cu);
    const dim3 gd(g), bd(fsk::kThreads);
    if (min_mapq) {
        // grid position q is element q - lo0 of the chunk: its byte is d_mapq_chunk[q - lo0]
        const uint8_t* mq = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_mapq_chunk) - lo0);
        launch_residue<true>(r[2] != 0, r[3] != 0, gd, bd, stream, a0, mq, r, min_mapq, lo0, hi0, base, d_offsets, nseg, d_out, d_selected,
                             mode & 3, nunits, min_units);
    } else {
        launch_residue<false>(r[2] != 0, r[3] != 0, gd, bd, stream, a0, nullptr, r, 0u, lo0, hi0, base, d_offsets, nseg, d_out, d_selected,
                              mode & 3, nunits, min_units);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The bodies of the three forms are fsseg's (flagstat_segments_shared.h): 33 words per segment, the rows, then the selected counts.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU (nseg > 0 from the NULL checks on): segf_args' refusals
// (flagstat_segments_filter.hip) with the two new masks asked after the predicate and before the flags
int segfr_args(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg, uint32_t require, uint32_t exclude,
               uint32_t include_any, uint32_t exclude_all, const uint8_t* mapq, uint32_t min_mapq, const void* out, int flags,
               const char* null_text)
{
    using namespace fsdrv;
    if (check_predicate(require, exclude, min_mapq) || check_predicate_rf(include_any, exclude_all) || check_flags(flags)) return -1;
    if (nseg == 0) return 0;
    return refused(fsseg::check_segments(offsets, out, nseg, null_text, fsseg::kMaxSegments / 2) || check_array_given(array, n) ||
                   check_mapq_given(mapq, n, min_mapq) || check_array_layout(array, n, 2));
}

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_u16_segments_filter_rf(const uint16_t* d_array, uint64_t n, const uint64_t* d_offsets, uint64_t nseg,
                                                uint32_t require, uint32_t exclude, uint32_t include_any, uint32_t exclude_all,
                                                const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected,
                                                int flags, void* stream)
{
    FS_ENTRY();
    int rc = segfr_args(d_array, n, d_offsets, nseg, require, exclude, include_any, exclude_all, d_mapq, min_mapq, d_out, flags,
                        fsseg::kNullDevice);
    if (rc || nseg == 0) return rc;
    const fsdrv::DeviceWord word{d_selected, "d_selected", "the counts are added with device atomics"};
    fsdrv::Inputs in = fsseg::offsets_input(d_offsets, nseg);
    in.add_columns(d_array, n, 2, nullptr, 0, 0, d_mapq, min_mapq);
    return fsseg::device_call(
        d_out, &word, 1, in.in, in.count, nseg, stream,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWaveFlags, grid); },
        [&](uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_filter_rf(d_array, d_mapq, 0, n, d_offsets, nseg, require, exclude, include_any, exclude_all,
                                                     min_mapq, d_out, d_selected, flags & 3, grid, s));
            return 0;
        });
}

int FLAGSTATS_hip_device_u16_segments_filter_rf_sync(const uint16_t* d_array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                                     uint32_t require, uint32_t exclude, uint32_t include_any, uint32_t exclude_all,
                                                     const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* out, uint64_t* selected,
                                                     int flags)
{
    FS_ENTRY();
    int rc = segfr_args(d_array, n, offsets, nseg, require, exclude, include_any, exclude_all, d_mapq, min_mapq, out, flags,
                        fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, nullptr, 0, 0, d_mapq, min_mapq);
    return fsseg::sync_call(
        in.in, in.count, n, offsets, nseg, 33,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWaveFlags, grid); },
        [&](fsseg::SegBuffers& buf, uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_filter_rf(d_array, d_mapq, 0, n, buf.off, nseg, require, exclude, include_any, exclude_all,
                                                     min_mapq, buf.cnt, buf.cnt + nseg * 32, 1 | (flags & 2), grid, s));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_both(out, selected, got, nseg, flags); });
}

int FLAGSTATS_hip_u16_x64_segments_filter_rf(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg, uint32_t require,
                                             uint32_t exclude, uint32_t include_any, uint32_t exclude_all, const uint8_t* mapq,
                                             uint32_t min_mapq, uint64_t* out, uint64_t* selected, int flags)
{
    FS_ENTRY();
    int rc = segfr_args(array, n, offsets, nseg, require, exclude, include_any, exclude_all, mapq, min_mapq, out, flags, fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    // a chunk's slice of the MAPQ column rides in the same staging buffer, behind the flags.  A predicate that passes nothing
    // selects nothing: nothing is moved.
    uint32_t reduced[4];
    const bool empty = fsk_filter_rf_reduce(require, exclude, include_any, exclude_all, reduced) == 0;
    const int mode = flags & 2;
    return fsseg::host_call(
        n, offsets, nseg, 33, fsdrv::chunk_flags(), [&] { return empty ? offsets[0] : offsets[nseg]; },
        [&](uint64_t cap) { return cap + ((min_mapq ? cap : 0) + 1) / 2; },
        [&](Engine& e, fsseg::SegBuffers& buf, int sl, uint64_t pos, uint64_t c, uint64_t cap, uint32_t grid) {
            uint8_t* d_mapq = reinterpret_cast<uint8_t*>(e.stage[sl] + cap);
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], array + pos, c * sizeof(uint16_t), hipMemcpyHostToDevice, e.stream[sl]));
            if (min_mapq) FS_HIP_TRY(hipMemcpyAsync(d_mapq, mapq + pos, c, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_segments_filter_rf(e.stage[sl], d_mapq, pos, c, buf.off, nseg, require, exclude, include_any, exclude_all,
                                                     min_mapq, buf.cnt, buf.cnt + nseg * 32, mode, grid, e.stream[sl]));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_both(out, selected, got, nseg, flags); });
}

}  // extern "C"
