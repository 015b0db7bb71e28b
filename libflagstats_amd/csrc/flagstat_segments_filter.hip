// flagstat_segments_filter.hip -- filtered segmented flagstat: per CSR segment of a uint16 FLAG array, the 32 counters of the
// flags that pass samtools' view filter and how many pass, in one launch:
//   pass(j) = (flag[j] & require) == require && (flag[j] & exclude) == 0 && (min_mapq == 0 || mapq[j] >= min_mapq).
// The segmented kernel (flagstat_segments.hip) with the filter kernel's predicate (flagstat_filter.hip) in front of the count.
//
// Work split and walk.  The segmented kernels' (tests/segments_oracle.WriterSplit mirrors them) -- but this kernel keeps its own
// copy of the walk that flagstat_segments, flagstat_segments_wide and flagstat_segments_where take from flagstat_segments_shared.h
// (seg_walk<UE>): in the shared form it was 7 % slower on ~1,000-flag segments (profiles/r18/ab_flagstat_segments_filter.log).  A
// change to the walk is made there and here.  Units of 4096 flags
// on the 16-byte grid of the array's aligned-down base, every wave a writer over a contiguous run of units, the 64-ary search
// for its first segment, the window of 64 offsets, plain stores in the store form for rows that lie inside one writer.  The
// pieces shared with that kernel live in flagstat_segments_shared.h, those shared with the filter kernel in
// flagstat_filter_device.h.
//
// Predicate.  A zero flag counts in no slot, so filtering is zeroing the flags that fail on their byte planes, in front of
// front4 (pass4 and the v_perm_b32 mask; derivation in flagstat_filter.hip).  The MAPQ column is addressed like the filter
// kernel's: `mq` is such that the byte of grid position q is mq[q], one unaligned dwordx2 per vector.  The kernel is a template
// on whether the column is read at all.
//   * chain regime (a run of at least `min_units` whole units in one segment): K1's tree_step / end_step with the filter
//     kernel's per-vector front; a vector's MAPQ bytes are loaded with it through reissue.  Every position of such a unit is an
//     element of the segment, so no position needs masking.
//   * per-flag regime: the unit's 8 rows and their MAPQ bytes are loaded at once (through guarded loaders that touch only
//     elements when the unit is the array's ragged first or last).  Per piece and row, the pass bits of positions outside the
//     piece are cleared (valid_bits / nibble_to_bit7), which zeroes those flags with the failing ones -- the pass mask does the
//     piece bounds, there is no separate masking of the vector -- and keeps them out of the passing count: a zero-filled or
//     foreign position passes every predicate without `require` bits.
//
// Emission (seg_emit<true, false> of flagstat_segments_shared.h).  The number of passing flags is a 22nd lane counter, reduced and
// reset with the 21 at a segment end; it is the
// `len` of the superset slot 9, and lane 32 of the instruction that writes the row's 32 slots writes selected[s]: a plain
// store where the row is stored plainly, else a relaxed agent-scope atomic add.
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

namespace fsk {

constexpr int kSegRowBytes = kSegRowVecs * 8;      // MAPQ bytes of a row

// K1's step at the default schedule over one unit, the predicate applied in the per-vector front: vector u's registers and its
// MAPQ bytes are re-issued for vector u + 6 of the same unit (`cur`) or u - 2 of the next (`next`, if HAS_NEXT).
template <bool MAPQ, bool HAS_NEXT>
__device__ __forceinline__ void segf_step_and_count(Lane<kSegFilterDepth>& s, const FilterArgs& f, uint4 (&v)[kUnroll], uint2 (&m)[kUnroll],
                                                    uint32_t& blk, uint32_t& cnt, const uint4* cur, const uint4* next,
                                                    const uint8_t* mcur, const uint8_t* mnext)
{
    blk = __builtin_amdgcn_readfirstlane(blk);
    tree_step<kSegFilterDepth>(s, blk, [&](int uu, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        split_out(v[uu], L0, H0, L1, H1);
        uint2 w = make_uint2(0, 0);
        if constexpr (MAPQ) {
            w = m[uu];
            reissue<HAS_NEXT ? 1 : 2>(uu, m, mcur, mnext, kSegRowBytes, load_mapq);
        }
        reissue<HAS_NEXT ? 1 : 2>(uu, v, cur, next, kSegRowVecs, load_vec<true>);
        const uint32_t p0 = pass4<MAPQ>(f, L0, H0, w.x);
        const uint32_t p1 = pass4<MAPQ>(f, L1, H1, w.y);
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
template <bool MAPQ>
__device__ __forceinline__ void count_piece_filter(uint32_t (&acc)[kInternal], uint32_t& cnt, const FilterArgs& f, const uint4 (&v)[kUnroll],
                                                   const uint2 (&m)[kUnroll], uint64_t w0, uint64_t b, uint64_t e, uint32_t lane)
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
        const uint32_t p0 = pass4<MAPQ>(f, L0, H0, m[r].x) & nibble_to_bit7(vb & 15u);
        const uint32_t p1 = pass4<MAPQ>(f, L1, H1, m[r].y) & nibble_to_bit7(vb >> 4);
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
// mq: the chunk's MAPQ column on the same grid (the byte of position q is mq[q]; not read when !MAPQ).  require & exclude == 0
// (the launcher's business), both below 2^16, min_mapq in 1..255 when MAPQ.  nunits = ceil(hi0 / 4096).  mode: bit 0 store form
// (out[] and selected[] zeroed in front), bit 1 superset.  selected may be nullptr.
template <bool MAPQ>
__global__ __launch_bounds__(kThreads) void flagstat_segments_filter(const uint4* __restrict__ a0, const uint8_t* __restrict__ mq,
                                                                     uint32_t require, uint32_t exclude, uint32_t min_mapq, uint64_t lo0,
                                                                     uint64_t hi0, uint64_t base, const uint64_t* __restrict__ off,
                                                                     uint64_t nseg, uint64_t* __restrict__ out,
                                                                     uint64_t* __restrict__ selected, int mode, uint64_t nunits,
                                                                     uint32_t min_units)
{
    __shared__ uint32_t red_all[kThreads / 64][24];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t waves = static_cast<uint64_t>(gridDim.x) * (kThreads / 64);
    const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * (kThreads / 64) + wave;
    const uint64_t u_begin = gw * nunits / waves, u_end = (gw + 1) * nunits / waves;
    const uint64_t p0 = u_begin * kSegWaveFlags > lo0 ? u_begin * kSegWaveFlags : lo0;  // this writer: grid positions [p0, E)
    const uint64_t E = u_end * kSegWaveFlags < hi0 ? u_end * kSegWaveFlags : hi0;
    if (p0 >= E) return;
    uint32_t* red = red_all[wave];

    SegWalk sw{off, nseg, base, hi0 - lo0, lo0, lane, 0, 0, 0};
    uint64_t s = sw.first_segment(p0);
    if (s >= nseg) return;
    sw.load_window(s);

    const FilterArgs f = filter_args_of(require, exclude, min_mapq);
    Lane<kSegFilterDepth> st;
    lane_init(st);
    uint32_t blk = 0;
    uint32_t cnt = 0;   // passing flags of this lane in segment s not yet emitted
    bool open = false;  // st and cnt hold counts of segment s not yet emitted
    uint64_t sb = 0, se = 0;
    uint32_t none = 0;  // no mask
    auto emit = [&](uint64_t seg, uint64_t b_, uint64_t e_) {
        seg_emit<true, false>(st, blk, cnt, none, none, red, out, selected, nullptr, seg, 0, (mode & 1) && b_ >= p0 && e_ <= E, mode, lane);
    };

    uint64_t u = p0 / kSegWaveFlags;
    while (s < nseg && u < u_end) {
        sw.bounds(s, sb, se);
        const uint64_t w0 = u * kSegWaveFlags;
        const uint64_t x = w0 > p0 ? w0 : p0;
        // (the order of these tests is seg_walk's in flagstat_segments_shared.h, for its reasons)
        if (sb >= E) break;
        if (se <= sb || se <= x) {  // empty (or, with malformed offsets, reversed or behind)
            ++s;
            continue;
        }
        if (sb >= w0 + kSegWaveFlags) {  // flags before the segment belong to none: skip whole units unread
            u = sb / kSegWaveFlags;
            continue;
        }
        const uint64_t seg_e = se < E ? se : E;
        if (sb <= w0 && w0 >= lo0) {
            const uint64_t k = (seg_e - w0) / kSegWaveFlags;  // whole units of segment s from here on
            if (k >= min_units && k > 0) {
                const uint4* p = a0 + u * kSegUnitVecs + lane;
                const uint8_t* pm = mq + (u * kSegUnitVecs + lane) * 8;
                uint4 v[kUnroll];
                uint2 m[kUnroll];
#pragma unroll
                for (int r = 0; r < kRollDistance; ++r) {
                    if constexpr (MAPQ) m[r] = load_mapq(pm + r * kSegRowBytes);
                    v[r] = load_vec<true>(p + r * kSegRowVecs);
                    __builtin_amdgcn_sched_barrier(0);
                }
                for (uint64_t i = 1; i < k; ++i) {
                    const uint4* pn = p + kSegUnitVecs;
                    const uint8_t* pmn = pm + kSegWaveFlags;
                    segf_step_and_count<MAPQ, true>(st, f, v, m, blk, cnt, p, pn, pm, pmn);
                    p = pn;
                    pm = pmn;
                }
                segf_step_and_count<MAPQ, false>(st, f, v, m, blk, cnt, p, nullptr, pm, nullptr);
                u += k;
                open = true;
                if (u * kSegWaveFlags >= se) {
                    emit(s, sb, se);
                    open = false;
                    ++s;
                }
                continue;
            }
        }
        // per-flag unit: its 8 rows and their MAPQ bytes loaded at once, then every segment piece in it
        uint4 v[kUnroll];
        uint2 m[kUnroll];
        const uint64_t j0 = u * kSegUnitVecs + lane;
        if (w0 >= lo0 && w0 + kSegWaveFlags <= hi0) {
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                v[r] = load_vec<true>(a0 + j0 + r * kSegRowVecs);
                if constexpr (MAPQ)
                    m[r] = load_mapq(mq + (j0 + r * kSegRowVecs) * 8);
                else
                    m[r] = make_uint2(0, 0);
            }
        } else {
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                v[r] = load_guarded(a0, j0 + r * kSegRowVecs, lo0, hi0);
                if constexpr (MAPQ)
                    m[r] = load_mapq_guarded(mq, j0 + r * kSegRowVecs, lo0, hi0);
                else
                    m[r] = make_uint2(0, 0);
            }
        }
        const uint64_t w1 = w0 + kSegWaveFlags;
        uint64_t xx = x;
        for (;;) {
            // s < nseg, sb < se, se > xx, sb < w1; the piece [b, e) lies inside [p0, E) and so inside [lo0, hi0)
            const uint64_t b = sb > xx ? sb : xx, e = se < w1 ? se : w1;
            count_piece_filter<MAPQ>(st.acc, cnt, f, v, m, w0, b, e, lane);
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
extern "C" hipError_t fsk_launch_segments_filter(const uint16_t* d_chunk, const uint8_t* d_mapq_chunk, uint64_t base, uint64_t m,
                                                 const uint64_t* d_offsets, uint64_t nseg, uint32_t require, uint32_t exclude,
                                                 uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected, int mode, uint32_t grid,
                                                 hipStream_t stream)
{
    if ((mode & ~3) || grid == 0 || require > 0xFFFFu || exclude > 0xFFFFu || min_mapq > 255u) return hipErrorInvalidValue;
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
    // a bit both required and excluded: no flag passes (samtools accepts the pair); the kernel's test assumes a disjoint pair
    if (m == 0 || (require & exclude)) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(addr & ~static_cast<uintptr_t>(15));
    const uint64_t hi0 = lo0 + m;
    uint32_t min_units = 0, blocks_per_cu = 0;
    fsk_segments_policy(&min_units, &blocks_per_cu);
    const dim3 gd(g), bd(fsk::kThreads);
    if (min_mapq) {
        // grid position q is element q - lo0 of the chunk: its byte is d_mapq_chunk[q - lo0]
        const uint8_t* mq = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_mapq_chunk) - lo0);
        hipLaunchKernelGGL((fsk::flagstat_segments_filter<true>), gd, bd, 0, stream, a0, mq, require, exclude, min_mapq, lo0, hi0, base,
                           d_offsets, nseg, d_out, d_selected, mode & 3, nunits, min_units);
    } else {
        hipLaunchKernelGGL((fsk::flagstat_segments_filter<false>), gd, bd, 0, stream, a0, static_cast<const uint8_t*>(nullptr), require,
                           exclude, 0u, lo0, hi0, base, d_offsets, nseg, d_out, d_selected, mode & 3, nunits, min_units);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The bodies of the three forms are fsseg's (flagstat_segments_shared.h): 33 words per segment, the rows, then the selected counts.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU (nseg > 0 from the NULL checks on)
int segf_args(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg, uint32_t require, uint32_t exclude,
              const uint8_t* mapq, uint32_t min_mapq, const void* out, int flags, const char* null_text)
{
    using namespace fsdrv;
    if (check_predicate(require, exclude, min_mapq) || check_flags(flags)) return -1;
    if (nseg == 0) return 0;
    return refused(fsseg::check_segments(offsets, out, nseg, null_text, fsseg::kMaxSegments / 2) || check_array_given(array, n) ||
                   check_mapq_given(mapq, n, min_mapq) || check_array_layout(array, n, 2));
}

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_u16_segments_filter(const uint16_t* d_array, uint64_t n, const uint64_t* d_offsets, uint64_t nseg,
                                             uint32_t require, uint32_t exclude, const uint8_t* d_mapq, uint32_t min_mapq,
                                             uint64_t* d_out, uint64_t* d_selected, int flags, void* stream)
{
    FS_ENTRY();
    int rc = segf_args(d_array, n, d_offsets, nseg, require, exclude, d_mapq, min_mapq, d_out, flags, fsseg::kNullDevice);
    if (rc || nseg == 0) return rc;
    const fsdrv::DeviceWord word{d_selected, "d_selected", "the counts are added with device atomics"};
    fsdrv::Inputs in = fsseg::offsets_input(d_offsets, nseg);
    in.add_columns(d_array, n, 2, nullptr, 0, 0, d_mapq, min_mapq);
    return fsseg::device_call(
        d_out, &word, 1, in.in, in.count, nseg, stream,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWaveFlags, grid); },
        [&](uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_filter(d_array, d_mapq, 0, n, d_offsets, nseg, require, exclude, min_mapq, d_out, d_selected,
                                                  flags & 3, grid, s));
            return 0;
        });
}

int FLAGSTATS_hip_device_u16_segments_filter_sync(const uint16_t* d_array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                                  uint32_t require, uint32_t exclude, const uint8_t* d_mapq, uint32_t min_mapq,
                                                  uint64_t* out, uint64_t* selected, int flags)
{
    FS_ENTRY();
    int rc = segf_args(d_array, n, offsets, nseg, require, exclude, d_mapq, min_mapq, out, flags, fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    fsdrv::Inputs in;
    in.add_columns(d_array, n, 2, nullptr, 0, 0, d_mapq, min_mapq);
    return fsseg::sync_call(
        in.in, in.count, n, offsets, nseg, 33,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWaveFlags, grid); },
        [&](fsseg::SegBuffers& buf, uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_filter(d_array, d_mapq, 0, n, buf.off, nseg, require, exclude, min_mapq, buf.cnt,
                                                  buf.cnt + nseg * 32, 1 | (flags & 2), grid, s));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_both(out, selected, got, nseg, flags); });
}

int FLAGSTATS_hip_u16_x64_segments_filter(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg, uint32_t require,
                                          uint32_t exclude, const uint8_t* mapq, uint32_t min_mapq, uint64_t* out, uint64_t* selected,
                                          int flags)
{
    FS_ENTRY();
    int rc = segf_args(array, n, offsets, nseg, require, exclude, mapq, min_mapq, out, flags, fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    // a chunk's slice of the MAPQ column rides in the same staging buffer, behind the flags.  An overlapping pair selects
    // nothing: nothing is moved.
    const int mode = flags & 2;
    return fsseg::host_call(
        n, offsets, nseg, 33, fsdrv::chunk_flags(), [&] { return (require & exclude) ? offsets[0] : offsets[nseg]; },
        [&](uint64_t cap) { return cap + ((min_mapq ? cap : 0) + 1) / 2; },
        [&](Engine& e, fsseg::SegBuffers& buf, int sl, uint64_t pos, uint64_t c, uint64_t cap, uint32_t grid) {
            uint8_t* d_mapq = reinterpret_cast<uint8_t*>(e.stage[sl] + cap);
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], array + pos, c * sizeof(uint16_t), hipMemcpyHostToDevice, e.stream[sl]));
            if (min_mapq) FS_HIP_TRY(hipMemcpyAsync(d_mapq, mapq + pos, c, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_segments_filter(e.stage[sl], d_mapq, pos, c, buf.off, nseg, require, exclude, min_mapq, buf.cnt,
                                                  buf.cnt + nseg * 32, mode, grid, e.stream[sl]));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_both(out, selected, got, nseg, flags); });
}

}  // extern "C"
