// flagstat_segments_wide_filter_where.hip -- segmented flagstat of a FLAG array held as 4-byte or 8-byte little-endian integers
// (int32 / int64 columns), read in place, under samtools' view filter AND a selection together: per CSR segment the 32 counters of
// {element[j] & 0xFFFF : pass(j) && sel(j)}, the number of such j, and the OR of element[j] & ~0xFFFF over the SELECTED elements of
// THAT segment only -- passing or not --, in one launch.  With f(j) = element[j] & 0xFFFF,
//   pass(j) = (f(j) & require) == require && (f(j) & exclude) == 0 && (min_mapq == 0 || mapq[j] >= min_mapq)
//   sel(j)  = bit (an LSB-first bitmap that may start at any bit) or byte (any non-zero byte selects) j of the selection
// The last cell of the grid {uint16, wide} x {whole array, per segment} x {no predicate, -f / -F / -q, mask, both}: it is
// flagstat_segments_wide_filter.hip with the selection as a third stream, or flagstat_segments_wide_where.hip with the predicate in
// front of the count.  The semantics are flagstat_wide_filter_where.hip's, per segment: the filter never restricts `high` (the
// predicate sees the low 16 bits only), the selection always does (a null slot's value is unspecified).  Garbage in an unselected
// slot, an element of a neighbouring segment or of a gap, and the bytes around the array enter no counter, no count and no mask.
//
// From both parents, as they are: the geometry (units of 8 KiB on the 16-byte grid of the aligned-down base, 2048 elements at
// W = 4, 1024 at W = 8, 8 rows of 64 lanes x 16 B; every wave of the grid a writer over a contiguous run of units), SegWalk,
// fsk_segments_policy and seg_emit<true, true>.  The walk is this kernel's own copy of seg_walk<UE> (flagstat_segments_shared.h), as
// both parents keep one and for their reason, registers; a change to the walk is made there and in the three copies;
// tests/test_segments_wide_filter_where_host.py holds this copy to flagstat_segments_wide_where.hip's rule by rule.
// From flagstat_segments_wide_filter.hip: the MAPQ column (`mq` is such that the byte of grid position q is mq[q]; one unaligned
// dword per vector at W = 4, one unaligned 16-bit load at W = 8; a template flag says whether it is read at all) and the two
// maskings of a piece.  From flagstat_segments_wide_where.hip: the selection's addressing -- which byte, which shift, which two
// bytes of a funnelled lane (its top comment has the derivation, not repeated here), the plain (cached) selection loads -- and the
// rule that GRID UNIT 0 OF A FUNNELLED LAUNCH IS LOADED THROUGH THE GUARDED LOADERS ONLY and is never chained (`guard0`): at
// EPV = 4 or 2 a lane of unit 0 whose bits do not straddle would read the selection byte in front of the first one that holds an
// element's bit.  The launcher's selection geometry is flagstat_segments_wide_where.h's geometry function, called, not restated.
//
// Two regimes, chosen per stretch by the parents' policy:
//   * chain regime (a run of at least `min_units` whole units inside one segment): the filtered wide step (wide_filter_step_with's,
//     flagstat_wide_filter_device.h) under the segmented per-wave stride, written out here because the selection enters it in two
//     places: a vector's MAPQ bytes and its selection word are re-issued with it; the unselected elements are zeroed in front of the
//     read-out (select_elements), so `high` sees selected elements only; and the selection's EPV bits or bytes are ANDed into the
//     pass word in front of the popcount and of the plane masks (counted_bits / counted_bytes of flagstat_filter_where_device.h),
//     because a zeroed element passes every predicate without `require` bits and an unselected one may pass any.  W = 8: the even
//     vector's selection is held until the odd one's arrives, like its MAPQ bytes.  Epochs of 255 units, flushed exactly when the
//     segment ends.  Nothing about the selection is carried from unit to unit except the pointers.
//   * per-piece regime: the unit's 8 rows, their MAPQ bytes and their selection are loaded once (guarded where the unit is not
//     wholly inside [lo0, hi0), and for unit 0 of a funnelled launch), the selection brought to EPV bits a row from bit 0 on.
//     Three maskings, which are not the same thing: the unselected elements are zeroed once per unit (the selection does not
//     depend on the piece), for `high`; mask_vec_wide zeroes the elements outside the piece, which keeps neighbours out of `high`
//     and out of the counters; and the pass word is ANDed with the piece's valid bits (valid_bits_wide) AND the selection bits,
//     both through one nibble_to_bit7, because a zeroed element passes every predicate without `require` bits.
// No selection or MAPQ byte is read that does not hold an element's bit or byte: the unguarded loaders run only on units every
// position of which is an element (and, funnelled, never on grid unit 0); the guarded ones touch element positions only.
//
// The byte form without -q is an instantiation of its own.  It cannot be routed through flagstat_segments_wide_filter<W, true>
// with the mask as the MAPQ column and min_mapq = 1, as the uint16 kernel routes its byte form: that kernel's `high` covers every
// element read, this one's the selected elements only.
//
// Emission (seg_emit<true, true>): lanes 0-31 of one instruction write the row (superset slot 9 from the counted number), lane 32
// selected[s], lane 33 high[s]: plain stores where the row is stored plainly, else relaxed agent-scope atomics (add, add, OR)
// issued only for non-zero values.  No LDS table, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/libflagstats_hip.h"
#include "flagstat_count_core.h"
#include "flagstat_derived_host.h"
#include "flagstat_engine.h"
#include "flagstat_filter_device.h"
#include "flagstat_filter_where_device.h"
#include "flagstat_segments.h"
#include "flagstat_segments_shared.h"
#include "flagstat_segments_wide.h"
#include "flagstat_segments_wide_device.h"
#include "flagstat_segments_wide_filter_where.h"
#include "flagstat_segments_wide_where.h"
#include "flagstat_where.h"
#include "flagstat_where_device.h"
#include "flagstat_wide_device.h"
#include "flagstat_wide_filter_device.h"
#include "flagstat_wide_where_device.h"

namespace fsk {

constexpr int kSegWideFilterWhereDepth = 8;   // chain depth as K1: epochs of 255 units

// One unit of the chain regime: the filtered wide step with the selection x[u] of vector u applied twice -- to the vector in
// front of its read-out, and to the group's pass word.  ROLL 1, 2: vector u's MAPQ bytes, selection and registers are re-issued
// for vector u + 6 of the same unit (`cur`) or u - 2 of the next (`next`, ROLL 1 only).
template <int W, bool MAPQ, int SEL_BITS, int ROLL, typename LoadSel>
__device__ __forceinline__ void segwfw_step_and_count(Lane<kSegWideFilterWhereDepth>& s, const FilterArgs& f, uint4 (&v)[kUnroll],
                                                      uint32_t (&m)[kUnroll], uint32_t (&x)[kUnroll], uint32_t& blk, uint32_t sh,
                                                      uint32_t& cnt, uint32_t& or_even, uint32_t& or_odd, LoadSel&& load_sel,
                                                      const uint4* __restrict__ cur, const uint4* __restrict__ next,
                                                      const uint8_t* __restrict__ mcur, const uint8_t* __restrict__ mnext,
                                                      const uint8_t* __restrict__ scur, const uint8_t* __restrict__ snext)
{
    constexpr int NIN = 32 / W;
    constexpr int EPV = 16 / W;
    constexpr int SS = kSegRowVecs * EPV / (SEL_BITS == 1 ? 8 : 1);   // selection bytes between a lane's consecutive vectors
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
            reissue<ROLL>(u, m, mcur, mnext, kSegRowVecs * EPV, load_mapq_wide<W>);
        }
        reissue<ROLL>(u, x, scur, snext, SS, load_sel);
        reissue<ROLL>(u, v, cur, next, kSegRowVecs, load_vec<true>);
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
    chain_push<0, kSegWideFilterWhereDepth>(s, blk, ct, cf, cs);
    end_step<kSegWideFilterWhereDepth>(s, blk);
}

// the EPV selection bits, from bit 0 on, of a vector's selection word as the unguarded loaders deliver it
template <int W, int SEL_BITS>
__device__ __forceinline__ uint32_t segwfw_selection_bits(uint32_t w, uint32_t sh)
{
    if constexpr (SEL_BITS == 1) {
        return __builtin_amdgcn_ubfe(w, sh, 16 / W);
    } else {
        uint32_t s;
        (void)bytes_mask(w, s);            // 0x01 per selected byte
        return (s * 0x01020408u) >> 24;    // bit 8 e -> bit 24 + e; the 16 partial products fall on 16 different bits
    }
}

// The elements of the piece that pass and are selected, out of the unit starting at grid position w0 (its 8 rows in v[], the
// unselected elements already zeroed; their MAPQ bytes in m[]), into the lane counters and the lane's count; the dwords of every
// selected element of the piece into the lane's mask accumulators.  counted: bit r * EPV + k says that element k of this lane's
// vector in row r lies in the piece and is selected.
template <int W, bool MAPQ>
__device__ __forceinline__ void count_piece_wide_filter_where(uint32_t (&acc)[kInternal], uint32_t& cnt, uint32_t& or_even, uint32_t& or_odd,
                                                              const FilterArgs& f, const uint4 (&v)[kUnroll], const uint32_t (&m)[kUnroll],
                                                              uint32_t counted, uint64_t w0, uint64_t b, uint64_t e, uint32_t lane)
{
    count_piece_wide_with<W>(acc, or_even, or_odd, v, w0, b, e, lane,
                             [&](int g, uint32_t& L0, uint32_t& H0, uint32_t& L1, uint32_t& H1) __attribute__((always_inline)) {
        // a count_planes call takes 8 elements of the lane: rows 2 g, 2 g + 1 (W = 4, 4 bits each) or 4 g .. 4 g + 3 (W = 8, 2 bits
        // each) -- in `counted` the 8 bits from bit 8 g on at either width, the first plane pair's in the low nibble
        const uint32_t n0 = (counted >> (8 * g)) & 15u, n1 = (counted >> (8 * g + 4)) & 15u;
        uint32_t q0, q1;   // the MAPQ bytes of the 4 elements of (L0, H0) and of (L1, H1)
        if constexpr (W == 4) {
            q0 = m[2 * g];
            q1 = m[2 * g + 1];
        } else {
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
// sel, shift: the chunk's selection on the same grid (flagstat_segments_wide_where.hip; FUNNEL: shift != 0; byte form: shift
// unused).  require & exclude == 0 (the launcher's business), both below 2^16, min_mapq in 1..255 when MAPQ.  nunits =
// ceil(hi0 / (8192 / W)).  mode: bit 0 store form (out[], selected[] and high[] zeroed in front), bit 1 superset.  selected and
// high may each be nullptr.
template <int W, bool MAPQ, int SEL_BITS, bool FUNNEL>
__global__ __launch_bounds__(kThreads) void flagstat_segments_wide_filter_where(const uint4* __restrict__ a0, const uint8_t* __restrict__ mq,
                                                                                const uint8_t* __restrict__ sel, uint32_t shift,
                                                                                uint32_t require, uint32_t exclude, uint32_t min_mapq,
                                                                                uint64_t lo0, uint64_t hi0, uint64_t base,
                                                                                const uint64_t* __restrict__ off, uint64_t nseg,
                                                                                uint64_t* __restrict__ out, uint64_t* __restrict__ selected,
                                                                                uint64_t* __restrict__ high, int mode, uint64_t nunits,
                                                                                uint32_t min_units)
{
    static_assert(W == 4 || W == 8, "4-byte or 8-byte elements");
    static_assert(SEL_BITS == 1 || (SEL_BITS == 8 && !FUNNEL), "a bitmap (at a byte boundary of the grid or not) or bytes");
    constexpr uint64_t UE = kSegWideUnitBytes / W;   // elements per unit
    constexpr int EPV = 16 / W;                       // elements, and MAPQ bytes, per vector
    constexpr uint64_t RE = 1024 / W;                 // elements per row
    constexpr int kRowMapq = kSegRowVecs * EPV;       // MAPQ bytes of a row
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
    // straddle -- the byte no unguarded load ever takes)
    const int32_t lane_sel = static_cast<int32_t>(SEL_BITS == 1 ? lane_bit >> 3 : lane_bit) + (FUNNEL ? static_cast<int32_t>(d) - 1 : 0);
    auto load_sel = [](const uint8_t* __restrict__ p) __attribute__((always_inline)) {
        // bitmap: plain loads, not non-temporal ones, as in flagstat_segments_wide_where.hip: the line has to stay for the next row
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

    const FilterArgs f = filter_args_of(require, exclude, min_mapq);
    Lane<kSegWideFilterWhereDepth> st;
    lane_init(st);
    uint32_t blk = 0;
    uint32_t cnt = 0;                   // counted elements of this lane in segment s not yet emitted
    uint32_t or_even = 0, or_odd = 0;   // dwords of segment s's selected elements, passing or not, not yet emitted
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
                    const uint8_t* pm = mq + (u * kSegUnitVecs + lane) * EPV;
                    const uint8_t* ps = sel + u * SU + lane_sel;
                    uint4 v[kUnroll];
                    uint32_t m[kUnroll], xs[kUnroll];
                    // the first kRollDistance vectors, each behind its MAPQ bytes and its selection; the rest is issued as they
                    // are consumed
#pragma unroll
                    for (int r = 0; r < kRollDistance; ++r) {
                        if constexpr (MAPQ) m[r] = load_mapq_wide<W>(pm + r * kRowMapq);
                        xs[r] = load_sel(ps + r * SS);
                        v[r] = load_vec<true>(p + r * kSegRowVecs);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    for (uint64_t i = 1; i < k; ++i) {
                        const uint4* pn = p + kSegUnitVecs;
                        const uint8_t* pmn = pm + UE;
                        const uint8_t* psn = ps + SU;
                        segwfw_step_and_count<W, MAPQ, SEL_BITS, 1>(st, f, v, m, xs, blk, sh, cnt, or_even, or_odd, load_sel, p, pn, pm, pmn,
                                                                    ps, psn);
                        p = pn;
                        pm = pmn;
                        ps = psn;
                    }
                    segwfw_step_and_count<W, MAPQ, SEL_BITS, 2>(st, f, v, m, xs, blk, sh, cnt, or_even, or_odd, load_sel, p, nullptr, pm,
                                                                nullptr, ps, nullptr);
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
        // per-piece unit: its 8 rows, their MAPQ bytes and their selection loaded at once, the selection as EPV bits a row from
        // bit 0 on in mp; the selection does not depend on the piece, so the unselected elements are zeroed once per unit
        uint4 v[kUnroll];
        uint32_t m[kUnroll];
        uint32_t mp = 0, unused = 0;
        const uint64_t j0 = u * kSegUnitVecs + lane;
        if (w0 >= lo0 && w0 + UE <= hi0 && !guard0) {
            const uint8_t* ps = sel + u * SU + lane_sel;
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                v[r] = load_vec<true>(a0 + j0 + r * kSegRowVecs);
                if constexpr (MAPQ)
                    m[r] = load_mapq_wide<W>(mq + (j0 + r * kSegRowVecs) * EPV);
                else
                    m[r] = 0;
                const uint32_t bits = segwfw_selection_bits<W, SEL_BITS>(load_sel(ps + r * SS), sh);
                select_elements<W, 1>(v[r], bits, 0u, unused);
                mp |= bits << (r * EPV);
            }
        } else {
#pragma unroll
            for (int r = 0; r < kUnroll; ++r) {
                v[r] = load_guarded_wide<W>(a0, j0 + r * kSegRowVecs, lo0, hi0);
                if constexpr (MAPQ)
                    m[r] = load_mapq_wide_guarded<W>(mq, j0 + r * kSegRowVecs, lo0, hi0);
                else
                    m[r] = 0;
                uint32_t bits;
                if constexpr (SEL_BITS == 1)
                    bits = load_bits_wide_guarded<W>(sel, shift, j0 + r * kSegRowVecs, lo0, hi0);
                else
                    bits = segwfw_selection_bits<W, 8>(load_mapq_wide_guarded<W>(sel, j0 + r * kSegRowVecs, lo0, hi0), 0u);
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
            // a selected element outside the piece, and an unselected one inside it, pass no predicate here
            count_piece_wide_filter_where<W, MAPQ>(st.acc, cnt, or_even, or_odd, f, v, m, mp & in_piece, w0, b, e, lane);
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

namespace {

// the selection forms of one (W, MAPQ): bytes, a bitmap at a byte boundary of the grid, a bitmap funnelled
template <int W, bool MAPQ, typename... Args>
void launch_form(int sel_bits, bool funnel, dim3 gd, hipStream_t stream, Args... args)
{
    const dim3 bd(fsk::kThreads);
    if (sel_bits == 8)
        hipLaunchKernelGGL((fsk::flagstat_segments_wide_filter_where<W, MAPQ, 8, false>), gd, bd, 0, stream, args...);
    else if (funnel)
        hipLaunchKernelGGL((fsk::flagstat_segments_wide_filter_where<W, MAPQ, 1, true>), gd, bd, 0, stream, args...);
    else
        hipLaunchKernelGGL((fsk::flagstat_segments_wide_filter_where<W, MAPQ, 1, false>), gd, bd, 0, stream, args...);
}

}  // namespace

extern "C" hipError_t fsk_launch_segments_wide_masked_filter(const void* d_chunk, int elem_bytes, const uint8_t* d_mapq_chunk,
                                                             const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t base, uint64_t m,
                                                             const uint64_t* d_offsets, uint64_t nseg, uint32_t require, uint32_t exclude,
                                                             uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected, uint64_t* d_high,
                                                             int mode, uint32_t grid, hipStream_t stream)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || (sel_bits != 1 && sel_bits != 8) || (mode & ~3) || grid == 0 || require > 0xFFFFu ||
        exclude > 0xFFFFu || min_mapq > 255u)
        return hipErrorInvalidValue;
    if (nseg == 0) return hipSuccess;
    if (d_out == nullptr || d_offsets == nullptr ||
        (m && (d_chunk == nullptr || d_sel == nullptr || (min_mapq && d_mapq_chunk == nullptr))))
        return hipErrorInvalidValue;
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
    // a bit both required and excluded: no element passes (samtools accepts the pair); the kernel's test assumes a disjoint pair.
    // Nothing is launched, so no element is read and the masks stay what the store form's zeroing or the caller left there.
    if (m == 0 || (require & exclude)) return hipSuccess;
    const uint4* a0 = reinterpret_cast<const uint4*>(addr & ~static_cast<uintptr_t>(15));
    const uint8_t* sel = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_sel) + geo[3]);
    const uint64_t lo0 = geo[0], hi0 = lo0 + m, nunits = geo[1];
    const uint32_t shift = static_cast<uint32_t>(geo[4]);
    // grid position q is element q - lo0 of the chunk: its MAPQ byte is d_mapq_chunk[q - lo0]
    const uint8_t* mq = min_mapq ? reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(d_mapq_chunk) - lo0) : nullptr;
    uint32_t min_units = 0, blocks_per_cu = 0;
    fsk_segments_policy(&min_units, &blocks_per_cu);
    const dim3 gd(static_cast<uint32_t>(geo[2]));
    const bool funnel = geo[5] != 0;
    const int md = mode & 3;
#define FSK_SWFW_LAUNCH(W_, Q_)                                                                                                          \
    launch_form<W_, Q_>(sel_bits, funnel, gd, stream, a0, mq, sel, shift, require, exclude, min_mapq, lo0, hi0, base, d_offsets, nseg, d_out, \
                        d_selected, d_high, md, nunits, min_units)
    if (elem_bytes == 4) {
        if (min_mapq)
            FSK_SWFW_LAUNCH(4, true);
        else
            FSK_SWFW_LAUNCH(4, false);
    } else {
        if (min_mapq)
            FSK_SWFW_LAUNCH(8, true);
        else
            FSK_SWFW_LAUNCH(8, false);
    }
#undef FSK_SWFW_LAUNCH
    return hipGetLastError();
}

// ------------------------------------------------------------------ C entry points (include/libflagstats_hip.h)
// The bodies of the three forms are fsseg's (flagstat_segments_shared.h): 34 words per segment, the rows, then the counts, then
// the masks.
using fsint::Engine;
using fsint::fail_text;

namespace {

// what every form refuses before it touches the GPU (nseg > 0 from the NULL checks on): the union of what the filtered and the
// selected wide segmented entries refuse, in their words
int segwfw_args(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg, uint32_t require, uint32_t exclude,
                const uint8_t* mapq, uint32_t min_mapq, const void* sel, uint64_t sel_offset, int sel_bits, const void* out, int flags,
                const char* null_text)
{
    using namespace fsdrv;
    if (check_elem_bytes(elem_bytes, "elem_bytes 2: 16-bit arrays go to the u16 segments_filter_where entries "
                                     "(FLAGSTATS_hip_u16_x64_segments_filter_where, FLAGSTATS_hip_device_u16_segments_filter_where)") ||
        check_predicate(require, exclude, min_mapq) || check_sel_bits(sel_bits) || check_flags(flags))
        return -1;
    if (nseg == 0) return 0;
    return refused(fsseg::check_segments(offsets, out, nseg, null_text, fsseg::kMaxSegments / 2) || check_array_given(array, n) ||
                   check_mapq_given(mapq, n, min_mapq) || check_sel_given(sel, n) || check_array_layout(array, n, elem_bytes) ||
                   check_sel_range(sel_offset, n));
}

}  // namespace

extern "C" {

int FLAGSTATS_hip_device_wide_segments_filter_where(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* d_offsets, uint64_t nseg,
                                                    uint32_t require, uint32_t exclude, const uint8_t* d_mapq, uint32_t min_mapq,
                                                    const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* d_out,
                                                    uint64_t* d_selected, uint64_t* d_high, int flags, void* stream)
{
    FS_ENTRY();
    int rc = segwfw_args(d_array, n, elem_bytes, d_offsets, nseg, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits, d_out, flags,
                         fsseg::kNullDevice);
    if (rc || nseg == 0) return rc;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const fsdrv::DeviceWord words[] = {{d_selected, "d_selected", "the counts are added with device atomics"},
                                       {d_high, "d_high", "the masks are ORed with device atomics"}};
    fsdrv::Inputs in = fsseg::offsets_input(d_offsets, nseg);
    in.add_columns(d_array, n, W, d_sel, sel_offset, sel_bits, d_mapq, min_mapq);
    return fsseg::device_call(
        d_out, words, 2, in.in, in.count, nseg, stream,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWideUnitBytes / W, grid); },
        [&](uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_wide_masked_filter(d_array, elem_bytes, d_mapq, d_sel, sel_offset, sel_bits, 0, n, d_offsets, nseg,
                                                              require, exclude, min_mapq, d_out, d_selected, d_high, flags & 3, grid, s));
            return 0;
        });
}

int FLAGSTATS_hip_device_wide_segments_filter_where_sync(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* offsets,
                                                         uint64_t nseg, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                                         uint32_t min_mapq, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                                         uint64_t* out, uint64_t* selected, uint64_t* high, int flags)
{
    FS_ENTRY();
    int rc = segwfw_args(d_array, n, elem_bytes, offsets, nseg, require, exclude, d_mapq, min_mapq, d_sel, sel_offset, sel_bits, out, flags,
                         fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    fsdrv::Inputs in;
    in.add_columns(d_array, n, W, d_sel, sel_offset, sel_bits, d_mapq, min_mapq);
    return fsseg::sync_call(
        in.in, in.count, n, offsets, nseg, 34,
        [&](uint32_t grid) { return fsseg::fits(d_array, n, fsk::kSegWideUnitBytes / W, grid); },
        [&](fsseg::SegBuffers& buf, uint32_t grid, hipStream_t s) {
            FS_HIP_TRY(fsk_launch_segments_wide_masked_filter(d_array, elem_bytes, d_mapq, d_sel, sel_offset, sel_bits, 0, n, buf.off, nseg,
                                                              require, exclude, min_mapq, buf.cnt, buf.cnt + nseg * 32, buf.cnt + nseg * 33,
                                                              1 | (flags & 2), grid, s));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_all(out, selected, high, got, nseg, flags); });
}

int FLAGSTATS_hip_wide_x64_segments_filter_where(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg,
                                                 uint32_t require, uint32_t exclude, const uint8_t* mapq, uint32_t min_mapq, const void* sel,
                                                 uint64_t sel_offset, int sel_bits, uint64_t* out, uint64_t* selected, uint64_t* high,
                                                 int flags)
{
    FS_ENTRY();
    int rc = segwfw_args(array, n, elem_bytes, offsets, nseg, require, exclude, mapq, min_mapq, sel, sel_offset, sel_bits, out, flags,
                         fsseg::kNullHost);
    if (rc || nseg == 0) return rc;
    // the elements cross the bus as they are, in chunks of "chunk_flags" * 2 bytes (the wide host entries'); a chunk's slices of the
    // MAPQ column and of the selection ride in the same staging buffer, behind its elements: the column's first, then the
    // selection's -- a bitmap slice from the byte that holds the chunk's first bit (the launch then starts (sel_offset + pos) & 7
    // bits into it); every chunk's launch adds to the same device rows and counts and ORs into the same device masks.  An
    // overlapping pair counts nothing and reads no element: nothing is moved.
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const int mode = flags & 2;
    const uint8_t* src = static_cast<const uint8_t*>(array);
    const uint8_t* sel_src = static_cast<const uint8_t*>(sel);
    auto mapq_slot = [&](uint64_t cap) { return min_mapq ? (cap + 1) / 2 : 0; };   // a chunk's MAPQ slice, in uint16
    return fsseg::host_call(
        n, offsets, nseg, 34, fsdrv::chunk_flags() * 2 / W, [&] { return (require & exclude) ? offsets[0] : offsets[nseg]; },
        [&](uint64_t cap) { return cap * W / 2 + mapq_slot(cap) + ((sel_bits == 1 ? (cap + 7) / 8 + 1 : cap) + 1) / 2; },
        [&](Engine& e, fsseg::SegBuffers& buf, int sl, uint64_t pos, uint64_t c, uint64_t cap, uint32_t grid) {
            uint64_t sel_first, sel_len;
            where_extent(c, sel_offset + pos, sel_bits, &sel_first, &sel_len);
            uint8_t* d_mapq = reinterpret_cast<uint8_t*>(e.stage[sl]) + cap * W;
            uint8_t* d_sel = d_mapq + mapq_slot(cap) * 2;
            FS_HIP_TRY(hipMemcpyAsync(e.stage[sl], src + pos * W, c * W, hipMemcpyHostToDevice, e.stream[sl]));
            if (min_mapq) FS_HIP_TRY(hipMemcpyAsync(d_mapq, mapq + pos, c, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(hipMemcpyAsync(d_sel, sel_src + sel_first, sel_len, hipMemcpyHostToDevice, e.stream[sl]));
            FS_HIP_TRY(fsk_launch_segments_wide_masked_filter(e.stage[sl], elem_bytes, d_mapq, d_sel, sel_bits == 1 ? (sel_offset + pos) & 7 : 0,
                                                              sel_bits, pos, c, buf.off, nseg, require, exclude, min_mapq, buf.cnt,
                                                              buf.cnt + nseg * 32, buf.cnt + nseg * 33, mode, grid, e.stream[sl]));
            return 0;
        },
        [&](const fsseg::HostRows& got) { fsseg::apply_all(out, selected, high, got, nseg, flags); });
}

}  // extern "C"
