// flagstat_segments_wide_filter_where.h -- internal interface of the segmented flagstat over 4-byte and 8-byte elements under
// samtools' filter and a selection together (flagstat_segments_wide_filter_where.hip): per CSR segment of one int32 / int64 FLAG
// column, the 32 counters of the elements whose low 16 bits pass -f / -F / -q AND that a bitmap or a byte mask selects, how many
// those are, and the OR of every bit above bit 15 of the segment's SELECTED elements ONLY, passing or not, in one launch.  The C
// entry points built on it are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_SEGMENTS_WIDE_FILTER_WHERE_H_
#define FLAGSTAT_SEGMENTS_WIDE_FILTER_WHERE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// The launcher of flagstat_segments_wide_filter.h with the selection of the launcher of flagstat_segments_wide_where.h beside the
// predicate (its name says "masked filter" and not "filter_where" so that no launcher's name is the beginning of another's).
// d_chunk holds the m elements [base, base + m) of the array (elem_bytes = 4 or 8, aligned to elem_bytes), d_mapq_chunk their m
// MAPQ bytes (any alignment; not read and may be NULL when min_mapq == 0).  The selection is indexed by array element: element k
// of the chunk is bit (sel_bits == 1, LSB-first bitmap) or byte (sel_bits == 8, any non-zero byte selects) sel_offset + k of d_sel.
// With f(j) = the low 16 bits of element j and
//   pass(j) = (f(j) & require) == require && (f(j) & exclude) == 0 && (min_mapq == 0 || mapq[j] >= min_mapq),
// for every segment i = [d_offsets[i], d_offsets[i+1]) (i < nseg, global element indices) and its intersection with the chunk:
//   d_out[i * 32 + slot] += the counters of {f(j) : pass(j) && sel(j)}                    (relaxed agent-scope atomic adds)
//   d_selected[i]        += the number of j with pass(j) && sel(j)                        (one atomic add, only if non-zero; may be NULL)
//   d_high[i]            |= OR of (element j & ~0xFFFF) over the SELECTED j of it ONLY,
//                           passing or not                                                (one atomic OR, only if non-zero; may be NULL)
// all plain device memory.  One kernel, asynchronous on `stream`, no workspace.  An unselected element, an element that lies in
// no segment and whatever surrounds the chunk enter no counter, no count and no mask.
//   mode bit 0: store form -- d_out[0 .. nseg * 32), d_selected[0 .. nseg) and d_high[0 .. nseg) are zeroed first (fsk_zero_words
//               on `stream`: one call over nseg * 34 words when d_selected == d_out + nseg * 32 and d_high == d_selected + nseg,
//               else one each), so every slot, count and mask is written; segments that lie inside one wave's range are then
//               stored with plain stores
//   mode bit 1: superset slots (0 / 16 primary paired reads among the counted, 9 = the piece's counted number minus its fail-QC
//               reads)
// require & exclude != 0 counts nothing: after the zeroing of the store form nothing is launched and nothing is read, so the masks
// are then 0 in the store form and untouched otherwise.  min_mapq == 0 selects the kernels that read no MAPQ byte.
// Bounds: every offset the kernel reads is clamped to [base, base + m] and a segment whose end lies before its begin is empty, so
// malformed offsets never make it read outside d_chunk[0 .. m) or d_mapq_chunk[0 .. m), or write outside the three outputs.  Of
// d_sel only bytes that hold the bit or byte of an element of the chunk are read (the range the geometry function of
// flagstat_segments_wide_where.h reports: this launcher calls it); of d_chunk only dwords of elements.  The kernel reads
// d_offsets[0 .. nseg] and nothing beyond.  nseg == 0 does nothing; m == 0 launches nothing (the store form still zeroes).  The
// chain threshold is fsk_segments_policy's min_units, in units of 8192 / elem_bytes elements.
// Refused (hipErrorInvalidValue, nothing queued): other widths, other mode bits, grid == 0, sel_bits other than 1 or 8, require or
// exclude above 0xFFFF, min_mapq above 255, and with nseg > 0 a NULL d_out or d_offsets, a NULL d_chunk or d_sel with m > 0, a
// NULL d_mapq_chunk with min_mapq > 0 and m > 0, a d_chunk not aligned to elem_bytes, an m with m * elem_bytes not a size, a
// sel_offset + m that is no index, and an (m, grid) that leaves one wave 2^32 elements or more (a wave's totals are uint32).
hipError_t fsk_launch_segments_wide_masked_filter(const void* d_chunk, int elem_bytes, const uint8_t* d_mapq_chunk, const void* d_sel,
                                                  uint64_t sel_offset, int sel_bits, uint64_t base, uint64_t m, const uint64_t* d_offsets,
                                                  uint64_t nseg, uint32_t require, uint32_t exclude, uint32_t min_mapq, uint64_t* d_out,
                                                  uint64_t* d_selected, uint64_t* d_high, int mode, uint32_t grid, hipStream_t stream);
}

#endif
