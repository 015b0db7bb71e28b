// flagstat_segments_wide_where.h -- internal interface of the selected-elements segmented flagstat over 4-byte and 8-byte elements
// (flagstat_segments_wide_where.hip): per CSR segment of one int32 / int64 FLAG column, the 32 counters of the elements that a
// bitmap or a byte mask selects, how many it selects, and the OR of every bit above bit 15 of the segment's SELECTED elements, in
// one launch.  The C entry points built on it are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_SEGMENTS_WIDE_WHERE_H_
#define FLAGSTAT_SEGMENTS_WIDE_WHERE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// fsk_launch_segments_wide (flagstat_segments_wide.h) under fsk_launch_wide_where's selection (flagstat_wide_where.h).  d_chunk
// holds the m elements [base, base + m) of the array (elem_bytes = 4 or 8, aligned to elem_bytes).  The selection is indexed by
// array element: element k of the chunk is bit (sel_bits == 1, LSB-first bitmap) or byte (sel_bits == 8, any non-zero byte
// selects) sel_offset + k of d_sel, i.e. sel_offset is the selection index of the chunk's element 0.  With f(j) = the low 16 bits
// of element j, for every segment i = [d_offsets[i], d_offsets[i+1]) (i < nseg, global element indices) and its intersection
// with the chunk:
//   d_out[i * 32 + slot] += the counters of {f(j) : sel(j)}                               (relaxed agent-scope atomic adds)
//   d_selected[i]        += the number of j with sel(j)                                   (one atomic add, only if non-zero; may be NULL)
//   d_high[i]            |= OR of (element j & ~0xFFFF) over the SELECTED j of it ONLY    (one atomic OR, only if non-zero; may be NULL)
// all plain device memory.  One kernel, asynchronous on `stream`, no workspace.  An unselected element, an element that lies in
// no segment and whatever surrounds the chunk enter no counter, no count and no mask.
//   mode bit 0: store form -- d_out[0 .. nseg * 32), d_selected[0 .. nseg) and d_high[0 .. nseg) are zeroed first (fsk_zero_words
//               on `stream`: one call over nseg * 34 words when d_selected == d_out + nseg * 32 and d_high == d_selected + nseg,
//               else one each), so every slot, count and mask is written; segments that lie inside one wave's range are then
//               stored with plain stores
//   mode bit 1: superset slots (0 / 16 primary paired reads among the selected, 9 = the piece's selected count minus its
//               fail-QC reads)
// Bounds: every offset the kernel reads is clamped to [base, base + m] and a segment whose end lies before its begin is empty, so
// malformed offsets never make it read outside d_chunk[0 .. m) or write outside the three outputs.  Of d_sel only bytes that hold
// the bit or byte of an element of the chunk are read (the range fsk_segments_wide_where_geometry reports); of d_chunk only dwords
// of elements.  The kernel reads d_offsets[0 .. nseg] and nothing beyond.  nseg == 0 does nothing; m == 0 launches nothing (the
// store form still zeroes).  The chain threshold is fsk_segments_policy's min_units, in units of 8192 / elem_bytes elements.
// Refused (hipErrorInvalidValue, nothing queued): other widths, other mode bits, grid == 0, sel_bits other than 1 or 8, and with
// nseg > 0 a NULL d_out or d_offsets, a NULL d_chunk or d_sel with m > 0, a d_chunk not aligned to elem_bytes, an m with
// m * elem_bytes not a size, a sel_offset + m that is no index, and an (m, grid) that leaves one wave 2^32 elements or more (a
// wave's totals are uint32).
hipError_t fsk_launch_segments_wide_where(const void* d_chunk, int elem_bytes, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                          uint64_t base, uint64_t m, const uint64_t* d_offsets, uint64_t nseg, uint64_t* d_out,
                                          uint64_t* d_selected, uint64_t* d_high, int mode, uint32_t grid, hipStream_t stream);
// The launcher's geometry without a launch (host arithmetic only; tests compare it with tests/segments_wide_where_oracle.py):
//   geo[0 .. 3) = lo0 (the chunk's first element on the 16-byte grid of its aligned-down base, in elements), units of
//                 8192 / elem_bytes elements, workgroups
//   geo[3], geo[4] = what the kernel is handed of the selection: its base pointer minus d_sel (two's complement: it may be
//                    negative) and, for the bitmap, the shift: bit q + shift of that base belongs to grid position q (bytes: the
//                    byte of grid position q is base[q], shift 0)
//   geo[5] = 1 if the launch is funnelled (a bitmap with shift != 0: a lane loads two adjacent selection bytes, and grid unit 0
//            goes through the guarded loaders only), else 0
//   geo[6], geo[7] = the first byte of d_sel that may be read and one past the last, as offsets from d_sel
// Refuses what fsk_launch_segments_wide_where refuses about (address, m, elem_bytes, sel_offset, sel_bits, grid); m == 0 gives all
// zeros.
hipError_t fsk_segments_wide_where_geometry(uint64_t address, uint64_t m, int elem_bytes, uint64_t sel_offset, int sel_bits, uint32_t grid,
                                            uint64_t* geo);
}

#endif
