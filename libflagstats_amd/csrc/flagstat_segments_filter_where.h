// flagstat_segments_filter_where.h -- internal interface of the filtered and selected segmented flagstat
// (flagstat_segments_filter_where.hip): per CSR segment of one uint16 FLAG array, the counters of the elements that pass samtools'
// view filter -f require / -F exclude / -q min_mapq AND that a bitmap or a byte mask selects, and how many those are, in one
// launch.  The C entry points built on it are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_SEGMENTS_FILTER_WHERE_H_
#define FLAGSTAT_SEGMENTS_FILTER_WHERE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// fsk_launch_segments_filter (flagstat_segments_filter.h) and fsk_launch_segments_where (flagstat_segments_where.h) in one: the
// union of their contracts.  d_chunk holds the m flags [base, base + m) of the array (any 2-byte alignment), d_mapq_chunk their m
// MAPQ bytes (any alignment; not read, and may be NULL, when min_mapq == 0).  The selection is indexed by array element: element
// k of the chunk is bit (sel_bits == 1, LSB-first bitmap) or byte (sel_bits == 8, any non-zero byte selects) sel_offset + k of
// d_sel.  With
//   counted(j) = (flag[j] & require) == require && (flag[j] & exclude) == 0 && (min_mapq == 0 || mapq[j] >= min_mapq) && sel(j)
// the counted flags of the intersection of every segment i = [d_offsets[i], d_offsets[i+1]) (i < nseg, global flag indices) with
// the chunk are counted into d_out[i * 32 + slot] and their number is added to d_selected[i] (nseg uint64; may be NULL: nothing
// reported), both plain device memory, with relaxed agent-scope atomics; one kernel, asynchronous on `stream`, no workspace.
//   mode bit 0: store form -- d_out[0 .. nseg * 32) and d_selected[0 .. nseg) are zeroed first (fsk_zero_words on `stream`:
//               hipMemsetAsync, a kernel while capturing), so every slot of every segment is written; segments that lie inside one
//               wave's range are then stored with plain stores, rows and selected alike
//   mode bit 1: superset slots (0 / 16 primary paired reads among the counted, 9 = the piece's counted flags minus its fail-QC
//               reads)
// Bounds: every offset the kernel reads is clamped to [base, base + m] and a segment whose end lies before its begin is empty,
// so malformed offsets never make it read outside d_chunk[0 .. m) or d_mapq_chunk[0 .. m) or write outside
// d_out[0 .. nseg * 32) or d_selected[0 .. nseg).  Of d_sel only bytes that hold the bit or byte of an element of the chunk are
// read (geo[5 .. 7) of fsk_segments_where_geometry, whose geometry this launcher uses).  The FLAG and the MAPQ of an element that
// is not selected may be read; they enter nothing.  The kernel reads d_offsets[0 .. nseg] and nothing beyond.  nseg == 0 does
// nothing; m == 0 and a pair with require & exclude != 0 (legal, passes nothing) launch nothing and read nothing (the store form
// still zeroes).  The work split, the chain threshold and the workgroups per CU of the public entries are fsk_segments_policy's.
// sel_bits == 8 with min_mapq == 0 launches fsk::flagstat_segments_filter<true> with the mask as its MAPQ column and
// min_mapq = 1 (exactly "passes the FLAG test and the byte is not zero"); every other form launches
// fsk::flagstat_segments_filter_where.
// Refused (hipErrorInvalidValue, nothing queued): what either parent refuses -- other mode bits, grid == 0, require or exclude
// above 0xFFFF, min_mapq above 255, sel_bits other than 1 or 8, and with nseg > 0 a NULL d_out or d_offsets, a NULL d_chunk or
// d_sel with m > 0, a NULL d_mapq_chunk with min_mapq > 0 and m > 0, an odd array address, an m with m * 2 no size, a
// sel_offset + m that is no index, and an (m, grid) that leaves one wave 2^32 flags or more (a wave's totals are uint32).
hipError_t fsk_launch_segments_filter_where(const uint16_t* d_chunk, const uint8_t* d_mapq_chunk, const void* d_sel, uint64_t sel_offset,
                                            int sel_bits, uint64_t base, uint64_t m, const uint64_t* d_offsets, uint64_t nseg,
                                            uint32_t require, uint32_t exclude, uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected,
                                            int mode, uint32_t grid, hipStream_t stream);
}

#endif
