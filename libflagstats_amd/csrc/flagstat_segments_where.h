// flagstat_segments_where.h -- internal interface of the selected-elements segmented flagstat (flagstat_segments_where.hip): per
// CSR segment of one uint16 FLAG array, the counters of the elements that a bitmap or a byte mask selects and how many it
// selects, in one launch.  The C entry points built on it are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_SEGMENTS_WHERE_H_
#define FLAGSTAT_SEGMENTS_WHERE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// fsk_launch_segments (flagstat_segments.h) under fsk_launch_where's selection (flagstat_where.h).  d_chunk holds the m flags
// [base, base + m) of the array (any 2-byte alignment).  The selection is indexed by array element: element k of the chunk is
// bit (sel_bits == 1, LSB-first bitmap) or byte (sel_bits == 8, any non-zero byte selects) sel_offset + k of d_sel, i.e.
// sel_offset is the selection index of the chunk's element 0.  For every segment i = [d_offsets[i], d_offsets[i+1]) (i < nseg,
// global flag indices) the selected flags of its intersection with the chunk are counted into d_out[i * 32 + slot] and their
// number is added to d_selected[i] (nseg uint64; may be NULL: nothing reported), both plain device memory, with relaxed
// agent-scope atomics; one kernel, asynchronous on `stream`, no workspace.
//   mode bit 0: store form -- d_out[0 .. nseg * 32) and d_selected[0 .. nseg) are zeroed first (fsk_zero_words on `stream`:
//               hipMemsetAsync, a kernel while capturing), so every slot of every segment is written; segments that lie inside one
//               wave's range are then stored with plain stores, rows and selected alike
//   mode bit 1: superset slots (0 / 16 primary paired reads among the selected, 9 = the piece's selected flags minus its
//               fail-QC reads)
// Bounds: every offset the kernel reads is clamped to [base, base + m] and a segment whose end lies before its begin is empty,
// so malformed offsets never make it read outside d_chunk[0 .. m) or write outside d_out[0 .. nseg * 32) or
// d_selected[0 .. nseg).  Of d_sel only bytes that hold the bit or byte of an element of the chunk are read (the range
// fsk_segments_where_geometry reports).  The kernel reads d_offsets[0 .. nseg] and nothing beyond.  nseg == 0 and m == 0 launch
// nothing (the store form still zeroes).  The work split, the chain threshold and the workgroups per CU of the public entries
// are fsk_segments_policy's.  sel_bits == 8 launches fsk::flagstat_segments_filter<true> with the mask as its MAPQ column
// (require = exclude = 0, min_mapq = 1: exactly "any non-zero byte"); sel_bits == 1 launches fsk::flagstat_segments_where.
// Refused (hipErrorInvalidValue, nothing queued): other mode bits, grid == 0, sel_bits other than 1 or 8, and with nseg > 0 a
// NULL d_out or d_offsets, a NULL d_chunk or d_sel with m > 0, an odd array address, an m with m * 2 no size, a sel_offset + m
// that is no index, and an (m, grid) that leaves one wave 2^32 flags or more (a wave's totals are uint32).
hipError_t fsk_launch_segments_where(const uint16_t* d_chunk, const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t base,
                                     uint64_t m, const uint64_t* d_offsets, uint64_t nseg, uint64_t* d_out, uint64_t* d_selected,
                                     int mode, uint32_t grid, hipStream_t stream);
// The launcher's geometry without a launch (host arithmetic only; tests compare it with tests/segments_where_oracle.py):
//   geo[0 .. 3) = lo0 (the chunk's first flag on the 16-byte grid of its aligned-down base), units of 4,096 flags, workgroups
//   geo[3], geo[4] = what the kernel is handed of the selection: its base pointer minus d_sel (two's complement: it may be -1)
//                    and, for the bitmap, the bit of byte j of that base at which the 8 bits of grid vector j start (bytes: the
//                    byte of grid position q is base[q], shift 0)
//   geo[5], geo[6] = the first byte of d_sel that may be read and one past the last, as offsets from d_sel
// Refuses what fsk_launch_segments_where refuses about (address, m, sel_offset, sel_bits, grid); m == 0 gives all zeros.
hipError_t fsk_segments_where_geometry(uint64_t address, uint64_t m, uint64_t sel_offset, int sel_bits, uint32_t grid, uint64_t* geo);
}

#endif
