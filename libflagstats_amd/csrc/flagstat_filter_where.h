// flagstat_filter_where.h -- internal interface of the filtered flagstat under a selection (flagstat_filter_where.hip): counters
// of the elements of a uint16 FLAG array that pass samtools' view filter -f require / -F exclude / -q min_mapq AND that a bitmap
// or a byte mask selects, plus how many those are.  The C entry points built on it are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_FILTER_WHERE_H_
#define FLAGSTAT_FILTER_WHERE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// Counts {d_array[i] : pass(i) && sel(i), 0 <= i < n} exactly as K1 counts an array and adds the 32 slots to d_out32 (uint64,
// plain device memory) with relaxed agent-scope atomics; *d_selected (plain device memory, may be NULL: nothing reported) += the
// number of i with pass(i) && sel(i).  pass is fsk_launch_filter's predicate (flagstat_filter.h), sel is fsk_launch_where's
// selection (flagstat_where.h):
//   pass(i) = (d_array[i] & require) == require && (d_array[i] & exclude) == 0 && (min_mapq == 0 || d_mapq[i] >= min_mapq)
//   sel(i)  = sel_bits 1: bit (sel_offset + i) & 7 of byte (sel_offset + i) >> 3 of d_sel;  sel_bits 8: byte sel_offset + i != 0
// min_mapq == 0 reads no byte of d_mapq, which may then be NULL; otherwise exactly d_mapq[0 .. n) is read.  Only bytes of d_sel
// that hold the bit or byte of an element are read (fsk_where_geometry's geo[6 .. 8)).  The FLAG and the MAPQ of an element that
// is not selected are read but enter nothing.  One kernel, asynchronous on `stream`, no workspace.
//   mode bit 0: store form -- d_out32[0 .. 32) and *d_selected are zeroed first (one call when d_selected is d_out32 + 32, else
//               one each), so every slot is written
//   mode bit 1: superset slots (0 / 16 primary paired reads among those counted, 9 = their number minus slot 25)
// n == 0 and a pair with require & exclude != 0 (legal, passes nothing) launch nothing and read nothing (the store form still
// zeroes).  `grid` = workgroups (of 256 threads) at most.  Refused (hipErrorInvalidValue): everything fsk_launch_filter or
// fsk_launch_where refuses -- grid 0, other mode bits, require or exclude above 0xFFFF, min_mapq above 255, a NULL d_mapq with
// min_mapq > 0 and n > 0, other values of sel_bits, a NULL d_sel with n > 0, an odd array address, a sel_offset + n that is no
// index, and an (n, grid) pair at which a wave's uint32 totals could overflow.
hipError_t fsk_launch_filter_where(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                   uint32_t min_mapq, const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* d_out32,
                                   uint64_t* d_selected, int mode, uint32_t grid, hipStream_t stream);
}

#endif
