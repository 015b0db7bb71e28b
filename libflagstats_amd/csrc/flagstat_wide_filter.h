// flagstat_wide_filter.h -- internal interface of the filtered wide-input flagstat (flagstat_wide_filter.hip): counters of the
// elements of a FLAG array held as 4-byte or 8-byte little-endian integers that pass samtools' view filter -f require /
// -F exclude / -q min_mapq, how many pass, and the OR of every bit above bit 15 of every element.  The C entry points built on it
// are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_WIDE_FILTER_H_
#define FLAGSTAT_WIDE_FILTER_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// With f(i) = the low 16 bits of element i of d_array (n elements of elem_bytes = 4 or 8, aligned to elem_bytes) and
//   pass(i) = (f(i) & require) == require && (f(i) & exclude) == 0 && (min_mapq == 0 || d_mapq[i] >= min_mapq):
// counts {f(i) : pass(i)} exactly as K1 counts an array and adds the 32 slots to d_out32 (uint64, plain device memory) with
// relaxed agent-scope atomics; *d_selected += the number of i with pass(i); *d_high |= OR over ALL n elements, passing or not, of
// (element & ~0xFFFF) taken as unsigned -- the predicate sees the low 16 bits only, and the mask says whether the column is a
// FLAG column, not whether the selected reads are.  d_selected and d_high (plain device memory) may each be NULL: not reported.
// min_mapq == 0 reads no byte of d_mapq, which may then be NULL; otherwise exactly d_mapq[0 .. n) is read (any alignment).  One
// kernel, asynchronous on `stream`, no workspace.
//   mode bit 0: store form -- d_out32[0 .. 32), *d_selected and *d_high are zeroed first (hipMemsetAsync on `stream`: one call
//               when d_selected is d_out32 + 32 and d_high is d_out32 + 33, else one per pointer), so every slot is written
//   mode bit 1: superset slots (0 / 16 primary paired reads among those that pass, 9 = their number minus slot 25)
// n == 0 launches nothing (the store form still zeroes).  A pair with require & exclude != 0 is legal and passes nothing: nothing
// is launched and NO ELEMENT IS READ, so *d_high is 0 in the store form and untouched in the += form -- the mask of such a call
// says nothing about the column.  `grid` = workgroups (of 256 threads) at most; 0 is refused, as are other mode bits, other
// widths, a misaligned array, require or exclude above 0xFFFF, min_mapq above 255 and a NULL d_mapq with min_mapq > 0 and n > 0
// (hipErrorInvalidValue).  The geometry is fsk_wide_geometry's (flagstat_wide.h), with its limit: a wave's totals are uint32, and
// an (n, grid) pair that could overflow them is refused.
hipError_t fsk_launch_wide_filter(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                  const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* d_out32, uint64_t* d_selected, uint64_t* d_high,
                                  int mode, uint32_t grid, hipStream_t stream);
}

#endif
