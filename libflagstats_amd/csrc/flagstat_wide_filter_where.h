// flagstat_wide_filter_where.h -- internal interface of the filtered and selected wide-input flagstat
// (flagstat_wide_filter_where.hip): counters of the elements of a FLAG array held as 4-byte or 8-byte little-endian integers that
// pass samtools' view filter -f require / -F exclude / -q min_mapq AND that a bitmap or a byte mask selects, how many those are,
// and the OR of every bit above bit 15 of the SELECTED elements, passing or not.  The C entry points built on it are declared in
// include/libflagstats_hip.h.
#ifndef FLAGSTAT_WIDE_FILTER_WHERE_H_
#define FLAGSTAT_WIDE_FILTER_WHERE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// With f(i) = the low 16 bits of element i of d_array (n elements of elem_bytes = 4 or 8, aligned to elem_bytes), pass(i) as in
// fsk_launch_wide_filter (flagstat_wide_filter.h) and sel(i) as in fsk_launch_wide_where (flagstat_wide_where.h: sel_bits 1 = bit
// sel_offset + i of an LSB-first bitmap, sel_bits 8 = byte sel_offset + i is not zero): counts {f(i) : pass(i) && sel(i)} exactly
// as K1 counts an array and adds the 32 slots to d_out32 (uint64, plain device memory) with relaxed agent-scope atomics;
// *d_selected += the number of i with pass(i) && sel(i); *d_high |= OR over the elements with sel(i), PASSING OR NOT, of
// (element & ~0xFFFF) taken as unsigned -- both parents' rules at once: the predicate sees the low 16 bits only and never
// restricts the mask, the selection always does (the value of a null slot is unspecified).  d_selected and d_high (plain device
// memory) may each be NULL: not reported.  min_mapq == 0 reads no byte of d_mapq, which may then be NULL; otherwise only
// d_mapq[0 .. n) is read (any alignment).  Only bytes of d_sel that hold the bit or byte of an element and only dwords of d_array
// that belong to an element are read; the FLAG or MAPQ of an element that is not selected may be read but enters nothing.  One
// kernel, asynchronous on `stream`, no workspace.
//   mode bit 0: store form -- d_out32[0 .. 32), *d_selected and *d_high are zeroed first (on `stream`: one call when d_selected
//               is d_out32 + 32 and d_high is d_out32 + 33, else one per pointer), so every slot is written
//   mode bit 1: superset slots (0 / 16 primary paired reads among the counted, 9 = their number minus slot 25)
// n == 0 launches nothing (the store form still zeroes).  A pair with require & exclude != 0 is legal and counts nothing: nothing
// is launched and NOTHING IS READ, so *d_high is 0 in the store form and untouched in the += form.  `grid` = workgroups (of 256
// threads) at most; 0 is refused, as are other mode bits, other widths, other values of sel_bits, a misaligned array, require or
// exclude above 0xFFFF, min_mapq above 255, a NULL d_sel with n > 0, a NULL d_mapq with min_mapq > 0 and n > 0 and a
// sel_offset + n that is no index (hipErrorInvalidValue).  The geometry is fsk_wide_where_geometry's (flagstat_wide_where.h: the
// step split, the selection bytes that may be read, step 0 of a funnelled bitmap launch through the guarded path), with its limit:
// a wave's totals are uint32, and an (n, grid) pair that could overflow them is refused.
hipError_t fsk_launch_wide_filter_where(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                        const uint8_t* d_mapq, uint32_t min_mapq, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                        uint64_t* d_out32, uint64_t* d_selected, uint64_t* d_high, int mode, uint32_t grid,
                                        hipStream_t stream);
}

#endif
