// flagstat_wide_where.h -- internal interface of the selected-elements wide-input flagstat (flagstat_wide_where.hip): counters of
// the elements of a FLAG array held as 4-byte or 8-byte little-endian integers that a bitmap or a byte mask selects, how many it
// selects, and the OR of every bit above bit 15 of the SELECTED elements.  The C entry points built on it are declared in
// include/libflagstats_hip.h.
#ifndef FLAGSTAT_WIDE_WHERE_H_
#define FLAGSTAT_WIDE_WHERE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// With f(i) = the low 16 bits of element i of d_array (n elements of elem_bytes = 4 or 8, aligned to elem_bytes) and sel(i) as in
// fsk_launch_where (flagstat_where.h: sel_bits 1 = bit sel_offset + i of an LSB-first bitmap, sel_bits 8 = byte sel_offset + i is
// not zero): counts {f(i) : sel(i)} exactly as K1 counts an array and adds the 32 slots to d_out32 (uint64, plain device memory)
// with relaxed agent-scope atomics; *d_selected += the number of i with sel(i); *d_high |= OR over the SELECTED elements only of
// (element & ~0xFFFF) taken as unsigned.  (The filtered entries' mask covers every element read, fsk_launch_wide_filter; this
// one does not on purpose: a selection is typically a validity bitmap, and the value of a null slot is unspecified.)  d_selected
// and d_high (plain device memory) may each be NULL: not reported.  Only bytes of d_sel that hold the bit or byte of an element
// and only dwords of d_array that belong to an element are read.  One kernel, asynchronous on `stream`, no workspace.
//   mode bit 0: store form -- d_out32[0 .. 32), *d_selected and *d_high are zeroed first (on `stream`: one call when d_selected
//               is d_out32 + 32 and d_high is d_out32 + 33, else one per pointer), so every slot is written
//   mode bit 1: superset slots (0 / 16 primary paired reads among the selected, 9 = selected minus slot 25)
// n == 0 launches nothing (the store form still zeroes).  `grid` = workgroups (of 256 threads) at most; 0 is refused, as are
// other mode bits, other widths, other values of sel_bits, a misaligned array and a sel_offset + n that is no index
// (hipErrorInvalidValue).  Limit: a wave's totals are uint32, and an (n, grid) pair that could overflow them is refused.
hipError_t fsk_launch_wide_where(const void* d_array, uint64_t n, int elem_bytes, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                 uint64_t* d_out32, uint64_t* d_selected, uint64_t* d_high, int mode, uint32_t grid, hipStream_t stream);
// The launcher's geometry without a launch (host arithmetic only; tests compare it with tests/wide_where_oracle.py):
// geo[0..5] = lo, hi (elements on the 16-byte grid of the aligned-down base), nsteps, fast_begin, fast_end, workgroups launched
// (the step split at W = elem_bytes; a bitmap launch whose bits do not start at a byte boundary of the grid runs step 0 through the
// guarded path even where the split calls it fast, see flagstat_wide_where.hip); geo[6], geo[7] = the first byte of d_sel that
// may be read and one past the last, as offsets from d_sel.  Refuses what fsk_launch_wide_where refuses about (address, n, elem_bytes, sel_offset, sel_bits, grid); n == 0
// gives all zeros.
hipError_t fsk_wide_where_geometry(uint64_t address, uint64_t n, int elem_bytes, uint64_t sel_offset, int sel_bits, uint32_t grid,
                                   uint64_t* geo);
}

#endif
