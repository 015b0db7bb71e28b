// flagstat_wide.h -- internal interface of the wide-input flagstat (flagstat_wide.hip): counters of a FLAG array held as 4-byte or
// 8-byte little-endian integers, plus the OR of every bit above bit 15.  The C entry points built on it are declared in
// include/libflagstats_hip.h.
#ifndef FLAGSTAT_WIDE_H_
#define FLAGSTAT_WIDE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// Counts the low 16 bits of each of the n elements of d_array (elem_bytes = 4 or 8, aligned to elem_bytes) exactly as K1 counts a
// uint16 and adds the 32 slots to d_out32 (uint64, plain device memory) with relaxed agent-scope atomics; *d_high (plain device
// memory, may be NULL: nothing reported) |= OR over all elements of (element & ~0xFFFF), taken as unsigned.  One kernel,
// asynchronous on `stream`, no workspace.
//   mode bit 0: store form -- d_out32[0 .. 32) and *d_high are zeroed first (hipMemsetAsync on `stream`: one call when d_high is
//               d_out32 + 32, else one each), so every slot is written
//   mode bit 1: superset slots (0 / 16 primary paired reads, 9 = n minus slot 25)
// n == 0 launches nothing (the store form still zeroes).  `grid` = workgroups (of 256 threads) at most; 0 is refused, as are
// other mode bits, other widths and a misaligned pointer (hipErrorInvalidValue).  Limit: a wave's totals are uint32, so every
// wave must own fewer than 2^32 elements; an (n, grid) pair that could break this is refused.  The public entries launch at
// least one workgroup per CU and cannot reach it.
hipError_t fsk_launch_wide(const void* d_array, uint64_t n, int elem_bytes, uint64_t* d_out32, uint64_t* d_high, int mode,
                           uint32_t grid, hipStream_t stream);
// The launcher's geometry without a launch (host arithmetic only; tests compare it with tests/steps_oracle.StepSplit):
// geo[0..5] = lo, hi (elements on the 16-byte grid of the aligned-down base), nsteps, fast_begin, fast_end, workgroups launched.
// Refuses what fsk_launch_wide refuses about (address, n, elem_bytes, grid); n == 0 gives all zeros.
hipError_t fsk_wide_geometry(uint64_t address, uint64_t n, int elem_bytes, uint32_t grid, uint64_t* geo);
}

#endif
