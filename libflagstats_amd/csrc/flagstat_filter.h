// flagstat_filter.h -- internal interface of the filtered flagstat (flagstat_filter.hip): counters of the elements of a uint16
// FLAG array that pass samtools' view filter -f require / -F exclude / -q min_mapq, plus how many pass.  The C entry points built
// on it are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_FILTER_H_
#define FLAGSTAT_FILTER_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// Counts {d_array[i] : pass(i), 0 <= i < n} exactly as K1 counts an array and adds the 32 slots to d_out32 (uint64, plain device
// memory) with relaxed agent-scope atomics; *d_selected (plain device memory, may be NULL: nothing reported) += the number of i
// with pass(i), where
//   pass(i) = (d_array[i] & require) == require && (d_array[i] & exclude) == 0 && (min_mapq == 0 || d_mapq[i] >= min_mapq).
// min_mapq == 0 reads no byte of d_mapq, which may then be NULL; otherwise exactly d_mapq[0 .. n) is read.  One kernel,
// asynchronous on `stream`, no workspace.
//   mode bit 0: store form -- d_out32[0 .. 32) and *d_selected are zeroed first (hipMemsetAsync on `stream`: one call when
//               d_selected is d_out32 + 32, else one each), so every slot is written
//   mode bit 1: superset slots (0 / 16 primary paired reads among those that pass, 9 = their number minus slot 25)
// n == 0 and a pair with require & exclude != 0 (legal, passes nothing) launch nothing (the store form still zeroes).  `grid` =
// workgroups (of 256 threads) at most; 0 is refused, as are other mode bits, require or exclude above 0xFFFF, min_mapq above 255,
// a NULL d_mapq with min_mapq > 0 and n > 0 and an odd array address (hipErrorInvalidValue).
// Limit: a wave's totals are uint32, so every wave must own fewer than 2^32 elements; an (n, grid) pair that could break this is
// refused (fsk_where_geometry's rule, flagstat_where.h).  The public entries launch at least one workgroup per CU.
hipError_t fsk_launch_filter(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                             uint32_t min_mapq, uint64_t* d_out32, uint64_t* d_selected, int mode, uint32_t grid, hipStream_t stream);
}

#endif
