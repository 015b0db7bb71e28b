// flagstat_wide_filter_rf.h -- internal interface of the filtered wide-input flagstat under samtools' whole view predicate on FLAG
// (flagstat_wide_filter_rf.hip): -f require, -F exclude, --rf include_any, -G exclude_all and -q min_mapq over a FLAG array held
// as 4-byte or 8-byte little-endian integers, read in place.  The C entry points built on it are declared in
// include/libflagstats_hip.h.
#ifndef FLAGSTAT_WIDE_FILTER_RF_H_
#define FLAGSTAT_WIDE_FILTER_RF_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// fsk_launch_wide_filter (flagstat_wide_filter.h) under the whole predicate: with f(i) = the low 16 bits of element i and pass()
// the predicate on FLAG stated at the reduction's declaration in flagstat_filter_rf.h, counts {f(i) : pass(f(i)) && (min_mapq == 0 ||
// d_mapq[i] >= min_mapq), 0 <= i < n} into d_out32, adds their number to *d_selected and ORs (element & ~0xFFFF) of ALL n
// elements, passing or not, into *d_high -- with that launcher's contract for everything else (mode bits, store-form memset, NULL
// d_selected / d_high, NULL d_mapq with min_mapq == 0, exactly d_mapq[0 .. n) read, one kernel, asynchronous on `stream`, no
// workspace, fsk_wide_geometry's limit on (n, grid)).  include_any == 0 and exclude_all == 0 switch those tests off.
// By the answer of that reduction, which the launcher calls first:
//   0  nothing is launched and NO ELEMENT IS READ (the store form still zeroes all three; the += form leaves all three as they
//      are), as fsk_launch_wide_filter does for require & exclude != 0: *d_high of such a call says nothing about the column
//   1  the launch is fsk_launch_wide_filter's with the reduced pair: fsk::flagstat_count_wide_filter
//   2  fsk::flagstat_count_wide_filter_rf with the reduced four masks
// Refused (hipErrorInvalidValue) besides what fsk_launch_wide_filter refuses: include_any or exclude_all above 0xFFFF.
hipError_t fsk_launch_wide_filter_rf(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                     uint32_t include_any, uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq,
                                     uint64_t* d_out32, uint64_t* d_selected, uint64_t* d_high, int mode, uint32_t grid,
                                     hipStream_t stream);
}

#endif
