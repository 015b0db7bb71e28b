// flagstat_filter_rf.h -- internal interface of the filtered flagstat under samtools' whole view predicate on FLAG
// (flagstat_filter_rf.hip): -f require, -F exclude, --rf include_any, -G exclude_all and -q min_mapq over a uint16 FLAG array.
// The C entry points built on it are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_FILTER_RF_H_
#define FLAGSTAT_FILTER_RF_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// The predicate on FLAG, reduced exactly.  With
//   pass(flag) = (flag & require) == require && (flag & exclude) == 0 && (include_any == 0 || (flag & include_any) != 0)
//                && (exclude_all == 0 || (flag & exclude_all) != exclude_all)
// these rules are applied until nothing changes, and out[0 .. 4) = the reduced require, exclude, include_any, exclude_all, which
// pass exactly the flags the given four pass:
//   require & exclude != 0                  nothing passes
//   include_any touches require             it is satisfied: dropped
//               otherwise                   its exclude bits are removed; none left: nothing passes; one left: it moves to require
//   exclude_all touches exclude             it can never be all set: dropped
//               otherwise                   its require bits are removed; none left: nothing passes; one left: it moves to exclude
// Returns 0 when nothing passes (out is then all zero), 1 when the reduced include_any and exclude_all are both 0 (a plain
// require / exclude pair: fsk_launch_filter's predicate), 2 when a residue is left.  A residual include_any or exclude_all has at
// least two bits and shares none with the reduced require | exclude, so a result of 1 or 2 always passes some flag.  Host code, no
// GPU; any 32-bit masks are taken as they are.
int fsk_filter_rf_reduce(uint32_t require, uint32_t exclude, uint32_t include_any, uint32_t exclude_all, uint32_t out[4]);

// fsk_launch_filter (flagstat_filter.h) under the whole predicate: counts {d_array[i] : pass(d_array[i]) && (min_mapq == 0 ||
// d_mapq[i] >= min_mapq), 0 <= i < n} into d_out32 and adds their number to *d_selected, with that launcher's contract for
// everything else (mode bits, store-form memset, NULL d_mapq with min_mapq == 0, exactly d_mapq[0 .. n) read, one kernel,
// asynchronous on `stream`, no workspace, the limit on (n, grid)).  include_any == 0 and exclude_all == 0 switch those tests off.
// By fsk_filter_rf_reduce's answer:
//   0  nothing is launched or read (the store form still zeroes), as fsk_launch_filter does for require & exclude != 0
//   1  the launch is fsk_launch_filter's with the reduced pair: fsk::flagstat_count_filter
//   2  fsk::flagstat_count_filter_rf with the reduced four masks
// Refused (hipErrorInvalidValue) besides what fsk_launch_filter refuses: include_any or exclude_all above 0xFFFF.
hipError_t fsk_launch_filter_rf(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, uint32_t include_any,
                                uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* d_out32, uint64_t* d_selected,
                                int mode, uint32_t grid, hipStream_t stream);
}

#endif
