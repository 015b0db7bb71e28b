// flagstat_segments_filter_rf.h -- internal interface of the filtered segmented flagstat under samtools' whole view predicate on
// FLAG (flagstat_segments_filter_rf.hip): per CSR segment of one uint16 FLAG array, the counters of the flags that pass
// -f require / -F exclude / --rf include_any / -G exclude_all / -q min_mapq and how many pass, in one launch.  The C entry points
// built on it are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_SEGMENTS_FILTER_RF_H_
#define FLAGSTAT_SEGMENTS_FILTER_RF_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// fsk_launch_segments_filter (flagstat_segments_filter.h) under the whole predicate: with pass() the predicate on FLAG stated at
// the reduction's declaration in flagstat_filter_rf.h, for every segment i = [d_offsets[i], d_offsets[i+1]) the flags j of its
// intersection with the chunk with pass(flag[j]) && (min_mapq == 0 || mapq[j] >= min_mapq) are counted into d_out[i * 32 + slot]
// and their number is added to d_selected[i] -- with that launcher's contract for everything else (d_chunk / d_mapq_chunk / base /
// m, mode bits, the store form's zeroing, NULL d_selected, NULL d_mapq_chunk with min_mapq == 0, the clamping of malformed offsets,
// nseg == 0 and m == 0, one kernel, asynchronous on `stream`, no workspace, fsk_segments_policy, the limit on (m, grid)).
// include_any == 0 and exclude_all == 0 switch those tests off.
// By the answer of that reduction, which the launcher calls first:
//   0  nothing is launched and NO ELEMENT, MAPQ BYTE OR OFFSET IS READ (the store form still zeroes d_out[0 .. nseg * 32) and
//      d_selected[0 .. nseg); the += form leaves both as they are), as fsk_launch_segments_filter does for require & exclude != 0
//   1  the launch is fsk_launch_segments_filter's with the reduced pair: fsk::flagstat_segments_filter
//   2  fsk::flagstat_segments_filter_rf with the reduced four masks
// Refused (hipErrorInvalidValue) besides what fsk_launch_segments_filter refuses: include_any or exclude_all above 0xFFFF.
hipError_t fsk_launch_segments_filter_rf(const uint16_t* d_chunk, const uint8_t* d_mapq_chunk, uint64_t base, uint64_t m,
                                         const uint64_t* d_offsets, uint64_t nseg, uint32_t require, uint32_t exclude,
                                         uint32_t include_any, uint32_t exclude_all, uint32_t min_mapq, uint64_t* d_out,
                                         uint64_t* d_selected, int mode, uint32_t grid, hipStream_t stream);
}

#endif
