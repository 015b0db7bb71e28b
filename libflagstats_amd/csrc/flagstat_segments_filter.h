// flagstat_segments_filter.h -- internal interface of the filtered segmented flagstat (flagstat_segments_filter.hip): per CSR
// segment of one uint16 FLAG array, the counters of the flags that pass samtools' view filter -f require / -F exclude /
// -q min_mapq and how many pass, in one launch.  The C entry points built on it are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_SEGMENTS_FILTER_H_
#define FLAGSTAT_SEGMENTS_FILTER_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// fsk_launch_segments (flagstat_segments.h) under fsk_launch_filter's predicate (flagstat_filter.h).  d_chunk holds the m flags
// [base, base + m) of the array (any 2-byte alignment), d_mapq_chunk their m MAPQ bytes (any alignment; not read and may be NULL
// when min_mapq == 0).  For every segment i = [d_offsets[i], d_offsets[i+1]) (i < nseg, global flag indices) the flags j of its
// intersection with the chunk that pass,
//   pass(j) = (flag[j] & require) == require && (flag[j] & exclude) == 0 && (min_mapq == 0 || mapq[j] >= min_mapq),
// are counted into d_out[i * 32 + slot] and their number is added to d_selected[i] (nseg uint64; may be NULL: nothing
// reported), both plain device memory, with relaxed agent-scope atomics; one kernel, asynchronous on `stream`, no workspace.
//   mode bit 0: store form -- d_out[0 .. nseg * 32) and d_selected[0 .. nseg) are zeroed first (fsk_zero_words on `stream`: hipMemsetAsync, a kernel while capturing), so
//               every slot of every segment is written; segments that lie inside one wave's range are then stored with plain
//               stores, rows and selected alike
//   mode bit 1: superset slots (0 / 16 primary paired reads among those that pass, 9 = the piece's passing flags minus its
//               fail-QC reads)
// Bounds: every offset the kernel reads is clamped to [base, base + m] and a segment whose end lies before its begin is empty,
// so malformed offsets never make it read outside d_chunk[0 .. m) or d_mapq_chunk[0 .. m) or write outside d_out[0 .. nseg * 32)
// or d_selected[0 .. nseg); only their counters are undefined.  The kernel reads d_offsets[0 .. nseg] and nothing beyond.
// nseg == 0, m == 0 and a pair with require & exclude != 0 (legal, passes nothing) launch nothing (the store form still
// zeroes).  The work split, the chain threshold and the workgroups per CU of the public entries are fsk_segments_policy's.
// Refused (hipErrorInvalidValue, nothing queued): other mode bits, grid == 0, require or exclude above 0xFFFF, min_mapq above
// 255, and with nseg > 0 a NULL d_out or d_offsets, a NULL d_chunk with m > 0, a NULL d_mapq_chunk with min_mapq > 0 and m > 0, an
// odd array address, and an (m, grid) that leaves one wave 2^32 flags or more (a wave's totals are uint32).
hipError_t fsk_launch_segments_filter(const uint16_t* d_chunk, const uint8_t* d_mapq_chunk, uint64_t base, uint64_t m,
                                      const uint64_t* d_offsets, uint64_t nseg, uint32_t require, uint32_t exclude, uint32_t min_mapq,
                                      uint64_t* d_out, uint64_t* d_selected, int mode, uint32_t grid, hipStream_t stream);
}

#endif
