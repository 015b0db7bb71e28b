// flagstat_segments_wide.h -- internal interface of the segmented flagstat over 4-byte and 8-byte elements
// (flagstat_segments_wide.hip): per CSR segment of one int32 / int64 FLAG column, the 32 counters of the elements' low 16 bits and
// the OR of every bit above bit 15, in one launch.  The C entry points built on it are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_SEGMENTS_WIDE_H_
#define FLAGSTAT_SEGMENTS_WIDE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsk {

constexpr int kSegWideUnitBytes = 8192;   // a wave's unit of work, as flagstat_segments': 8 rows of 64 lanes x 16 B = 8192 / W elements

}  // namespace fsk

extern "C" {
// fsk_launch_segments (flagstat_segments.h) over the elements fsk_launch_wide (flagstat_wide.h) reads.  d_chunk holds the m
// elements [base, base + m) of the array (elem_bytes = 4 or 8, aligned to elem_bytes).  For every segment i = [d_offsets[i],
// d_offsets[i+1]) (i < nseg, global element indices) the low 16 bits of the elements of its intersection with the chunk are
// counted into d_out[i * 32 + slot] with relaxed agent-scope atomic adds, and the OR of their (element & ~0xFFFF), taken as
// unsigned, goes into d_high[i] (nseg uint64; may be NULL: nothing reported) with a relaxed agent-scope atomic OR, issued only
// for a non-zero value; both plain device memory.  One kernel, asynchronous on `stream`, no workspace.  Elements that lie in no
// segment enter no counter and no mask.
//   mode bit 0: store form -- d_out[0 .. nseg * 32) and d_high[0 .. nseg) are zeroed first (fsk_zero_words on `stream`: one call
//               when d_high is d_out + nseg * 32, else one each), so every slot of every segment and every mask is written;
//               segments that lie inside one wave's range are then stored with plain stores, rows and masks alike
//   mode bit 1: superset slots (0 / 16 primary paired reads, 9 = the piece's length minus its fail-QC reads)
// Bounds: every offset the kernel reads is clamped to [base, base + m] and a segment whose end lies before its begin is empty, so
// malformed offsets never make it read outside d_chunk[0 .. m) or write outside d_out[0 .. nseg * 32) or d_high[0 .. nseg); only
// their counters and masks are undefined.  The kernel reads d_offsets[0 .. nseg] and nothing beyond.  nseg == 0 does nothing;
// m == 0 launches nothing (the store form still zeroes).  The chain threshold is fsk_segments_policy's min_units, in units of
// 8192 / elem_bytes elements.
// Refused (hipErrorInvalidValue, nothing queued): other widths, other mode bits, grid == 0, and with nseg > 0 a NULL d_out or
// d_offsets, a NULL d_chunk with m > 0, a pointer not aligned to elem_bytes, and an (m, grid) that leaves one wave 2^32 elements
// or more (a wave's totals are uint32).
hipError_t fsk_launch_segments_wide(const void* d_chunk, int elem_bytes, uint64_t base, uint64_t m, const uint64_t* d_offsets,
                                    uint64_t nseg, uint64_t* d_out, uint64_t* d_high, int mode, uint32_t grid, hipStream_t stream);
}

#endif
