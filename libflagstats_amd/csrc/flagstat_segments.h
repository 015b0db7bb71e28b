// flagstat_segments.h -- internal interface of the segmented flagstat (flagstat_segments.hip): counters for many CSR segments
// of one uint16 FLAG array in one launch.  The C entry points built on it are declared in include/libflagstats_hip.h.
#ifndef FLAGSTAT_SEGMENTS_H_
#define FLAGSTAT_SEGMENTS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fsk {

constexpr int kSegWaveFlags = 4096;   // a wave's unit of work: 8 rows of 512 flags (64 lanes x 16 B), 8 KiB contiguous

}  // namespace fsk

extern "C" {
// Counts the intersection of every segment i = [d_offsets[i], d_offsets[i+1]) (i < nseg, global flag indices) with the global
// flag range [base, base + m), whose m flags d_chunk holds (any 2-byte alignment), and adds it to d_out[i * 32 + slot]
// (uint64, plain device memory) with relaxed agent-scope atomics; asynchronous on `stream`.
//   mode bit 0: store form -- d_out[0 .. nseg * 32) is zeroed first (fsk_zero_words on `stream`: one hipMemsetAsync, a kernel while capturing), so every slot of every
//               segment is written; segments that lie inside one wave's range are then stored with plain stores
//   mode bit 1: superset slots (0 / 16 primary paired reads, 9 = the piece's length minus its fail-QC reads)
// Bounds: every offset the kernel reads is clamped to [base, base + m] and a segment whose end lies before its begin is
// empty, so malformed offsets never make it read outside d_chunk[0 .. m) or write outside d_out[0 .. nseg * 32); only their
// counters are undefined.  The kernel reads d_offsets[0 .. nseg] and nothing beyond.  `grid` = workgroups (of 256 threads)
// at most; 0 is refused.  Limit: a wave's totals are uint32, so every wave must own fewer than 2^32 flags, i.e. m < 2^32 * 4 *
// (workgroups launched); the public entries launch >= 4 waves per CU and cannot reach it, direct callers with a small grid can.
hipError_t fsk_launch_segments(const uint16_t* d_chunk, uint64_t base, uint64_t m, const uint64_t* d_offsets, uint64_t nseg,
                               uint64_t* d_out, int mode, uint32_t grid, hipStream_t stream);
// workgroups per CU of the segmented kernel and the shortest run of whole wave units (4096 flags) inside one segment that
// goes through K1's carry-save chain instead of the per-flag counters (measurement: tests/perf/segments_sweep.py)
void fsk_segments_policy(uint32_t* min_units, uint32_t* blocks_per_cu);
void fsk_set_segments_policy(uint32_t min_units, uint32_t blocks_per_cu);
}

#endif
