// flagstat_where.h -- internal interface of the selected-elements flagstat (flagstat_where.hip): counters of the elements of a
// uint16 FLAG array that a bitmap or a byte mask selects, plus how many it selects.  The C entry points built on it are declared
// in include/libflagstats_hip.h.
#ifndef FLAGSTAT_WHERE_H_
#define FLAGSTAT_WHERE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {
// Counts {d_array[i] : sel(i), 0 <= i < n} exactly as K1 counts an array and adds the 32 slots to d_out32 (uint64, plain device
// memory) with relaxed agent-scope atomics; *d_selected (plain device memory, may be NULL: nothing reported) += the number of i
// with sel(i).  sel_bits 1: sel(i) = bit (sel_offset + i) & 7 of byte (sel_offset + i) >> 3 of d_sel (LSB-first bitmap);
// sel_bits 8: sel(i) = byte sel_offset + i of d_sel is not zero.  Only bytes of d_sel that hold the bit or byte of an element are
// read.  One kernel, asynchronous on `stream`, no workspace.
//   mode bit 0: store form -- d_out32[0 .. 32) and *d_selected are zeroed first (hipMemsetAsync on `stream`: one call when
//               d_selected is d_out32 + 32, else one each), so every slot is written
//   mode bit 1: superset slots (0 / 16 primary paired reads among the selected, 9 = selected minus slot 25)
// n == 0 launches nothing (the store form still zeroes).  `grid` = workgroups (of 256 threads) at most; 0 is refused, as are
// other mode bits, other values of sel_bits, an odd array address and a sel_offset + n that is no index (hipErrorInvalidValue).
// Limit: a wave's totals are uint32, so every wave must own fewer than 2^32 elements; an (n, grid) pair that could break this is
// refused.  The public entries launch at least one workgroup per CU and cannot reach it.
hipError_t fsk_launch_where(const uint16_t* d_array, uint64_t n, const void* d_sel, uint64_t sel_offset, int sel_bits,
                            uint64_t* d_out32, uint64_t* d_selected, int mode, uint32_t grid, hipStream_t stream);
// The launcher's geometry without a launch (host arithmetic only; tests compare it with tests/where_oracle.py):
// geo[0..5] = lo, hi (flags on the 16-byte grid of the aligned-down base), nsteps, fast_begin, fast_end, workgroups launched;
// geo[6], geo[7] = the first byte of d_sel that may be read and one past the last, as offsets from d_sel.
// Refuses what fsk_launch_where refuses about (address, n, sel_offset, sel_bits, grid); n == 0 gives all zeros.
hipError_t fsk_where_geometry(uint64_t address, uint64_t n, uint64_t sel_offset, int sel_bits, uint32_t grid, uint64_t* geo);
}

namespace fsdrv {

// the bytes of the selection that hold an element's bit or byte: [first, first + bytes) from `sel` on (n > 0).  The device
// entries check the allocation from `sel` itself up to first + bytes: only `sel` is known to be device memory, and an offset at
// or past the allocation's end would otherwise name an address the runtime cannot vouch for
inline void where_extent(uint64_t n, uint64_t sel_offset, int sel_bits, uint64_t* first, uint64_t* bytes)
{
    *first = sel_bits == 1 ? sel_offset >> 3 : sel_offset;
    *bytes = (sel_bits == 1 ? ((sel_offset + n - 1) >> 3) + 1 : sel_offset + n) - *first;
}

}  // namespace fsdrv

#endif
