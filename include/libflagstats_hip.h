/*
 * libflagstats_hip.h -- C ABI of libflagstats_hip.so, the MI355X (gfx950) engine behind libflagstats' flagstat entry points.
 * Plain C: pointers and sizes, no HIP or torch types (streams travel as void*).  Every symbol below is exported by
 * libflagstats_amd/libflagstats_hip.so (tests/test_host_logic.py checks that).  Measurement entries (read probes, timing
 * helpers, the clock probe, the GPU decoder called directly) and the full knob reference: libflagstats_hip_probe.h.
 */
#ifndef LIBFLAGSTATS_HIP_H_
#define LIBFLAGSTATS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ================= the drop-in: same names, argument meaning and return as the reference =================
 *
 * Contract (all entry points of this library): counters follow the reference's FLAGSTAT_scalar exactly
 * (libflagstats.h:118-142, :170-176): 32 slots, [0..15] pass-QC, [16..31] fail-QC, slot index = FLAGSTAT_*_OFF
 * (libflagstats.h:69-112); the 19 live slots are {2,6,7,8,10,11,12,13,14} and {18,22..30}; the other slots are never
 * written.  Counters are ACCUMULATED (+=), never zeroed by the callee (`++f[...]`; python/libflagstats.pyx:19 zeroes in
 * the caller).  There is NO CPU fallback: if the GPU path cannot run the call fails loudly -- a message on stderr and a
 * non-zero return; the three reference-shaped entry points (FLAGSTATS_u16, FLAGSTAT_hip, STORM_pospopcnt_u16), whose
 * reference callers ignore the return value (python/libflagstats.pyx:22, benchmark/flagstats.cpp:329), abort() after the
 * message instead of handing back silently-zero counters (knob "on_error" / FLAGSTATS_HIP_ON_ERROR=return restores the
 * plain non-zero return).  Any thread may call; the caller's current HIP device is restored before returning. */

/* replaces: typedef at libflagstats.h:2970 */
typedef int (*FLAGSTATS_func)(const uint16_t*, uint32_t, uint32_t*);

/* replaces: `static uint64_t FLAGSTATS_u16(const uint16_t* array, uint32_t n_len, uint32_t* flags)` libflagstats.h:3024-3070
 * (callers: python/libflagstats.pyx:22).  `array` is a HOST pointer (any 2-byte alignment); flags[32] += counters.
 * Returns 0 like the reference; non-zero only if the GPU path failed. */
uint64_t FLAGSTATS_u16(const uint16_t* array, uint32_t n_len, uint32_t* flags);

/* replaces: `static FLAGSTATS_func FLAGSTATS_get_function(uint32_t n_len)` libflagstats.h:2976-3022 (callers:
 * benchmark/flagstats.cpp:328,450,665).  One kernel family, no host kernels: returns &FLAGSTAT_hip for every n; the
 * length-aware rule (:2999-3021) stays in the reference's dispatcher, which INTEGRATION.md section B extends with this
 * library as its first branch (n >= FLAGSTATS_HIP_MIN_LEN). */
FLAGSTATS_func FLAGSTATS_get_function(uint32_t n_len);

/* the kernel itself, shaped like every FLAGSTAT_<impl> of the reference (FLAGSTAT_avx512 libflagstats.h:1644,
 * FLAGSTAT_scalar :170): host pointer in, flags[32] += counters, returns 0 on success. */
int FLAGSTAT_hip(const uint16_t* array, uint32_t len, uint32_t* flags);

/* replaces: `static int STORM_pospopcnt_u16(const uint16_t* data, size_t len, uint32_t* out)` python/libalgebra.h:3496-3551
 * (SURVEY section 8 f4): out[16] is ZEROED first (:3497), then out[j] = number of words with bit j set.  HOST pointer. */
int STORM_pospopcnt_u16(const uint16_t* data, size_t len, uint32_t* out);

/* ================= extensions the reference's uint32 ABI cannot express ================= */

/* 64-bit length, 64-bit counters, HOST pointer: out[32] += counters.  Streams the array through two device buffers (the
 * H2D copy of chunk k+1 overlaps the kernel on chunk k; truly asynchronous when `array` is page-locked, e.g. from
 * FLAGSTATS_hip_host_alloc; large pageable arrays are copied into page-locked chunks by worker threads). */
int FLAGSTATS_u16_x64(const uint16_t* array, uint64_t n, uint64_t* out);

/* DEVICE-resident array (any 2-byte alignment), DEVICE counters: d_out[32] (uint64, device memory) += counters,
 * asynchronously on `stream` (a hipStream_t passed as void*; NULL = HIP's null stream).  One kernel launch; the adds are
 * atomic, so launches on several streams may share d_out.  d_array may also be page-locked host memory: it is then read in
 * place over PCIe, with no staging copy.
 * Streams and HIP graphs: every entry that takes a `stream` (this one, _store, _superset, device_pospopcnt_u16, the
 * all-reduce forms) keeps one small workspace per caller stream -- the 64 most recently used streams of a device have one; a
 * 65th stream takes the least recently used one's (after a device-wide wait), and raising the knob "blocks_per_cu" replaces a
 * stream's workspace at its next call.  Plain launches never notice.  A launch CAPTURED into a graph holds its stream's
 * workspace pointer: the graph stays valid while its stream stays among the 64 most recently used and "blocks_per_cu" is not
 * raised; after either, replaying it touches freed memory -- capture it again instead.
 * Capture and replay are tested (tests/test_gpu_graphs.py, torch.cuda.graph in both capture error modes) for this entry, _store,
 * _superset, device_pospopcnt_u16, device_u16_segments, _where, _filter, _segments_filter, device_wide and device_wide_filter
 * (tests/test_gpu_segments_wide.py: device_wide_segments; tests/test_gpu_segments_where.py: device_u16_segments_where),
 * and for the torch layers on top of them: one call or all of them in one graph, after one plain call on the device (the first
 * call creates the device's engine, which is no stream work).  A captured launch freezes its pointers, n, its grid and the form
 * the knobs chose at capture time (epilogue form, the segments policy); it reads arrays, selections, MAPQ bytes and device
 * offsets at replay time, so a replay counts what the buffers hold then.  The store forms' zeroes are part of the graph (while
 * the stream is capturing they come from a small kernel, not a memset node: memset nodes were seen to write stale bytes when
 * replayed on ROCm 7.0).  Replay-stream contract: a captured launch of the entries with a workspace uses the workspace of
 * the stream it was captured on, without a lock -- replay the graph on that stream, or order every replay against that stream's
 * other work (and against other graphs captured on it); two of them running at once corrupt each other's counters.
 * NOT tested under capture: the all-reduce forms, the sessions, a graph replayed after its stream's workspace was evicted or
 * "blocks_per_cu" raised (see above), and graphs running concurrently over one captured workspace. */
int FLAGSTATS_hip_device_u16(const uint16_t* d_array, uint64_t n, uint64_t* d_out, void* stream);
/* same, but d_out[32] = counters (all 32 slots written, never-written slots as 0): one query per call with no zeroing
 * launch in front; used by the multi-GPU step before its all-reduce. */
int FLAGSTATS_hip_device_u16_store(const uint16_t* d_array, uint64_t n, uint64_t* d_out, void* stream);
/* DEVICE-resident array, HOST counters: out[32] += counters; synchronous. */
int FLAGSTATS_hip_device_u16_sync(const uint16_t* d_array, uint64_t n, uint64_t* out);

/* Superset forms: the same 19 counters PLUS, counted by the same kernel,
 *   slot 0 / slot 16  primary paired reads, pass-QC / fail-QC  = samtools' n_pair_all[w] (benchmark/flagstats.cpp:58)
 *   slot 9            pass-QC reads = n - slot 25   (the reference's SIMD kernels' "QC adjust", libflagstats.h:1843)
 * -- what the reference's SIMD kernels leave in those slots for their SIMD-covered prefix, here for every flag.
 * With them the whole samtools flagstat report (benchmark/flagstats.cpp:577-588) follows from the 32 slots. */
int FLAGSTATS_u16_x64_superset(const uint16_t* array, uint64_t n, uint64_t* out);                          /* host array */
int FLAGSTATS_hip_device_u16_superset(const uint16_t* d_array, uint64_t n, uint64_t* d_out, void* stream); /* async */
int FLAGSTATS_hip_device_u16_superset_sync(const uint16_t* d_array, uint64_t n, uint64_t* out);

/* ================= segmented flagstat: one counter row per segment, many segments in one launch =================
 * Segment i (i < nseg) is [offsets[i], offsets[i+1]) of the array (CSR offsets, nseg + 1 of them, uint64); its counters go to
 * out[i * 32 + slot], every row with the slot contract above (and with the superset flag, slots 0 / 16 and slot 9 = the
 * segment's length minus its slot 25, as the superset forms below).  Offsets must be non-decreasing with offsets[nseg] <= n;
 * flags before offsets[0] or after offsets[nseg] are ignored; empty segments are allowed; nseg == 0 does nothing and succeeds.
 * `flags`: bit 0 = store (out = counters: all 32 slots of every row written, never-written slots and empty segments as 0)
 * instead of +=, bit 1 = superset.
 * DEVICE offsets are not checked for order (that would need a synchronisation): every offset the kernel reads is clamped to
 * [0, n] and a segment whose end lies before its begin is empty, so malformed device offsets never read outside the array or
 * write outside d_out[nseg][32] -- only their counters are undefined.  The kernel reads d_offsets[0..nseg] only.
 * HOST offsets are validated first: decreasing offsets, offsets[nseg] > n, NULL pointers with nseg > 0 and an nseg whose
 * nseg * 256 bytes of device counters cannot be allocated fail (non-zero, message), and `out` is left untouched. */
/* DEVICE array, DEVICE offsets[nseg+1] (uint64), DEVICE out[nseg][32] (uint64); asynchronous on `stream` (one kernel; the store
 * form puts one memset in front of it).  The adds are atomic: launches on several streams may share d_out in the += form. */
int FLAGSTATS_hip_device_u16_segments(const uint16_t* d_array, uint64_t n, const uint64_t* d_offsets, uint64_t nseg,
                                      uint64_t* d_out, int flags, void* stream);
/* DEVICE array, HOST offsets, HOST out[nseg][32]; synchronous */
int FLAGSTATS_hip_device_u16_segments_sync(const uint16_t* d_array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                           uint64_t* out, int flags);
/* HOST array, HOST offsets, HOST out[nseg][32]; synchronous.  Only [offsets[0], offsets[nseg]) crosses the bus, in the engine's
 * chunks (knob "chunk_flags"); a segment that spans chunks is summed on the device. */
int FLAGSTATS_hip_u16_x64_segments(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                   uint64_t* out, int flags);

/* ================= wide input: a FLAG column held as 4-byte or 8-byte integers, counted in place =================
 * numpy's default integer, a pandas / CSV column and torch's natural integer tensors are int64 or int32, Arrow / Parquet FLAG
 * columns int32.  These entries read such an array as it is (little-endian elements of `elem_bytes` = 4 or 8 bytes, signed or
 * unsigned alike) instead of asking for a uint16 copy: the LOW 16 BITS of every element are counted exactly as the entries above
 * count a uint16 -- the same 32 slots, the same scalar-exact rule -- and, in the same pass over the array,
 *   high = OR over all elements of (element & ~0xFFFF), taken as unsigned
 * is reported: high == 0 means every element was a valid 16-bit FLAG; a negative element sets bit 31 (elem_bytes 4) or bit 63
 * (elem_bytes 8); any other bit names a value of 65,536 or more (a wrong column, a parse error).  The mask is exact and
 * deterministic.  The counters are always those of the truncated values (as FLAGSTATS_text_to_u16 documents for text input); it is
 * the caller who decides what a non-zero mask means.
 * `flags`: bit 0 = store (out = counters, all 32 slots written; high = mask) instead of out += counters, high |= mask;
 * bit 1 = superset (slots 0 / 16 and slot 9 = n minus slot 25, as the superset forms above).  `high` / `d_high` may be NULL:
 * nothing is reported.  n == 0 succeeds and touches nothing (the store form writes zeros).
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, out and high untouched, nothing launched): elem_bytes other than 4 or
 * 8 (2: use the u16 entries), an array pointer not aligned to elem_bytes, flag bits other than 0 and 1, a NULL array with
 * n > 0; for the device form also a d_out or d_high that is not plain device memory, pointers on different devices, a stream
 * of another device and an allocation shorter than n * elem_bytes (d_out: 256, d_high: 8) bytes from the pointer on. */
/* DEVICE array, DEVICE d_out[32] and d_high[1] (uint64); asynchronous on `stream`: ONE kernel (the store form puts one memset
 * per pointer in front of it; one in all when d_high == d_out + 32).  No per-stream workspace is kept, so a captured launch
 * holds no pointer of the library's (the caveat of FLAGSTATS_hip_device_u16) and may be replayed on any stream.  Capture into a
 * graph is tested for both widths and both layouts of d_high (see FLAGSTATS_hip_device_u16); the entry queries its pointers
 * (hipPointerGetAttributes, hipMemGetAddressRange: neither disturbs a capture) and creates the device's engine on a first call, so
 * make one plain call before capturing.  Adds and ORs are atomic: launches on several streams may share d_out and d_high in
 * the += form. */
int FLAGSTATS_hip_device_wide(const void* d_array, uint64_t n, int elem_bytes, uint64_t* d_out, uint64_t* d_high, int flags,
                              void* stream);
/* DEVICE array, HOST out[32] and high[1]; synchronous */
int FLAGSTATS_hip_device_wide_sync(const void* d_array, uint64_t n, int elem_bytes, uint64_t* out, uint64_t* high, int flags);
/* HOST array, HOST out[32] and high[1]; synchronous.  The array crosses the bus as it is (n * elem_bytes bytes) in the engine's
 * chunks (knob "chunk_flags": chunk_flags * 2 bytes each); counters and mask are summed / ORed on the device. */
int FLAGSTATS_hip_wide_x64(const void* array, uint64_t n, int elem_bytes, uint64_t* out, uint64_t* high, int flags);

/* ================= selected elements: flagstat under a bitmap or a byte mask =================
 * The table for the reads with MAPQ >= 30, for one read group or contig, for the non-null rows of an Arrow column: instead of
 * compacting the column first (values[mask]: a pass over column and mask, a copy, a pass over the copy) these entries read the
 * uint16 array and its selection once, in one kernel.  The 32 counters are FLAGSTAT_scalar's over the subsequence
 * {array[i] : sel(i), 0 <= i < n}; `selected` is the number of i with sel(i).  Two encodings of sel, chosen by `sel_bits`:
 *   sel_bits == 1: an LSB-first bitmap (Arrow's validity layout, numpy.packbits(m, bitorder="little")): element i is bit
 *                  (sel_offset + i) & 7 of byte (sel_offset + i) >> 3 of `sel`; sel_offset is any uint64 (an Arrow slice's offset)
 *   sel_bits == 8: one byte per element (numpy bool, torch.bool): element i is byte sel_offset + i, any non-zero byte selects
 * Only bytes of `sel` that hold the bit or byte of an element are read.
 * `flags`: bit 0 = store (out = counters, all 32 slots written; selected = count) instead of out += counters, selected += count;
 * bit 1 = superset (slots 0 / 16 = primary paired reads among the selected, slot 9 = selected minus slot 25).  `selected` /
 * `d_selected` may be NULL: nothing is reported.  n == 0 succeeds and touches nothing (the store form writes zeros); `sel` may
 * be NULL then.
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, out and selected untouched, nothing launched): sel_bits other than 1
 * or 8, an odd array pointer, flag bits other than 0 and 1, a NULL array or selection with n > 0, a sel_offset + n that is no
 * index; for the device forms also a d_out or d_selected that is not plain device memory, pointers on different devices, a
 * stream of another device and an allocation shorter than the call needs (d_array: n * 2 bytes, d_sel: the bytes that hold the
 * n bits or bytes, d_out: 256, d_selected: 8). */
/* DEVICE array and selection, DEVICE d_out[32] and d_selected[1] (uint64); asynchronous on `stream`: ONE kernel (the store form
 * puts one memset per pointer in front of it; one in all when d_selected == d_out + 32), no workspace.  Adds are atomic: launches
 * on several streams may share d_out and d_selected in the += form. */
int FLAGSTATS_hip_device_u16_where(const uint16_t* d_array, uint64_t n, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                   uint64_t* d_out, uint64_t* d_selected, int flags, void* stream);
/* DEVICE array and selection, HOST out[32] and selected[1]; synchronous */
int FLAGSTATS_hip_device_u16_where_sync(const uint16_t* d_array, uint64_t n, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                        uint64_t* out, uint64_t* selected, int flags);
/* HOST array and selection, HOST out[32] and selected[1]; synchronous.  Array and selection cross the bus in the engine's chunks
 * (knob "chunk_flags"), each chunk's slice of the selection with its flags; the counters are summed on the device. */
int FLAGSTATS_hip_u16_x64_where(const uint16_t* array, uint64_t n, const void* sel, uint64_t sel_offset, int sel_bits,
                                uint64_t* out, uint64_t* selected, int flags);

/* ================= filtered: flagstat under samtools' view filter -f / -F / -q =================
 * `samtools view -f require -F exclude -q min_mapq | samtools flagstat` without the mask array that the `where` entries would
 * need: the predicate is a function of the FLAG value and of one uint8 column next to it, and is applied inside the count.
 *   pass(i) = (array[i] & require) == require && (array[i] & exclude) == 0 && (min_mapq == 0 || mapq[i] >= min_mapq)
 * The 32 counters are FLAGSTAT_scalar's over {array[i] : pass(i), 0 <= i < n}; `selected` is the number of i with pass(i).
 * require & exclude != 0 is legal, as in samtools, and passes nothing (nothing is launched).  min_mapq == 0 reads no byte of
 * `mapq`, which may then be NULL; require == exclude == 0 with min_mapq == 0 is the plain count, selected == n.
 * `flags`: as for the `where` entries -- bit 0 = store (out = counters, all 32 slots written; selected = count) instead of +=;
 * bit 1 = superset (slots 0 / 16 = primary paired reads among those that pass, slot 9 = selected minus slot 25).  `selected` /
 * `d_selected` may be NULL: nothing is reported.  n == 0 succeeds and touches nothing (the store form writes zeros).
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, out and selected untouched, nothing launched): require or exclude above
 * 0xFFFF, min_mapq above 255, a NULL mapq with min_mapq > 0 and n > 0, a NULL array with n > 0, an odd array pointer, flag bits
 * other than 0 and 1, NULL counters, an n with n * 2 not a size or too large for a wave's uint32 totals; for the device forms also
 * a d_out or d_selected that is not plain device memory, pointers on different devices, a stream of another device and an
 * allocation shorter than the call needs (d_array: n * 2 bytes, d_mapq: n bytes when min_mapq > 0, d_out: 256, d_selected: 8). */
/* DEVICE array and MAPQ column, DEVICE d_out[32] and d_selected[1] (uint64); asynchronous on `stream`: ONE kernel (the store form
 * puts one memset per pointer in front of it; one in all when d_selected == d_out + 32), no workspace.  Adds are atomic: launches
 * on several streams may share d_out and d_selected in the += form. */
int FLAGSTATS_hip_device_u16_filter(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                    uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected, int flags, void* stream);
/* DEVICE array and MAPQ column, HOST out[32] and selected[1]; synchronous */
int FLAGSTATS_hip_device_u16_filter_sync(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                         uint32_t min_mapq, uint64_t* out, uint64_t* selected, int flags);
/* HOST array and MAPQ column, HOST out[32] and selected[1]; synchronous.  Array and column cross the bus in the engine's chunks
 * (knob "chunk_flags"), each chunk's slice of the column behind its flags; the counters are summed on the device. */
int FLAGSTATS_hip_u16_x64_filter(const uint16_t* array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* mapq,
                                 uint32_t min_mapq, uint64_t* out, uint64_t* selected, int flags);

/* ================= filtered, the whole predicate: samtools' view filter -f / -F / --rf / -G / -q =================
 * The filtered entries with the two options of `samtools view` that no require / exclude pair can express once they name two
 * bits: --rf (--incl-flags) include_any keeps a read only if it has AT LEAST ONE of these bits (--rf 0x50: first or reverse), -G
 * exclude_all drops a read only if it has ALL of these bits (-G 0xC: read and mate both unmapped).  uint16 arrays as a whole only.
 *   pass(i) = (array[i] & require) == require && (array[i] & exclude) == 0
 *             && (include_any == 0 || (array[i] & include_any) != 0)
 *             && (exclude_all == 0 || (array[i] & exclude_all) != exclude_all)
 *             && (min_mapq == 0 || mapq[i] >= min_mapq)
 * include_any == 0 and exclude_all == 0 switch those tests off; with both 0 the entries are the filtered entries.  Everything
 * else is the filtered entries' contract: the 32 counters over {array[i] : pass(i), 0 <= i < n} and the optional superset (slot 9
 * from the passing count), `selected`, `flags` (bit 0 store, bit 1 superset), min_mapq == 0 reads no byte of `mapq`, which may
 * then be NULL, otherwise exactly mapq[0 .. n) is read; n == 0 succeeds and touches nothing (the store form writes zeros).
 * The four masks are first reduced exactly on the host (a single --rf bit is a required bit, a single -G bit an excluded one, a
 * bit that -f / -F already decide leaves --rf / -G), and by what is left a call is one of three things:
 *   nothing can pass (require & exclude != 0, every --rf bit excluded, every -G bit required): nothing is launched or read; the
 *       store form still zeroes
 *   a plain require / exclude pair is left: the launch is the filtered entries' kernel, at its speed
 *   a residue of two or more free bits in --rf or -G is left: one kernel of its own (fsk::flagstat_count_filter_rf)
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, out and selected untouched, nothing launched): what the filtered
 * entries refuse, and include_any or exclude_all above 0xFFFF. */
/* DEVICE array and MAPQ column, DEVICE d_out[32] and d_selected[1] (uint64); asynchronous on `stream`: ONE kernel (the store form
 * puts one memset per pointer in front of it; one in all when d_selected == d_out + 32), no workspace, nothing synchronised; may
 * be captured into a graph.  Adds are atomic: launches on several streams may share d_out and d_selected in the += form. */
int FLAGSTATS_hip_device_u16_filter_rf(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude, uint32_t include_any,
                                       uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* d_out,
                                       uint64_t* d_selected, int flags, void* stream);
/* DEVICE array and MAPQ column, HOST out[32] and selected[1]; synchronous */
int FLAGSTATS_hip_device_u16_filter_rf_sync(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude,
                                            uint32_t include_any, uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq,
                                            uint64_t* out, uint64_t* selected, int flags);
/* HOST array and MAPQ column, HOST out[32] and selected[1]; synchronous.  Array and column cross the bus in the engine's chunks
 * (knob "chunk_flags"), each chunk's slice of the column behind its flags; the counters are summed on the device. */
int FLAGSTATS_hip_u16_x64_filter_rf(const uint16_t* array, uint64_t n, uint32_t require, uint32_t exclude, uint32_t include_any,
                                    uint32_t exclude_all, const uint8_t* mapq, uint32_t min_mapq, uint64_t* out, uint64_t* selected,
                                    int flags);

/* ================= filtered and selected: samtools' view filter -f / -F / -q under a bitmap or a byte mask =================
 * The table for `-F 0x904 -q 30` of a FLAG column that has a validity bitmap (Arrow leaves the value of a null slot unspecified,
 * so a null FLAG must not be tested or counted), or of the reads that pass the filter AND lie in a region / read-group / dedup
 * mask: filter and selection together, in one kernel and one pass, with no combined mask in memory.
 *   counted(i) = pass(i) && sel(i)
 * pass(i) is exactly that of the filtered entries (require, exclude, mapq, min_mapq) and sel(i) exactly that of the `where`
 * entries (sel_bits == 1: an LSB-first bitmap at any sel_offset; sel_bits == 8: one byte per element, any non-zero byte
 * selects).  The 32 counters are FLAGSTAT_scalar's over {array[i] : counted(i), 0 <= i < n}; `selected` is the number of i with
 * counted(i).  require & exclude != 0 is legal and counts nothing (nothing is launched, nothing is read).  min_mapq == 0 reads
 * no byte of `mapq`, which may then be NULL; otherwise exactly mapq[0 .. n) is read.  Only bytes of `sel` that hold the bit or
 * byte of an element are read.  The FLAG or MAPQ of an element that is not selected may be read; it enters no counter and no
 * count.  A NULL selection with n > 0 is refused: the filtered entries are the call without one.
 * `flags`: as for both parents -- bit 0 = store (out = counters, all 32 slots written; selected = count) instead of +=; bit 1 =
 * superset (slots 0 / 16 = primary paired reads among those counted, slot 9 = selected minus slot 25).  `selected` /
 * `d_selected` may be NULL: nothing is reported.  n == 0 succeeds and touches nothing (the store form writes zeros).
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, out and selected untouched, nothing launched): what the filtered or
 * the `where` entries refuse -- require or exclude above 0xFFFF, min_mapq above 255, sel_bits other than 1 or 8, flag bits other
 * than 0 and 1, a NULL array, a NULL mapq with min_mapq > 0 or a NULL selection with n > 0, an odd array pointer, an n with n * 2
 * not a size or too large for a wave's uint32 totals, a sel_offset + n that is no index, NULL counters; for the device forms also
 * a d_out or d_selected that is not plain device memory, pointers on different devices, a stream of another device and an
 * allocation shorter than the call needs (d_array: n * 2 bytes, d_mapq: n bytes when min_mapq > 0, d_sel: the bytes that hold the
 * n bits or bytes, d_out: 256, d_selected: 8). */
/* DEVICE array, MAPQ column and selection, DEVICE d_out[32] and d_selected[1] (uint64); asynchronous on `stream`: ONE kernel (the
 * store form puts one memset per pointer in front of it; one in all when d_selected == d_out + 32), no workspace, nothing
 * synchronised; may be captured into a graph.  Adds are atomic: launches on several streams may share d_out and d_selected in
 * the += form. */
int FLAGSTATS_hip_device_u16_filter_where(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude,
                                          const uint8_t* d_mapq, uint32_t min_mapq, const void* d_sel, uint64_t sel_offset,
                                          int sel_bits, uint64_t* d_out, uint64_t* d_selected, int flags, void* stream);
/* DEVICE array, MAPQ column and selection, HOST out[32] and selected[1]; synchronous */
int FLAGSTATS_hip_device_u16_filter_where_sync(const uint16_t* d_array, uint64_t n, uint32_t require, uint32_t exclude,
                                               const uint8_t* d_mapq, uint32_t min_mapq, const void* d_sel, uint64_t sel_offset,
                                               int sel_bits, uint64_t* out, uint64_t* selected, int flags);
/* HOST array, MAPQ column and selection, HOST out[32] and selected[1]; synchronous.  All three cross the bus in the engine's
 * chunks (knob "chunk_flags"), each chunk's slices of the column and of the selection behind its flags; the counters are summed
 * on the device. */
int FLAGSTATS_hip_u16_x64_filter_where(const uint16_t* array, uint64_t n, uint32_t require, uint32_t exclude, const uint8_t* mapq,
                                       uint32_t min_mapq, const void* sel, uint64_t sel_offset, int sel_bits, uint64_t* out,
                                       uint64_t* selected, int flags);

/* ================= filtered segments: samtools' view filter -f / -F / -q per segment =================
 * Per-contig, per-sample or per-block tables of the reads that pass `-F 0x904 -q 30`: the segmented entries under the filtered
 * entries' predicate, in one launch.  Segment i is [offsets[i], offsets[i+1]) under the contract of the segmented entries;
 * pass(j) is that of the filtered entries (an overlapping pair is legal, selects nothing and launches nothing; min_mapq == 0
 * reads no byte of `mapq`, which may then be NULL).  Row i of out[nseg][32] holds FLAGSTAT_scalar's counters over
 * {array[j] : j in segment i, pass(j)}, and selected[i] (nseg uint64; the pointer may be NULL: nothing is reported) the number
 * of such j.  Flags outside every segment count nowhere.
 * `flags`: bit 0 = store (rows and selected[0 .. nseg) are zeroed in front, every slot of every row is written, empty segments
 * read 0) instead of +=; bit 1 = superset (slots 0 / 16 = primary paired reads among those that pass, slot 9 = selected[i]
 * minus slot 25).  nseg == 0 succeeds and touches nothing.
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, out and selected untouched, nothing launched): require or exclude above
 * 0xFFFF, min_mapq above 255, a NULL mapq with min_mapq > 0 and n > 0, a NULL array with n > 0, an odd array pointer, flag bits
 * other than 0 and 1, NULL offsets or rows with nseg > 0, host offsets that decrease or end beyond n, an nseg whose rows cannot be
 * allocated, an n with n * 2 not a size or too large for a wave's uint32 totals; for the device form also a d_out or d_selected
 * that is not plain device memory, pointers on different devices, a stream of another device and an allocation shorter than the
 * call needs (d_array: n * 2 bytes, d_mapq: n bytes when min_mapq > 0, d_offsets: (nseg + 1) * 8, d_out: nseg * 256,
 * d_selected: nseg * 8).  Device offsets are not checked (that would synchronise): every offset the kernel reads is clamped to
 * [0, n], so bad offsets give undefined counters and never an access outside the array, the column (read only at bytes of
 * elements in [0, n)), the rows or the counts. */
/* DEVICE array, column and offsets, DEVICE d_out[nseg][32] and d_selected[nseg] (uint64); asynchronous on `stream`: ONE kernel
 * (the store form puts one memset per pointer in front of it), no workspace.  Adds are atomic: launches on several streams may
 * share d_out and d_selected in the += form. */
int FLAGSTATS_hip_device_u16_segments_filter(const uint16_t* d_array, uint64_t n, const uint64_t* d_offsets, uint64_t nseg,
                                             uint32_t require, uint32_t exclude, const uint8_t* d_mapq, uint32_t min_mapq,
                                             uint64_t* d_out, uint64_t* d_selected, int flags, void* stream);
/* DEVICE array and column, HOST offsets, HOST out[nseg][32] and selected[nseg]; synchronous */
int FLAGSTATS_hip_device_u16_segments_filter_sync(const uint16_t* d_array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                                  uint32_t require, uint32_t exclude, const uint8_t* d_mapq, uint32_t min_mapq,
                                                  uint64_t* out, uint64_t* selected, int flags);
/* HOST array, column and offsets, HOST out[nseg][32] and selected[nseg]; synchronous.  Only [offsets[0], offsets[nseg]) of array
 * and column crosses the bus, in the engine's chunks (knob "chunk_flags"), each chunk's slice of the column behind its flags; a
 * segment that spans chunks is summed on the device. */
int FLAGSTATS_hip_u16_x64_segments_filter(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                          uint32_t require, uint32_t exclude, const uint8_t* mapq, uint32_t min_mapq,
                                          uint64_t* out, uint64_t* selected, int flags);

/* ================= selected elements per segment: the bitmap or byte mask under CSR segments =================
 * Per-contig, per-sample, per-read-group or per-block tables over the rows that a mask picks -- an Arrow validity bitmap, the
 * result of an upstream query, a deduplication or region mask: the segmented entries under the `where` entries' selection, in one
 * launch, instead of one `where` launch per segment or a compaction in front.  Segment i is [offsets[i], offsets[i+1]) under the
 * contract of the segmented entries.  The selection is indexed by ARRAY ELEMENT, not by segment: element j of the array is bit
 * (sel_bits == 1, LSB-first bitmap, any sel_offset) or byte (sel_bits == 8, any non-zero byte selects) sel_offset + j of `sel`,
 * as in the `where` entries.  Row i of out[nseg][32] holds FLAGSTAT_scalar's counters over {array[j] : j in segment i, sel(j)},
 * and selected[i] (nseg uint64; the pointer may be NULL: nothing is reported) the number of such j.  Flags outside every segment
 * count nowhere, selected or not.  Only bytes of `sel` that hold the bit or byte of an element of [0, n) are ever read.
 * `flags`: bit 0 = store (rows and selected[0 .. nseg) are zeroed in front, every slot of every row and every selected[i] is
 * written, empty segments and segments with nothing selected read 0) instead of +=; bit 1 = superset (slots 0 / 16 = primary
 * paired reads among the selected, slot 9 = selected[i] minus slot 25).  nseg == 0 succeeds and touches nothing.
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, out and selected untouched, nothing launched): sel_bits other than 1 or
 * 8, flag bits other than 0 and 1, NULL offsets or rows with nseg > 0, a NULL array or selection with n > 0 and nseg > 0, an odd
 * array pointer, an n with n * 2 not a size, a sel_offset + n that is no index, host offsets that decrease or end beyond n, an nseg
 * whose rows cannot be allocated, an n too large for a wave's uint32 totals; for the device forms also a d_out or d_selected that
 * is not plain device memory, pointers on different devices, a stream of another device and an allocation shorter than the call
 * needs (d_array: n * 2 bytes, d_sel: from d_sel up to the last byte that holds an element's bit or byte, d_offsets:
 * (nseg + 1) * 8, d_out: nseg * 256, d_selected: nseg * 8).  Device offsets are not checked (that would synchronise): every
 * offset the kernel reads is clamped to [0, n], so bad offsets give undefined counters and never an access outside the array,
 * the selection's bytes of elements, the rows or the counts. */
/* DEVICE array, selection and offsets, DEVICE d_out[nseg][32] and d_selected[nseg] (uint64); asynchronous on `stream`: ONE kernel
 * (the store form puts one memset per pointer in front of it), no workspace, so a captured launch holds no pointer of the
 * library's; make one plain call before capturing.  Adds are atomic: launches on several streams may share d_out and
 * d_selected in the += form. */
int FLAGSTATS_hip_device_u16_segments_where(const uint16_t* d_array, uint64_t n, const uint64_t* d_offsets, uint64_t nseg,
                                            const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* d_out,
                                            uint64_t* d_selected, int flags, void* stream);
/* DEVICE array and selection, HOST offsets, HOST out[nseg][32] and selected[nseg]; synchronous */
int FLAGSTATS_hip_device_u16_segments_where_sync(const uint16_t* d_array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                                 const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* out,
                                                 uint64_t* selected, int flags);
/* HOST array, selection and offsets, HOST out[nseg][32] and selected[nseg]; synchronous.  Only [offsets[0], offsets[nseg]) of the
 * array and the selection bytes that cover it cross the bus, in the engine's chunks (knob "chunk_flags"), each chunk's slice of
 * the selection behind its flags; a segment that spans chunks is summed on the device. */
int FLAGSTATS_hip_u16_x64_segments_where(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg, const void* sel,
                                         uint64_t sel_offset, int sel_bits, uint64_t* out, uint64_t* selected, int flags);

/* ================= filtered and selected per segment: -f / -F / -q under a bitmap or byte mask, per CSR segment =================
 * The table of `-F 0x904 -q 30` per row group, contig, sample or block of a FLAG column that has a validity bitmap (Arrow leaves
 * the value of a null slot unspecified, so a null FLAG must not be tested, counted or reported in selected[i]), or of the reads
 * that pass the filter AND lie in a region / read-group / dedup mask: the filtered segmented entries and the selected segmented
 * entries together, in one launch and one pass, with no combined mask in memory, instead of one filter_where launch per segment.
 *   counted(j) = pass(j) && sel(j)
 * Segment i is [offsets[i], offsets[i+1]) under the contract of the segmented entries.  pass(j) is exactly that of the filtered
 * entries (require, exclude, mapq, min_mapq: an overlapping pair is legal, counts nothing, launches nothing and reads nothing;
 * min_mapq == 0 reads no byte of `mapq`, which may then be NULL) and sel(j) exactly that of the `where` entries, indexed by ARRAY
 * ELEMENT, not by segment (sel_bits == 1: bit sel_offset + j of an LSB-first bitmap, any sel_offset; sel_bits == 8: byte
 * sel_offset + j, any non-zero byte selects).  Row i of out[nseg][32] holds FLAGSTAT_scalar's counters over
 * {array[j] : j in segment i, counted(j)}, and selected[i] (nseg uint64; the pointer may be NULL: nothing is reported) the number
 * of such j.  Flags outside every segment count nowhere.  Only bytes of `sel` that hold the bit or byte of an element of [0, n)
 * are ever read, and of `mapq` only bytes of elements of [0, n).  The FLAG or MAPQ of an element that is not selected may be
 * read; it enters no counter and no count.  A NULL selection with n > 0 is refused: the filtered segmented entries are the call
 * without one.
 * `flags`: bit 0 = store (rows and selected[0 .. nseg) are zeroed in front, every slot of every row and every selected[i] is
 * written, empty segments and segments with nothing counted read 0) instead of +=; bit 1 = superset (slots 0 / 16 = primary
 * paired reads among those counted, slot 9 = selected[i] minus slot 25).  nseg == 0 succeeds and touches nothing.
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, out and selected untouched, nothing launched): what the filtered
 * segmented or the selected segmented entries refuse -- require or exclude above 0xFFFF, min_mapq above 255, sel_bits other than
 * 1 or 8, flag bits other than 0 and 1, NULL offsets or rows with nseg > 0, an nseg whose rows cannot be allocated, and with
 * nseg > 0 a NULL array, a NULL mapq with min_mapq > 0 or a NULL selection with n > 0, an odd array pointer, an n with n * 2 not
 * a size, a sel_offset + n that is no index, host offsets that decrease or end beyond n, an n too large for a wave's uint32
 * totals; for the device forms also a d_out or d_selected that is not plain device memory, pointers on different devices, a
 * stream of another device and an allocation shorter than the call needs (d_array: n * 2 bytes, d_mapq: n bytes when
 * min_mapq > 0, d_sel: from d_sel up to the last byte that holds an element's bit or byte, d_offsets: (nseg + 1) * 8, d_out:
 * nseg * 256, d_selected: nseg * 8).  Device offsets are not checked (that would synchronise): every offset the kernel reads is
 * clamped to [0, n], so bad offsets give undefined counters and never an access outside the array, the column's and the
 * selection's bytes of elements, the rows or the counts. */
/* DEVICE array, column, selection and offsets, DEVICE d_out[nseg][32] and d_selected[nseg] (uint64); asynchronous on `stream`: ONE
 * kernel (the store form puts one memset per pointer in front of it), no workspace, so a captured launch holds no pointer of the
 * library's; make one plain call before capturing.  Adds are atomic: launches on several streams may share d_out and
 * d_selected in the += form. */
int FLAGSTATS_hip_device_u16_segments_filter_where(const uint16_t* d_array, uint64_t n, const uint64_t* d_offsets, uint64_t nseg,
                                                   uint32_t require, uint32_t exclude, const uint8_t* d_mapq, uint32_t min_mapq,
                                                   const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* d_out,
                                                   uint64_t* d_selected, int flags, void* stream);
/* DEVICE array, column and selection, HOST offsets, HOST out[nseg][32] and selected[nseg]; synchronous */
int FLAGSTATS_hip_device_u16_segments_filter_where_sync(const uint16_t* d_array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                                        uint32_t require, uint32_t exclude, const uint8_t* d_mapq, uint32_t min_mapq,
                                                        const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* out,
                                                        uint64_t* selected, int flags);
/* HOST array, column, selection and offsets, HOST out[nseg][32] and selected[nseg]; synchronous.  Only [offsets[0], offsets[nseg])
 * of the array, of the column (when min_mapq > 0) and the selection bytes that cover it cross the bus, in the engine's chunks
 * (knob "chunk_flags"), each chunk's slices of the column and of the selection behind its flags; a segment that spans chunks is
 * summed on the device. */
int FLAGSTATS_hip_u16_x64_segments_filter_where(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                                uint32_t require, uint32_t exclude, const uint8_t* mapq, uint32_t min_mapq,
                                                const void* sel, uint64_t sel_offset, int sel_bits, uint64_t* out, uint64_t* selected,
                                                int flags);

/* ================= filtered wide input: -f / -F / -q on a FLAG column held as 4-byte or 8-byte integers =================
 * The two normal cases at once: the column arrives as int32 or int64 (the wide entries) and the table wanted is that of
 * `samtools view -F 0x904 -q 30` (the filtered entries).  One pass over the array as it is, no uint16 copy, no mask array.
 * With f(i) = the low 16 bits of element i (little-endian elements of `elem_bytes` = 4 or 8 bytes, aligned to elem_bytes):
 *   pass(i) = (f(i) & require) == require && (f(i) & exclude) == 0 && (min_mapq == 0 || mapq[i] >= min_mapq)
 * (`mapq`: one uint8 per element, at any byte alignment; min_mapq == 0 reads no byte of it and it may then be NULL).
 *   out      : FLAGSTAT_scalar's 32 counters over {f(i) : pass(i), 0 <= i < n}
 *   selected : the number of i with pass(i)
 *   high     : OR of (element & ~0xFFFF), taken as unsigned, over ALL n elements the call reads, passing or not.  The predicate
 *              sees only the low 16 bits; an element whose low bits fail still reports its high bits: the mask says whether the
 *              column is a valid FLAG column, not whether the selected reads are.
 * require & exclude != 0 is legal, as in samtools, and passes nothing: nothing is launched and NO ELEMENT IS READ, so `high` is
 * then 0 in the store form and untouched in the += form -- it says nothing about the column.  require == exclude == 0 with
 * min_mapq == 0 is the wide count, selected == n.
 * `flags`: bit 0 = store (out = counters, all 32 slots written; selected = count; high = mask) instead of out += counters,
 * selected += count, high |= mask; bit 1 = superset (slots 0 / 16 = primary paired reads among those that pass, slot 9 =
 * selected minus slot 25).  `selected` / `d_selected` and `high` / `d_high` may each be NULL: that value is not reported.
 * n == 0 succeeds and touches nothing (the store form writes zeros).
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, outputs untouched, nothing launched): elem_bytes other than 4 or 8
 * (2: use the u16 filter entries), an array pointer not aligned to elem_bytes, an n with n * elem_bytes not a size or too large
 * for a wave's uint32 totals, require or exclude above 0xFFFF, min_mapq above 255, a NULL mapq with min_mapq > 0 and n > 0, a
 * NULL array with n > 0, flag bits other than 0 and 1, NULL counters; for the device form also a d_out, d_selected or d_high
 * that is not plain device memory, host memory for d_array or d_mapq, pointers on different devices, a stream of another device
 * and an allocation shorter than the call needs (d_array: n * elem_bytes bytes, d_mapq: n bytes when min_mapq > 0, d_out: 256,
 * d_selected: 8, d_high: 8). */
/* DEVICE array and MAPQ column, DEVICE d_out[32], d_selected[1] and d_high[1] (uint64); asynchronous on `stream`: ONE kernel
 * (the store form puts one memset per pointer in front of it; one in all when d_selected == d_out + 32 and d_high == d_out + 33),
 * no workspace.  Adds and ORs are atomic: launches on several streams may share the three in the += form. */
int FLAGSTATS_hip_device_wide_filter(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                     const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected,
                                     uint64_t* d_high, int flags, void* stream);
/* DEVICE array and MAPQ column, HOST out[32], selected[1] and high[1]; synchronous */
int FLAGSTATS_hip_device_wide_filter_sync(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                          const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* out, uint64_t* selected,
                                          uint64_t* high, int flags);
/* HOST array and MAPQ column, HOST out[32], selected[1] and high[1]; synchronous.  The array crosses the bus as it is in the
 * engine's chunks (knob "chunk_flags": chunk_flags * 2 bytes of elements each), each chunk's slice of the column behind its
 * elements; counters, count and mask are summed / ORed on the device. */
int FLAGSTATS_hip_wide_x64_filter(const void* array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                  const uint8_t* mapq, uint32_t min_mapq, uint64_t* out, uint64_t* selected, uint64_t* high,
                                  int flags);

/* ================= filtered wide input, the whole predicate: -f / -F / --rf / -G / -q on a 4-byte or 8-byte FLAG column =========
 * The filtered wide entries with the two options of `samtools view` that no require / exclude pair can express once they name two
 * bits (--rf include_any: AT LEAST ONE of these bits; -G exclude_all: not ALL of these bits), on the column as it arrives: int32
 * or int64, read once and in place.  Whole columns only.  With f(i) = the low 16 bits of element i:
 *   pass(i) = (f(i) & require) == require && (f(i) & exclude) == 0
 *             && (include_any == 0 || (f(i) & include_any) != 0)
 *             && (exclude_all == 0 || (f(i) & exclude_all) != exclude_all)
 *             && (min_mapq == 0 || mapq[i] >= min_mapq)
 * include_any == 0 and exclude_all == 0 switch those tests off; with both 0 the entries are the filtered wide entries.  Everything
 * else is the filtered wide entries' contract: out, selected and high, `flags`, NULL selected / high, the MAPQ column, n == 0.
 * The whole predicate sees the low 16 bits only: a bit above bit 15 satisfies no --rf and completes no -G, and is reported in
 * `high` whether its element passes or not.
 * The four masks are first reduced exactly on the host, as for the uint16 entries of the whole predicate, and by what is left a
 * call is one of three things:
 *   nothing can pass (require & exclude != 0, every --rf bit excluded, every -G bit required): nothing is launched and NO ELEMENT
 *       IS READ, so `high` is then 0 in the store form and untouched in the += form, like out and selected -- it says nothing
 *       about the column
 *   a plain require / exclude pair is left: the launch is the filtered wide entries' kernel, at its speed
 *   a residue of two or more free bits in --rf or -G is left: one kernel of its own (fsk::flagstat_count_wide_filter_rf)
 * In the last two `high` is the OR over all n elements, whatever min_mapq is.
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, outputs untouched, nothing launched): what the filtered wide entries
 * refuse (elem_bytes 2: use the u16 entries of the whole predicate), and include_any or exclude_all above 0xFFFF. */
/* DEVICE array and MAPQ column, DEVICE d_out[32], d_selected[1] and d_high[1] (uint64); asynchronous on `stream`: ONE kernel
 * (the store form puts one memset per pointer in front of it; one in all when d_selected == d_out + 32 and d_high == d_out + 33),
 * no workspace, nothing synchronised; may be captured into a graph.  Adds and ORs are atomic: launches on several streams may
 * share the three in the += form. */
int FLAGSTATS_hip_device_wide_filter_rf(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                        uint32_t include_any, uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq,
                                        uint64_t* d_out, uint64_t* d_selected, uint64_t* d_high, int flags, void* stream);
/* DEVICE array and MAPQ column, HOST out[32], selected[1] and high[1]; synchronous */
int FLAGSTATS_hip_device_wide_filter_rf_sync(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                             uint32_t include_any, uint32_t exclude_all, const uint8_t* d_mapq, uint32_t min_mapq,
                                             uint64_t* out, uint64_t* selected, uint64_t* high, int flags);
/* HOST array and MAPQ column, HOST out[32], selected[1] and high[1]; synchronous.  The array crosses the bus as it is in the
 * engine's chunks (knob "chunk_flags": chunk_flags * 2 bytes of elements each), each chunk's slice of the column behind its
 * elements; counters, count and mask are summed / ORed on the device. */
int FLAGSTATS_hip_wide_x64_filter_rf(const void* array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                     uint32_t include_any, uint32_t exclude_all, const uint8_t* mapq, uint32_t min_mapq,
                                     uint64_t* out, uint64_t* selected, uint64_t* high, int flags);

/* ================= selected elements of wide input: a bitmap or byte mask on a FLAG column of 4-byte or 8-byte integers =========
 * An Arrow FLAG column is both at once: int32 values and an LSB-first validity bitmap at some bit offset.  One pass over the
 * array as it is and its selection: no uint16 copy in front (which would turn a negative element or one >= 65,536 into a
 * plausible FLAG), no compaction, no unpacked bitmap.  With f(i) = the low 16 bits of element i (little-endian elements of
 * `elem_bytes` = 4 or 8 bytes, aligned to elem_bytes) and sel(i) exactly as in FLAGSTATS_hip_device_u16_where (sel_bits == 1:
 * bit sel_offset + i of an LSB-first bitmap, any bit offset; sel_bits == 8: byte sel_offset + i, any non-zero byte selects):
 *   out      : FLAGSTAT_scalar's 32 counters over {f(i) : sel(i), 0 <= i < n}
 *   selected : the number of i with sel(i)
 *   high     : OR of (element & ~0xFFFF), taken as unsigned, over the SELECTED elements ONLY.  This differs on purpose from the
 *              filtered wide entries above, whose `high` covers every element read, passing or not: a selection is typically a
 *              validity bitmap and the value of a null slot is unspecified, so what lies in a slot that is not selected must not
 *              make high != 0.  high == 0 says that every selected element is a valid 16-bit FLAG, and nothing about the others.
 * Only bytes of `sel` that hold the bit or byte of an element of [0, n) and only dwords of elements of [0, n) are ever read.
 * `flags`: bit 0 = store (out = counters, all 32 slots written; selected = count; high = mask) instead of out += counters,
 * selected += count, high |= mask; bit 1 = superset (slots 0 / 16 = primary paired reads among the selected, slot 9 = selected
 * minus slot 25).  `selected` / `d_selected` and `high` / `d_high` may each be NULL: that value is not reported.
 * n == 0 succeeds and touches nothing (the store form writes zeros to all three).
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, outputs untouched, nothing launched): elem_bytes other than 4 or 8
 * (2: use the u16 where entries), sel_bits other than 1 or 8, an array pointer not aligned to elem_bytes, an n with n * elem_bytes
 * not a size or too large for a wave's uint32 totals, a sel_offset + n that is no index, a NULL array or selection with n > 0,
 * flag bits other than 0 and 1, NULL counters; for the device form also a d_out, d_selected or d_high that is not plain device
 * memory, host memory for d_array or d_sel, pointers on different devices, a stream of another device and an allocation shorter
 * than the call needs (d_array: n * elem_bytes bytes, d_sel: from d_sel up to the last byte that holds an element's bit or
 * byte, d_out: 256, d_selected: 8, d_high: 8). */
/* DEVICE array and selection, DEVICE d_out[32], d_selected[1] and d_high[1] (uint64); asynchronous on `stream`: ONE kernel (the
 * store form puts one zeroing per pointer in front of it; one in all when d_selected == d_out + 32 and d_high == d_out + 33), no
 * workspace, so a captured launch holds no pointer of the library's (capture and replay: tests/test_gpu_wide_where_graphs.py;
 * make one plain call before capturing).  Adds and ORs are atomic: launches on several streams may share the three in the +=
 * form. */
int FLAGSTATS_hip_device_wide_where(const void* d_array, uint64_t n, int elem_bytes, const void* d_sel, uint64_t sel_offset,
                                    int sel_bits, uint64_t* d_out, uint64_t* d_selected, uint64_t* d_high, int flags, void* stream);
/* DEVICE array and selection, HOST out[32], selected[1] and high[1]; synchronous */
int FLAGSTATS_hip_device_wide_where_sync(const void* d_array, uint64_t n, int elem_bytes, const void* d_sel, uint64_t sel_offset,
                                         int sel_bits, uint64_t* out, uint64_t* selected, uint64_t* high, int flags);
/* HOST array and selection, HOST out[32], selected[1] and high[1]; synchronous.  The array crosses the bus as it is in the
 * engine's chunks (knob "chunk_flags": chunk_flags * 2 bytes of elements each), each chunk's slice of the selection behind its
 * elements (a bitmap slice from the byte that holds the chunk's first bit); counters, count and mask are summed / ORed on the
 * device. */
int FLAGSTATS_hip_wide_x64_where(const void* array, uint64_t n, int elem_bytes, const void* sel, uint64_t sel_offset, int sel_bits,
                                 uint64_t* out, uint64_t* selected, uint64_t* high, int flags);

/* ================= filter AND selection on wide input: -f / -F / -q under a bitmap or byte mask, int32 / int64 column ==========
 * What an Arrow / Parquet / pandas / torch reader holds: the FLAG column as int32 or int64, an LSB-first validity bitmap (often
 * sliced to an odd bit offset) and a uint8 MAPQ column -- and it wants `samtools view -F 0x904 -q 30 | samtools flagstat` over the
 * valid rows.  One pass and one kernel over the three as they are.  With f(i) = the low 16 bits of element i (little-endian
 * elements of `elem_bytes` = 4 or 8 bytes, aligned to elem_bytes), pass(i) exactly as in FLAGSTATS_hip_device_wide_filter and
 * sel(i) exactly as in FLAGSTATS_hip_device_wide_where:
 *   out      : FLAGSTAT_scalar's 32 counters over {f(i) : pass(i) && sel(i), 0 <= i < n}
 *   selected : the number of i with pass(i) && sel(i)
 *   high     : OR of (element & ~0xFFFF), taken as unsigned, over the elements with sel(i), PASSING OR NOT.  Both parents' rules at
 *              once: the filter never restricts the mask (the predicate sees the low 16 bits only), the selection always does (the
 *              value of a null slot is unspecified).  With an all-ones selection the three are FLAGSTATS_hip_device_wide_filter's,
 *              with require == exclude == min_mapq == 0 they are FLAGSTATS_hip_device_wide_where's.
 * min_mapq == 0 reads no MAPQ byte and `mapq` may be NULL; otherwise only mapq[0 .. n) is read, at any alignment.  Only bytes of
 * `sel` that hold the bit or byte of an element of [0, n) and only dwords of elements of [0, n) are ever read; the FLAG or MAPQ
 * of an element that is not selected may be read but enters nothing.  require & exclude != 0 is legal: it counts nothing,
 * launches nothing and READS NOTHING, so `high` is 0 in the store form and untouched otherwise.
 * `flags`: bit 0 = store (out = counters, all 32 slots written; selected = count; high = mask) instead of out += counters,
 * selected += count, high |= mask; bit 1 = superset (slots 0 / 16 = primary paired reads among the counted, slot 9 = selected
 * minus slot 25).  `selected` / `d_selected` and `high` / `d_high` may each be NULL: that value is not reported.
 * n == 0 succeeds and touches nothing (the store form writes zeros to all three).
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, outputs untouched, nothing launched): everything the filtered wide
 * entries and the selected wide entries refuse, in their words -- elem_bytes other than 4 or 8 (2: use the u16 filter_where
 * entries), require or exclude above 0xFFFF, min_mapq above 255, sel_bits other than 1 or 8, an array pointer not aligned to
 * elem_bytes, an n with n * elem_bytes not a size or too large for a wave's uint32 totals, a sel_offset + n that is no index, a
 * NULL array with n > 0, a NULL mapq with min_mapq > 0 and n > 0, a NULL selection with n > 0 (no selection: use the filtered
 * wide entries), flag bits other than 0 and 1, NULL counters; for the device form also a d_out, d_selected or d_high that is not
 * plain device memory, host memory for d_array, d_sel or d_mapq, pointers on different devices, a stream of another device and
 * an allocation shorter than the call needs (d_array: n * elem_bytes bytes, d_mapq: n, d_sel: from d_sel up to the last byte
 * that holds an element's bit or byte, d_out: 256, d_selected: 8, d_high: 8). */
/* DEVICE array, MAPQ column and selection, DEVICE d_out[32], d_selected[1] and d_high[1] (uint64); asynchronous on `stream`: ONE
 * kernel (the store form puts one zeroing per pointer in front of it; one in all when d_selected == d_out + 32 and d_high ==
 * d_out + 33), no workspace, nothing synchronised, so a captured launch holds no pointer of the library's (capture and replay:
 * tests/test_gpu_wide_filter_where_graphs.py; make one plain call before capturing).  Adds and ORs are atomic: launches on
 * several streams may share the three in the += form. */
int FLAGSTATS_hip_device_wide_filter_where(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                           const uint8_t* d_mapq, uint32_t min_mapq, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                           uint64_t* d_out, uint64_t* d_selected, uint64_t* d_high, int flags, void* stream);
/* DEVICE array, MAPQ column and selection, HOST out[32], selected[1] and high[1]; synchronous */
int FLAGSTATS_hip_device_wide_filter_where_sync(const void* d_array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                                const uint8_t* d_mapq, uint32_t min_mapq, const void* d_sel, uint64_t sel_offset,
                                                int sel_bits, uint64_t* out, uint64_t* selected, uint64_t* high, int flags);
/* HOST array, MAPQ column and selection, HOST out[32], selected[1] and high[1]; synchronous.  The array crosses the bus as it is
 * in the engine's chunks (knob "chunk_flags": chunk_flags * 2 bytes of elements each), each chunk's slices of the MAPQ column and
 * of the selection behind its elements (a bitmap slice from the byte that holds the chunk's first bit); counters, count and mask
 * are summed / ORed on the device. */
int FLAGSTATS_hip_wide_x64_filter_where(const void* array, uint64_t n, int elem_bytes, uint32_t require, uint32_t exclude,
                                        const uint8_t* mapq, uint32_t min_mapq, const void* sel, uint64_t sel_offset, int sel_bits,
                                        uint64_t* out, uint64_t* selected, uint64_t* high, int flags);

/* ================= wide input per segment: a row and a high mask for every segment of an int32 / int64 column =================
 * The union of the segmented and the wide entries: segment i (i < nseg) is [offsets[i], offsets[i+1]) of an array of 4-byte or
 * 8-byte little-endian elements (aligned to elem_bytes), read as it is.  With f(j) = the low 16 bits of element j,
 *   out[i * 32 + slot] : FLAGSTAT_scalar's 32 counters over {f(j) : offsets[i] <= j < offsets[i+1]}
 *   high[i]            : OR over the elements j of segment i of (element & ~0xFFFF), taken as unsigned; 0 for an empty segment
 * so a non-zero mask names the segment that holds the out-of-range element.  Elements before offsets[0], after offsets[nseg]
 * and the bytes around the array enter no counter and no mask.  `high` / `d_high` may be NULL: no mask is reported.
 * `flags`: bit 0 = store (every slot of every row and every high[i] written; empty segments read 0) instead of out += counters,
 * high |= mask; bit 1 = superset (slots 0 / 16, and slot 9 = the segment's length minus its slot 25).  nseg == 0 succeeds and
 * touches nothing.
 * DEVICE offsets are clamped to [0, n] and not checked for order, as documented for FLAGSTATS_hip_device_u16_segments: malformed
 * offsets give undefined rows and masks, never an access outside the array, d_out[nseg][32] or d_high[nseg].  HOST offsets are
 * validated first (non-decreasing, offsets[nseg] <= n); on failure `out` and `high` are left untouched.
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, outputs untouched, nothing launched): elem_bytes other than 4 or 8 (2:
 * use the u16 segments entries), flag bits other than 0 and 1, an array pointer not aligned to elem_bytes, a NULL array with
 * n > 0, NULL offsets or out with nseg > 0, an nseg whose counters are not a size; for the device form also a d_out or d_high
 * that is not plain device memory, pointers on different devices, a stream of another device and an allocation shorter than the
 * call needs (d_array: n * elem_bytes bytes, d_offsets: (nseg + 1) * 8, d_out: nseg * 256, d_high: nseg * 8). */
/* DEVICE array and offsets, DEVICE d_out[nseg][32] and d_high[nseg] (uint64); asynchronous on `stream`: ONE kernel (the store
 * form puts one memset per pointer in front of it; one in all when d_high == d_out + nseg * 32), no workspace, so a captured
 * launch holds no pointer of the library's.  Adds and ORs are atomic: launches on several streams may share d_out and d_high in
 * the += form. */
int FLAGSTATS_hip_device_wide_segments(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* d_offsets, uint64_t nseg,
                                       uint64_t* d_out, uint64_t* d_high, int flags, void* stream);
/* DEVICE array, HOST offsets, HOST out[nseg][32] and high[nseg]; synchronous */
int FLAGSTATS_hip_device_wide_segments_sync(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* offsets,
                                            uint64_t nseg, uint64_t* out, uint64_t* high, int flags);
/* HOST array and offsets, HOST out[nseg][32] and high[nseg]; synchronous.  Only [offsets[0], offsets[nseg]) crosses the bus, as
 * it is, in the engine's chunks (knob "chunk_flags": chunk_flags * 2 bytes of elements each); a segment that spans chunks is
 * summed and ORed on the device. */
int FLAGSTATS_hip_wide_x64_segments(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg,
                                    uint64_t* out, uint64_t* high, int flags);

/* ================= filtered wide input per segment: -f / -F / -q for every segment of an int32 / int64 column =================
 * The last corner of the grid {uint16, wide} x {whole array, per segment} x {no predicate, filter}: the per-contig, per-sample or
 * per-block table of the reads passing `-F 0x904 -q 30`, straight from a FLAG column held as 4-byte or 8-byte little-endian
 * integers (aligned to elem_bytes), in one pass and one launch.  Segment i (i < nseg) is [offsets[i], offsets[i+1]).  With
 * f(j) = the low 16 bits of element j and
 *   pass(j) = (f(j) & require) == require && (f(j) & exclude) == 0 && (min_mapq == 0 || mapq[j] >= min_mapq)
 * (`mapq`: one uint8 per element of the whole array, at any byte alignment; min_mapq == 0 reads no byte of it and it may then
 * be NULL):
 *   out[i * 32 + slot] : FLAGSTAT_scalar's 32 counters over {f(j) : pass(j), offsets[i] <= j < offsets[i+1]}
 *   selected[i]        : the number of j in segment i with pass(j)
 *   high[i]            : OR of (element & ~0xFFFF), taken as unsigned, over EVERY element of segment i and of no other, passing
 *                        or not -- FLAGSTATS_hip_device_wide_filter's meaning per segment: the mask says whether the segment is
 *                        part of a valid FLAG column, and names the segment that holds an out-of-range element
 * Elements before offsets[0], after offsets[nseg] and the bytes around the array enter no counter, no count and no mask; empty
 * segments read 0.  `selected` / `d_selected` and `high` / `d_high` may each be NULL: that value is not reported.
 * require & exclude != 0 is legal and passes nothing: nothing is launched and NO ELEMENT IS READ, so in the store form rows,
 * counts and masks are 0 and in the += form they are untouched -- `high` then says nothing about the column.
 * `flags`: bit 0 = store (every slot of every row, every selected[i] and every high[i] written) instead of out += counters,
 * selected += count, high |= mask; bit 1 = superset (slots 0 / 16 = primary paired reads among those that pass, slot 9 =
 * selected[i] minus slot 25).  nseg == 0 succeeds and touches nothing.
 * DEVICE offsets are clamped to [0, n] and not checked for order, as documented for FLAGSTATS_hip_device_u16_segments: malformed
 * offsets give undefined rows, counts and masks, never an access outside the array, the column or the outputs.  HOST offsets are
 * validated first (non-decreasing, offsets[nseg] <= n); on failure the outputs are left untouched.
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, outputs untouched, nothing launched): elem_bytes other than 4 or 8 (2:
 * use the u16 segmented filter entries), require or exclude above 0xFFFF, min_mapq above 255, flag bits other than 0 and 1, NULL
 * offsets or out with nseg > 0, an nseg whose counters are not a size, a NULL array with n > 0, a NULL mapq with min_mapq > 0
 * and n > 0, an array pointer not aligned to elem_bytes, an n with n * elem_bytes not a size or too large for a wave's uint32
 * totals; for the device form also a d_out, d_selected or d_high that is not plain device memory, host memory for d_array,
 * d_mapq or d_offsets, pointers on different devices, a stream of another device and an allocation shorter than the call needs
 * (d_array: n * elem_bytes bytes, d_mapq: n bytes when min_mapq > 0, d_offsets: (nseg + 1) * 8, d_out: nseg * 256, d_selected:
 * nseg * 8, d_high: nseg * 8). */
/* DEVICE array, MAPQ column and offsets, DEVICE d_out[nseg][32], d_selected[nseg] and d_high[nseg] (uint64); asynchronous on
 * `stream`: ONE kernel (the store form puts one memset per pointer in front of it; one in all when d_selected == d_out + nseg *
 * 32 and d_high == d_selected + nseg), no workspace, so a captured launch holds no pointer of the library's.  Adds and ORs are
 * atomic: launches on several streams may share the three in the += form. */
int FLAGSTATS_hip_device_wide_segments_filter(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* d_offsets,
                                              uint64_t nseg, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                              uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected, uint64_t* d_high,
                                              int flags, void* stream);
/* DEVICE array and MAPQ column, HOST offsets, HOST out[nseg][32], selected[nseg] and high[nseg]; synchronous */
int FLAGSTATS_hip_device_wide_segments_filter_sync(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* offsets,
                                                   uint64_t nseg, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                                   uint32_t min_mapq, uint64_t* out, uint64_t* selected, uint64_t* high,
                                                   int flags);
/* HOST array, MAPQ column and offsets, HOST out[nseg][32], selected[nseg] and high[nseg]; synchronous.  Only [offsets[0],
 * offsets[nseg]) of the array and of the column crosses the bus, in the engine's chunks (knob "chunk_flags": chunk_flags * 2
 * bytes of elements each, a chunk's slice of the column behind them); a segment that spans chunks is summed and ORed on the
 * device. */
int FLAGSTATS_hip_wide_x64_segments_filter(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg,
                                           uint32_t require, uint32_t exclude, const uint8_t* mapq, uint32_t min_mapq,
                                           uint64_t* out, uint64_t* selected, uint64_t* high, int flags);

/* ================= selected elements of wide input per segment: a bitmap or byte mask for every segment of an int32 / int64 column
 * What an Arrow / Parquet reader holds: an int32 (or int64) FLAG column, an LSB-first validity bitmap at some bit offset, and the
 * table wanted per row group, contig, sample or block.  One pass over the array as it is and its selection, one launch: no
 * uint16 copy in front, no compaction, no unpacked bitmap, no launch per segment.  Segment i (i < nseg) is [offsets[i],
 * offsets[i+1]) of an array of 4-byte or 8-byte little-endian elements (aligned to elem_bytes).  The selection is indexed by ARRAY
 * ELEMENT, not by segment, exactly as in FLAGSTATS_hip_device_wide_where (sel_bits == 1: bit sel_offset + j of an LSB-first bitmap,
 * any bit offset; sel_bits == 8: byte sel_offset + j, any non-zero byte selects).  With f(j) = the low 16 bits of element j and
 * S_i = {j : offsets[i] <= j < offsets[i+1], sel(j)}:
 *   out[i * 32 + slot] : FLAGSTAT_scalar's 32 counters over {f(j) : j in S_i}
 *   selected[i]        : the number of elements of S_i
 *   high[i]            : OR of (element & ~0xFFFF), taken as unsigned, over the SELECTED elements ONLY of segment i and of no
 *                        other -- FLAGSTATS_hip_device_wide_where's meaning per segment, NOT the filtered entries' (whose mask
 *                        covers every element of the segment): the value of a null slot is unspecified, so what lies in a slot
 *                        that is not selected must not make high[i] != 0
 * Garbage in a null slot, an unselected element, an element of a neighbouring segment or of a gap, elements before offsets[0] and
 * after offsets[nseg] and the bytes around the array enter no counter, no count and no mask; empty segments read 0.  Only bytes
 * of `sel` that hold the bit or byte of an element of [0, n) and only dwords of elements of [0, n) are ever read.  `selected` /
 * `d_selected` and `high` / `d_high` may each be NULL: that value is not reported.
 * `flags`: bit 0 = store (every slot of every row, every selected[i] and every high[i] written) instead of out += counters,
 * selected += count, high |= mask; bit 1 = superset (slots 0 / 16 = primary paired reads among the selected, slot 9 =
 * selected[i] minus slot 25).  nseg == 0 succeeds and touches nothing.
 * DEVICE offsets are clamped to [0, n] and not checked for order, as documented for FLAGSTATS_hip_device_u16_segments: malformed
 * offsets give undefined rows, counts and masks, never an access outside the array, the selection or the outputs.  HOST offsets
 * are validated first (non-decreasing, offsets[nseg] <= n); on failure the outputs are left untouched.
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, outputs untouched, nothing launched): elem_bytes other than 4 or 8 (2:
 * use the u16 segments_where entries), sel_bits other than 1 or 8, flag bits other than 0 and 1, NULL offsets or out with
 * nseg > 0, an nseg whose counters are not a size, a NULL array or selection with n > 0, an array pointer not aligned to
 * elem_bytes, an n with n * elem_bytes not a size or too large for a wave's uint32 totals, a sel_offset + n that is no index; for
 * the device form also a d_out, d_selected or d_high that is not plain device memory, host memory for d_array, d_sel or
 * d_offsets, pointers on different devices, a stream of another device and an allocation shorter than the call needs (d_array:
 * n * elem_bytes bytes, d_sel: from d_sel up to the last byte that holds an element's bit or byte, d_offsets: (nseg + 1) * 8,
 * d_out: nseg * 256, d_selected: nseg * 8, d_high: nseg * 8). */
/* DEVICE array, selection and offsets, DEVICE d_out[nseg][32], d_selected[nseg] and d_high[nseg] (uint64); asynchronous on
 * `stream`: ONE kernel (the store form puts one zeroing per pointer in front of it; one in all when d_selected == d_out + nseg *
 * 32 and d_high == d_selected + nseg), no workspace, nothing synchronised, so a captured launch holds no pointer of the library's
 * (make one plain call before capturing).  Adds and ORs are atomic: launches on several streams may share the three in the +=
 * form. */
int FLAGSTATS_hip_device_wide_segments_where(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* d_offsets,
                                             uint64_t nseg, const void* d_sel, uint64_t sel_offset, int sel_bits, uint64_t* d_out,
                                             uint64_t* d_selected, uint64_t* d_high, int flags, void* stream);
/* DEVICE array and selection, HOST offsets, HOST out[nseg][32], selected[nseg] and high[nseg]; synchronous */
int FLAGSTATS_hip_device_wide_segments_where_sync(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* offsets,
                                                  uint64_t nseg, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                                  uint64_t* out, uint64_t* selected, uint64_t* high, int flags);
/* HOST array, selection and offsets, HOST out[nseg][32], selected[nseg] and high[nseg]; synchronous.  Only [offsets[0],
 * offsets[nseg]) of the array and the selection bytes that cover it cross the bus, in the engine's chunks (knob "chunk_flags":
 * chunk_flags * 2 bytes of elements each), each chunk's slice of the selection behind its elements (a bitmap slice from the byte
 * that holds the chunk's first bit); a segment that spans chunks is summed and ORed on the device. */
int FLAGSTATS_hip_wide_x64_segments_where(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg,
                                          const void* sel, uint64_t sel_offset, int sel_bits, uint64_t* out, uint64_t* selected,
                                          uint64_t* high, int flags);

/* ================= filtered and selected wide input per segment: -f / -F / -q under a bitmap or byte mask for every segment of
 * an int32 / int64 column =================
 * The last cell of the grid {uint16, wide} x {whole array, per segment} x {no predicate, filter, mask, filter and mask}: what an
 * Arrow / Parquet reader wants of an int32 (or int64) FLAG column, its validity bitmap at some bit offset, a uint8 MAPQ column
 * and row-group, contig or sample offsets -- the `-F 0x904 -q 30` table per segment over the non-null rows -- in one pass over
 * the three columns as they are and one launch: no uint16 copy, no combined mask, no launch per segment.  Segment i (i < nseg) is
 * [offsets[i], offsets[i+1]) of an array of 4-byte or 8-byte little-endian elements (aligned to elem_bytes).  The predicate is
 * FLAGSTATS_hip_device_wide_segments_filter's (`mapq`: one uint8 per element of the whole array, at any byte alignment;
 * min_mapq == 0 reads no byte of it and it may then be NULL), the selection FLAGSTATS_hip_device_wide_segments_where's, indexed
 * by ARRAY ELEMENT (sel_bits == 1: bit sel_offset + j of an LSB-first bitmap, any bit offset; sel_bits == 8: byte sel_offset + j,
 * any non-zero byte selects).  With f(j) = the low 16 bits of element j:
 *   out[i * 32 + slot] : FLAGSTAT_scalar's 32 counters over {f(j) : pass(j) && sel(j), offsets[i] <= j < offsets[i+1]}
 *   selected[i]        : the number of j in segment i with pass(j) && sel(j)
 *   high[i]            : OR of (element & ~0xFFFF), taken as unsigned, over the SELECTED elements ONLY of segment i and of no
 *                        other, PASSING OR NOT -- FLAGSTATS_hip_device_wide_filter_where's meaning per segment, both parents'
 *                        rules at once: the filter never restricts the mask (it sees the low 16 bits only), the selection always
 *                        does (the value of a null slot is unspecified and must not make high[i] != 0)
 * Garbage in a null slot, an unselected element, an element of a neighbouring segment or of a gap, elements before offsets[0] and
 * after offsets[nseg] and the bytes around the array enter no counter, no count and no mask; empty segments read 0.  Only bytes
 * of `sel` and of `mapq` that hold the bit or byte of an element of [0, n) and only dwords of elements of [0, n) are ever read.
 * `selected` / `d_selected` and `high` / `d_high` may each be NULL: that value is not reported.
 * require & exclude != 0 is legal and counts nothing: nothing is launched and NOTHING IS READ, so in the store form rows, counts
 * and masks are 0 and in the += form they are untouched -- `high` then says nothing about the column.
 * `flags`: bit 0 = store (every slot of every row, every selected[i] and every high[i] written) instead of out += counters,
 * selected += count, high |= mask; bit 1 = superset (slots 0 / 16 = primary paired reads among the counted, slot 9 =
 * selected[i] minus slot 25).  nseg == 0 succeeds and touches nothing.
 * DEVICE offsets are clamped to [0, n] and not checked for order, as documented for FLAGSTATS_hip_device_u16_segments: malformed
 * offsets give undefined rows, counts and masks, never an access outside the array, the columns or the outputs.  HOST offsets are
 * validated first (non-decreasing, offsets[nseg] <= n); on failure the outputs are left untouched.
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, outputs untouched, nothing launched): elem_bytes other than 4 or 8 (2:
 * use the u16 segments_filter_where entries), sel_bits other than 1 or 8, flag bits other than 0 and 1, require or exclude above
 * 0xFFFF, min_mapq above 255, NULL offsets or out with nseg > 0, an nseg whose counters are not a size, a NULL array or selection
 * with n > 0, a NULL mapq with min_mapq > 0 and n > 0, an array pointer not aligned to elem_bytes, an n with n * elem_bytes not a
 * size or too large for a wave's uint32 totals, a sel_offset + n that is no index; for the device form also a d_out, d_selected
 * or d_high that is not plain device memory, host memory for d_array, d_mapq, d_sel or d_offsets, pointers on different devices,
 * a stream of another device and an allocation shorter than the call needs (d_array: n * elem_bytes bytes, d_mapq: n bytes when
 * min_mapq > 0, d_sel: from d_sel up to the last byte that holds an element's bit or byte, d_offsets: (nseg + 1) * 8, d_out:
 * nseg * 256, d_selected: nseg * 8, d_high: nseg * 8). */
/* DEVICE array, MAPQ column, selection and offsets, DEVICE d_out[nseg][32], d_selected[nseg] and d_high[nseg] (uint64);
 * asynchronous on `stream`: ONE kernel (the store form puts one zeroing per pointer in front of it; one in all when d_selected ==
 * d_out + nseg * 32 and d_high == d_selected + nseg), no workspace, nothing synchronised, so a captured launch holds no pointer of
 * the library's (make one plain call before capturing).  Adds and ORs are atomic: launches on several streams may share the three
 * in the += form. */
int FLAGSTATS_hip_device_wide_segments_filter_where(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* d_offsets,
                                                    uint64_t nseg, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                                    uint32_t min_mapq, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                                    uint64_t* d_out, uint64_t* d_selected, uint64_t* d_high, int flags, void* stream);
/* DEVICE array, MAPQ column and selection, HOST offsets, HOST out[nseg][32], selected[nseg] and high[nseg]; synchronous */
int FLAGSTATS_hip_device_wide_segments_filter_where_sync(const void* d_array, uint64_t n, int elem_bytes, const uint64_t* offsets,
                                                         uint64_t nseg, uint32_t require, uint32_t exclude, const uint8_t* d_mapq,
                                                         uint32_t min_mapq, const void* d_sel, uint64_t sel_offset, int sel_bits,
                                                         uint64_t* out, uint64_t* selected, uint64_t* high, int flags);
/* HOST array, MAPQ column, selection and offsets, HOST out[nseg][32], selected[nseg] and high[nseg]; synchronous.  Only
 * [offsets[0], offsets[nseg]) of the array and of the column and the selection bytes that cover it cross the bus, in the engine's
 * chunks (knob "chunk_flags": chunk_flags * 2 bytes of elements each), each chunk's slices of the column and of the selection
 * behind its elements (a bitmap slice from the byte that holds the chunk's first bit); a segment that spans chunks is summed and
 * ORed on the device. */
int FLAGSTATS_hip_wide_x64_segments_filter_where(const void* array, uint64_t n, int elem_bytes, const uint64_t* offsets, uint64_t nseg,
                                                 uint32_t require, uint32_t exclude, const uint8_t* mapq, uint32_t min_mapq,
                                                 const void* sel, uint64_t sel_offset, int sel_bits, uint64_t* out,
                                                 uint64_t* selected, uint64_t* high, int flags);

/* 64-bit positional popcount in this library's convention: out[16] += bit counts (host array / device array) */
int FLAGSTATS_hip_pospopcnt_u16_x64(const uint16_t* array, uint64_t n, uint64_t* out);
int FLAGSTATS_hip_device_pospopcnt_u16(const uint16_t* d_array, uint64_t n, uint64_t* d_out, void* stream);

/* ================= context =================
 * State: one engine per device (streams, staging, workspaces), created on first use.  Entry points that take a DEVICE
 * pointer run on the device that pointer lives on; entry points without one use the default device (FLAGSTATS_hip_init,
 * else env FLAGSTATS_HIP_DEVICE, else 0). */
int FLAGSTATS_hip_available(void);          /* 1 if a gfx950-capable device can be used */
int FLAGSTATS_hip_device_count(void);       /* HIP devices visible to this process (0 if none) */
int FLAGSTATS_hip_init(int device);         /* optional: selects the default device (lazily FLAGSTATS_HIP_DEVICE or 0) */
void FLAGSTATS_hip_shutdown(void);          /* releases every engine (close sessions and contexts first) */
const char* FLAGSTATS_hip_last_error(void); /* text of the last failure on this thread ("" if none) */
int FLAGSTATS_hip_device_id(void);          /* device the context is bound to, -1 before init */
int FLAGSTATS_hip_compute_units(void);      /* CU count of that device, -1 before init */
/* fork(): unlike the reference's pure function (libflagstats.h:3024-3070) this library is an engine -- a HIP context,
 * streams, helper threads -- that does not exist in a child fork()ed after its first use.  Every entry point refuses such a
 * child before touching any GPU state: a message naming the fork on stderr and in FLAGSTATS_hip_last_error, a non-zero /
 * NULL return (the reference-shaped entry points then abort() per "on_error"); release-type entries (shutdown, *_free,
 * *_destroy, stream_close) do nothing there.  Use the "spawn" start method, or make the first call after the fork.
 * FLAGSTATS_hip_forked: 1 in such a child, else 0 (touches nothing, claims nothing). */
int FLAGSTATS_hip_forked(void);

/* explicit contexts: a private engine (own streams, staging and workspaces) on `device`; several may exist per device and
 * are fully independent of each other and of the default engines -- one per caller thread gives concurrent host-array calls. */
typedef struct FLAGSTATS_hip_ctx FLAGSTATS_hip_ctx;
FLAGSTATS_hip_ctx* FLAGSTATS_hip_ctx_create(int device);   /* device < 0: the default device; NULL on failure */
void FLAGSTATS_hip_ctx_destroy(FLAGSTATS_hip_ctx* ctx);
int FLAGSTATS_hip_ctx_device(const FLAGSTATS_hip_ctx* ctx);
int FLAGSTATS_hip_ctx_u16_x64(FLAGSTATS_hip_ctx* ctx, const uint16_t* array, uint64_t n, uint64_t* out); /* as FLAGSTATS_u16_x64 */
int FLAGSTATS_hip_ctx_device_u16_sync(FLAGSTATS_hip_ctx* ctx, const uint16_t* d_array, uint64_t n, uint64_t* out);

/* Knobs (also env FLAGSTATS_HIP_<KEY IN CAPITALS>); the ones a caller may want -- the full list, with what each was measured
 * to do, is in libflagstats_hip_probe.h:
 *   "on_error"      reference-shaped entry points on failure: 1 abort() after the message (default), 0 return non-zero
 *   "chunk_flags"   flags per H2D chunk of the host-pointer entries (default 32 Mi = 64 MiB)
 *   "small_flags"   host-pointer calls up to this many flags take the latency path (default 1 Mi; 0 = always stage)
 *   "lz4_decoder" / "zstd_decoder"   block files: 0 host threads, 1 on the GPU, 2 (default) by size
 *   "numa"          1 (default): pinned buffers and worker threads are placed on the GPU's host NUMA node
 * Returns 0 on success. */
int FLAGSTATS_hip_set(const char* key, uint64_t value);
uint64_t FLAGSTATS_hip_get(const char* key);

/* ================= multi-GPU: contiguous shards, counters summed; no other exchange =================
 * rank's shard of n flags over `world` ranks: [begin, end), remainder to the last rank */
void FLAGSTATS_hip_shard_range(uint64_t n, int rank, int world, uint64_t* begin, uint64_t* end);
/* one process, `ndev` devices, HOST array: shard i goes through a private engine on devices[i] (NULL = devices 0..ndev-1; a
 * device may repeat) over that device's PCIe link, one host thread per shard; out[32] += the host-side sum. */
int FLAGSTATS_hip_multi_u16_x64(const uint16_t* array, uint64_t n, const int* devices, int ndev, uint64_t* out);
/* one process, DEVICE-resident shards (d_arrays[i] holds n[i] flags on whichever device it was allocated on): counted where
 * they live, all devices concurrently; out[32] += host-side sum. */
int FLAGSTATS_hip_multi_device_u16(const uint16_t* const* d_arrays, const uint64_t* n, int nshards, uint64_t* out);
/* one process per device (RCCL over xGMI; librccl.so.1 is bound at first use, env FLAGSTATS_HIP_RCCL overrides its path).
 * Communicators travel as void* (an ncclComm_t made here or by the caller):
 *   rank 0: FLAGSTATS_hip_comm_unique_id(id) -> ship the 128 bytes to every rank by any means
 *   all:    comm = FLAGSTATS_hip_comm_init_rank(id, nranks, rank, device)
 *   query:  FLAGSTATS_hip_device_u16_allreduce(d_shard, n, d_out, comm, stream)
 *           = K1 + K2 storing this shard's counters into d_out[32], then ONE
 *             ncclAllReduce(d_out, d_out, 32, ncclUint64, ncclSum) on the same stream. */
int FLAGSTATS_hip_comm_unique_id(void* id128);
void* FLAGSTATS_hip_comm_init_rank(const void* id128, int nranks, int rank, int device); /* NULL on failure */
int FLAGSTATS_hip_comm_destroy(void* comm);
int FLAGSTATS_hip_comm_count(void* comm);   /* ranks RCCL sees in the communicator (ncclCommCount); < 0 on failure */
/* which RCCL is bound: path of the shared object that holds ncclAllReduce (dladdr; "" if unknown) and ncclGetVersion's number
 * (-1 if unknown); binds RCCL if nothing has yet; non-zero when RCCL cannot be loaded */
int FLAGSTATS_hip_comm_library(char* path, uint64_t cap, int* version);
int FLAGSTATS_hip_allreduce_counters(uint64_t* d_counters, void* comm, void* stream);
int FLAGSTATS_hip_device_u16_allreduce(const uint16_t* d_array, uint64_t n, uint64_t* d_out, void* comm, void* stream);
/* the same query with the collective OFF the launch stream: K1 + K2 (store) on `stream`, the all-reduce on `comm_stream`,
 * ordered behind the kernels by an event without timing, so it overlaps whatever `stream` runs next.  d_out may be
 * rewritten once `comm_stream` has passed the all-reduce: FLAGSTATS_hip_stream_wait_stream(stream, comm_stream, device) makes
 * `stream` wait on the device (cheap, e.g. once per ring of counter buffers); a host sync of comm_stream works too. */
int FLAGSTATS_hip_device_u16_allreduce_overlapped(const uint16_t* d_array, uint64_t n, uint64_t* d_out, void* comm, void* stream,
                                                  void* comm_stream);
int FLAGSTATS_hip_stream_wait_stream(void* waiter, void* on, int device);

/* ================= memory helpers for callers without a HIP runtime of their own ================= */
void* FLAGSTATS_hip_host_alloc(size_t bytes);   /* pinned host memory */
void FLAGSTATS_hip_host_free(void* p);
void* FLAGSTATS_hip_device_alloc(size_t bytes); /* device memory on the default device */
void* FLAGSTATS_hip_device_alloc_on(int device, size_t bytes);
void FLAGSTATS_hip_device_free(void* p);
int FLAGSTATS_hip_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int FLAGSTATS_hip_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
int FLAGSTATS_hip_synchronize(void);

/* ================= inputs =================
 * synthetic inputs on device (counterpart of benchmark/generate.cpp:8-14): d_array[k] = flag(kind, seed, mask,
 * first_index + k), k in [0, n).  kind 0 uniform (& mask), 1 NA12878-like (mask bit0 = +eps), 2 ramp.  Asynchronous. */
int FLAGSTATS_hip_generate_u16(uint16_t* d_array, uint64_t n, int kind, uint64_t seed, uint32_t mask,
                               uint64_t first_index, void* stream);
/* FLAG text -> uint16 array (counterpart of benchmark/utility.cpp:9-16, the reference's `samtools view FILE | cut -f 2 |
 * utility > FLAGS.bin` step): one decimal FLAG per line, std::getline + atoi rules (a final unterminated line counts; an
 * empty or non-numeric line is 0; "99\r" is 99; the int is truncated to 16 bits).  Host code.  Returns the number of values
 * written to out[0..cap), or < 0 if `cap` is too small; FLAGSTATS_text_count_lines gives the exact count beforehand. */
int64_t FLAGSTATS_text_to_u16(const char* text, uint64_t len, uint16_t* out, uint64_t cap);
uint64_t FLAGSTATS_text_count_lines(const char* text, uint64_t len);

/* ================= block files: the reference's `bench decompress -d` / `-D` callers =================
 * File format written by benchmark/flagstats.cpp:119-138 and read at :311-316: a sequence of
 *   int32 uncompressed_size, int32 compressed_size, <raw LZ4 block>   (little-endian; not LZ4 frames).
 * The LZ4 path decodes blocks on `threads` host threads (<= 0: up to 24) into pinned chunk buffers, overlapped with the H2D
 * copy and K1 of earlier chunks -- or, for large files (knob "lz4_decoder"), sends the file over PCIe as it is and decodes the
 * blocks on the GPU; out[32] += counters of every flag (a block contributes uncompressed_size >> 1 flags, as
 * benchmark/flagstats.cpp:323). */
typedef struct FLAGSTATS_blockfile_stats {
    uint64_t n_flags, n_blocks, compressed_bytes, uncompressed_bytes;
    double wall_s, index_s, setup_s, decode_cpu_s; /* setup_s: index + buffers; decode_cpu_s: sum over threads */
    double wait_decode_s, wait_copy_s;             /* orchestrator: waiting for decoders / for H2D copies */
    int32_t threads, chunks;
    int32_t gpu_decode, reserved;                  /* 1: the blocks were decoded on the GPU: threads = parallel file readers
                                                      (0 in image mode), chunks = pieces copied, decode_cpu_s = 0,
                                                      wait_copy_s = copies, wait_decode_s = decode left exposed after the last copy */
} FLAGSTATS_blockfile_stats;
int FLAGSTATS_hip_blockfile_lz4(const char* path, int threads, uint64_t* out, FLAGSTATS_blockfile_stats* stats);
int FLAGSTATS_hip_blockimage_lz4(const void* image, uint64_t bytes, int threads, uint64_t* out,
                                 FLAGSTATS_blockfile_stats* stats); /* same, file already in memory */
/* Zstandard block files (.zst: benchmark/flagstats.cpp:192-226 writer, :636-682 reader): same block header, payload = one
 * Zstandard frame.  libzstd stays the third-party dependency it is in the reference; it is resolved at run time
 * (libzstd.so.1, or env FLAGSTATS_HIP_ZSTD_LIB) when the host has to decode a .zst file, and the call fails loudly without
 * it.  Large files are decoded on the GPU instead (knob "zstd_decoder"; stats->gpu_decode = 1), which needs libzstd only for
 * files with frames the GPU decoder does not take. */
int FLAGSTATS_hip_blockfile_zstd(const char* path, int threads, uint64_t* out, FLAGSTATS_blockfile_stats* stats);
int FLAGSTATS_hip_blockimage_zstd(const void* image, uint64_t bytes, int threads, uint64_t* out,
                                  FLAGSTATS_blockfile_stats* stats);
int FLAGSTATS_hip_zstd_available(void);   /* 1 if libzstd could be loaded */
/* codec by extension as the reference's check_file_extension (benchmark/flagstats.cpp:828-839): .lz4 | .zst */
int FLAGSTATS_hip_blockfile(const char* path, int threads, uint64_t* out, FLAGSTATS_blockfile_stats* stats);
/* raw uint16 file (benchmark/flagstats.cpp:415-468, `-D`): the same threaded pipeline without a codec -- workers pread
 * 1 MiB slices straight into the pinned chunks (env FLAGSTATS_HIP_RAW_IO=mmap: mmap + FLAGSTATS_u16_x64) */
int FLAGSTATS_hip_file_raw(const char* path, uint64_t* out, FLAGSTATS_blockfile_stats* stats);
/* A host array in ordinary (pageable) memory through the same chunk pipeline: `threads` workers (0 = automatic) copy 1 MiB
 * slices into the engine's page-locked chunks, which cross PCIe behind them; out[32] += counters.  FLAGSTATS_u16 /
 * FLAGSTATS_u16_x64 do this by themselves for pageable arrays of at least `staged_min_flags` flags (default 2^27); exported
 * for callers that know their arrays are in small pages and want it from 64 MiB (profiles/r05/pageable_c.log). */
int FLAGSTATS_hip_host_staged_u16(const uint16_t* array, uint64_t n, int threads, uint64_t* out, FLAGSTATS_blockfile_stats* stats);
/* the file entries with SUPERSET counters (slots 0 / 16 = n_pair_all, slot 9 = pass-QC reads): what the samtools report of
 * `bench decompress -s` (block file) / `-S` (raw file) needs, benchmark/flagstats.cpp:577-588 */
int FLAGSTATS_hip_blockfile_superset(const char* path, int threads, uint64_t* out, FLAGSTATS_blockfile_stats* stats);
int FLAGSTATS_hip_file_raw_superset(const char* path, uint64_t* out, FLAGSTATS_blockfile_stats* stats);
/* the host LZ4 *block* decoder of the pipeline above (replaces the reference's call to liblz4's LZ4_decompress_safe,
 * benchmark/flagstats.cpp:316): returns decoded bytes, < 0 on malformed input */
int64_t FLAGSTATS_lz4_block_decode(const void* src, uint64_t srclen, void* dst, uint64_t dstcap);

/* ================= streaming sessions =================
 * For callers that keep their own per-block loop and accumulate into one counter array read after the loop, as
 * benchmark/flagstats.cpp:304,311-342 does.  The caller decodes straight into pinned memory handed out by `acquire` (zero
 * copy) and `commit`s; copies and kernels run behind it; `finish` waits and adds the counters of everything committed since
 * the last finish.
 *   FLAGSTATS_hip_stream* s = FLAGSTATS_hip_stream_open();
 *   for each block: uint16_t* p = FLAGSTATS_hip_stream_acquire(s, N);  decode N flags into p;
 *                   FLAGSTATS_hip_stream_commit(s, N);
 *   FLAGSTATS_hip_stream_finish(s, counters);  FLAGSTATS_hip_stream_close(s);
 * `push` = acquire + memcpy + commit for callers that cannot decode in place.  A block may not exceed the chunk size (knob
 * "chunk_flags").  The pointer from `acquire` is valid until `commit`. */
typedef struct FLAGSTATS_hip_stream FLAGSTATS_hip_stream;
FLAGSTATS_hip_stream* FLAGSTATS_hip_stream_open(void);                       /* NULL on failure */
uint16_t* FLAGSTATS_hip_stream_acquire(FLAGSTATS_hip_stream* s, uint64_t n); /* room for n flags; NULL on failure */
int FLAGSTATS_hip_stream_commit(FLAGSTATS_hip_stream* s, uint64_t n);        /* n <= the acquired size */
int FLAGSTATS_hip_stream_push(FLAGSTATS_hip_stream* s, const uint16_t* array, uint64_t n);
int FLAGSTATS_hip_stream_finish(FLAGSTATS_hip_stream* s, uint64_t* out);     /* out[32] += counters; session reusable */
uint64_t FLAGSTATS_hip_stream_flags(const FLAGSTATS_hip_stream* s);          /* flags committed since the last finish */
void FLAGSTATS_hip_stream_close(FLAGSTATS_hip_stream* s);

/* ================= filtered segments, the whole predicate: -f / -F / --rf / -G / -q per segment of a uint16 column =================
 * Per-contig, per-sample or per-block tables of the reads that pass `-F 0x904 --rf 0x50 -q 30`: the filtered segmented entries
 * with the two options of `samtools view` that no require / exclude pair can express once they name two bits, --rf include_any
 * (AT LEAST ONE of these bits) and -G exclude_all (not ALL of these bits), in one launch.  uint16 arrays only: per segment of a
 * 4-byte or 8-byte column, and together with a bitmap or byte mask, the two options are not built.
 *   pass(j) = (array[j] & require) == require && (array[j] & exclude) == 0
 *             && (include_any == 0 || (array[j] & include_any) != 0)
 *             && (exclude_all == 0 || (array[j] & exclude_all) != exclude_all)
 *             && (min_mapq == 0 || mapq[j] >= min_mapq)
 * include_any == 0 and exclude_all == 0 switch those tests off; with both 0 the entries are the filtered segmented entries.
 * Everything else is the union of the two parents' contracts.  Segment i is [offsets[i], offsets[i+1]) under the contract of the
 * segmented entries; row i of out[nseg][32] holds FLAGSTAT_scalar's counters over {array[j] : j in segment i, pass(j)}, and
 * selected[i] (nseg uint64; the pointer may be NULL: nothing is reported) the number of such j.  Flags outside every segment
 * count nowhere.  min_mapq == 0 reads no byte of `mapq`, which may then be NULL; otherwise only bytes of elements in [0, n) are
 * read.
 * `flags`: bit 0 = store (rows and selected[0 .. nseg) are zeroed in front, every slot of every row is written, empty segments
 * read 0) instead of +=; bit 1 = superset (slots 0 / 16 = primary paired reads among those that pass, slot 9 = selected[i]
 * minus slot 25).  nseg == 0 succeeds and touches nothing.
 * The four masks are first reduced exactly on the host (a single --rf bit is a required bit, a single -G bit an excluded one, a
 * bit that -f / -F already decide leaves --rf / -G), and by what is left a call is one of three things:
 *   nothing can pass (require & exclude != 0, every --rf bit excluded, every -G bit required): nothing is launched and no
 *       element, MAPQ byte or offset is read (the host form moves nothing); the store form still zeroes rows and counts, the +=
 *       form leaves both as they are
 *   a plain require / exclude pair is left: the launch is the filtered segmented entries' kernel, at its speed
 *   a residue of two or more free bits in --rf or -G is left: one kernel of its own (fsk::flagstat_segments_filter_rf)
 * Refused (non-zero, message in FLAGSTATS_hip_last_error, out and selected untouched, nothing launched): what the filtered
 * segmented entries refuse, and include_any or exclude_all above 0xFFFF (asked after require / exclude / min_mapq and before
 * `flags`).  Device offsets are not checked (that would synchronise): every offset the kernel reads is clamped to [0, n], so
 * malformed offsets give undefined counters and never an access outside the array, the column, the rows or the counts. */
/* DEVICE array, column and offsets, DEVICE d_out[nseg][32] and d_selected[nseg] (uint64); asynchronous on `stream`: ONE kernel
 * (the store form puts one memset per pointer in front of it), no workspace, nothing synchronised; may be captured into a graph.
 * Adds are atomic: launches on several streams may share d_out and d_selected in the += form. */
int FLAGSTATS_hip_device_u16_segments_filter_rf(const uint16_t* d_array, uint64_t n, const uint64_t* d_offsets, uint64_t nseg,
                                                uint32_t require, uint32_t exclude, uint32_t include_any, uint32_t exclude_all,
                                                const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* d_out, uint64_t* d_selected,
                                                int flags, void* stream);
/* DEVICE array and column, HOST offsets, HOST out[nseg][32] and selected[nseg]; synchronous */
int FLAGSTATS_hip_device_u16_segments_filter_rf_sync(const uint16_t* d_array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                                     uint32_t require, uint32_t exclude, uint32_t include_any, uint32_t exclude_all,
                                                     const uint8_t* d_mapq, uint32_t min_mapq, uint64_t* out, uint64_t* selected,
                                                     int flags);
/* HOST array, column and offsets, HOST out[nseg][32] and selected[nseg]; synchronous.  Only [offsets[0], offsets[nseg]) of array
 * and column crosses the bus, in the engine's chunks (knob "chunk_flags"), each chunk's slice of the column behind its flags; a
 * segment that spans chunks is summed on the device. */
int FLAGSTATS_hip_u16_x64_segments_filter_rf(const uint16_t* array, uint64_t n, const uint64_t* offsets, uint64_t nseg,
                                             uint32_t require, uint32_t exclude, uint32_t include_any, uint32_t exclude_all,
                                             const uint8_t* mapq, uint32_t min_mapq, uint64_t* out, uint64_t* selected, int flags);

#ifdef __cplusplus
}
#endif
#endif
