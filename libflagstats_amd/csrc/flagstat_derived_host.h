// flagstat_derived_host.h -- internal: the host code that the kernels derived from K1 share.  All fifteen derived units use it:
// the seven flat ones (flagstat_{wide,where,filter,filter_where,wide_filter,wide_where,wide_filter_where}.hip) directly, the
// eight segmented ones (flagstat_segments*.hip) through flagstat_segments_shared.h; flagstat_filter_rf.hip, the filtered unit's
// --rf / -G form, uses it as that unit does.  It holds the launcher's step split and
// store-form memset, the rules of an entry's arguments with the text of their refusals (one function per rule; a unit's *_args
// composes them in its own order), a call's inputs table, the device row of a synchronous call (32 counters and one trailing
// word, or two: kRowWords / kRowWords2), and the bodies of the three entry forms of the flat units -- on the caller's stream,
// synchronous over device memory, chunked over host memory.  What differs between the kernels arrives as arguments and
// callables: the hints of their refusals, how a chunk's inputs are copied and launched.  A HIP call that a callable makes goes
// through FS_HIP_TRY there, so the text of its failure names the caller's own expression.
// (Product library only: the entries check allocation extents, which the host-stub build does not have.)
#ifndef FLAGSTAT_DERIVED_HOST_H_
#define FLAGSTAT_DERIVED_HOST_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <mutex>
#include <optional>

#include "flagstat_engine.h"
#include "flagstat_kernels.h"
#include "flagstat_where.h"

namespace fsdrv {

constexpr int kStepBytes = fsk::kVecPerStep * 16;   // 32 KiB

// ------------------------------------------------------------------ launchers
// Host-side geometry: everything a kernel assumes is derived here from (address, n, W), W = elem_bytes in {2, 4, 8}.  The array
// is addressed on the 16-byte grid of its aligned-down base: geo[0..5] = lo, hi (the caller's elements occupy positions [lo, hi)
// of the grid of W-byte elements), nsteps, fast_begin, fast_end (steps whose vectors are all fully inside [lo, hi)) and the
// grid, at most one workgroup per step.  n == 0: all zero.  tests/steps_oracle.StepSplit(addr % 16, n * W / 2, grid) mirrors it.
inline hipError_t step_split(uint64_t address, uint64_t n, int elem_bytes, uint32_t grid, uint64_t* geo)
{
    if ((elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8) || grid == 0 || geo == nullptr) return hipErrorInvalidValue;
    const uint64_t W = static_cast<uint64_t>(elem_bytes);
    const uint64_t addr = address;
    if (addr & (W - 1)) return hipErrorInvalidValue;
    for (int i = 0; i < 6; ++i) geo[i] = 0;
    if (n == 0) return hipSuccess;
    if (n > (~0ull - 64) / W) return hipErrorInvalidValue;  // n * W must be a size
    const uint64_t base = addr & ~static_cast<uint64_t>(15);
    const uint64_t epv = 16 / W;                            // elements per 16-byte vector
    const uint64_t lo = (addr - base) / W, hi = lo + n;
    const uint64_t nvec = (hi + epv - 1) / epv;
    const uint64_t vps = fsk::kVecPerStep;
    const uint64_t nsteps = (nvec + vps - 1) / vps;
    // steps whose vectors are all fully inside [lo, hi)
    uint64_t fast_begin = (lo == 0) ? 0 : 1;
    uint64_t fast_end = (hi / epv) / vps;
    if (fast_end < fast_begin) fast_end = fast_begin;
    if (static_cast<uint64_t>(grid) > nsteps) grid = static_cast<uint32_t>(nsteps);
    // a wave's totals are uint32: a workgroup pushes at most ceil(nsteps / grid) + 2 steps (its share and both edge steps), each
    // wave a quarter of every step
    const uint64_t wave_elems_per_step = kStepBytes / W / (fsk::kThreads / 64);
    if (nsteps / grid + 3 >= (1ull << 32) / wave_elems_per_step) return hipErrorInvalidValue;
    geo[0] = lo;
    geo[1] = hi;
    geo[2] = nsteps;
    geo[3] = fast_begin;
    geo[4] = fast_end;
    geo[5] = grid;
    return hipSuccess;
}

// the store form's zeroes in front of a launch: the counters and the optional 33rd word (mask, selected count), in one memset
// where they are one allocation's 33 words (fsk_zero_words: hipMemsetAsync, or a kernel while the stream is being captured)
inline hipError_t zero_counters(uint64_t* d_out32, uint64_t* d_word, hipStream_t stream)
{
    const bool together = d_word == d_out32 + 32;
    hipError_t e = fsk_zero_words(d_out32, together ? 33 : 32, stream);
    if (e == hipSuccess && d_word && !together) e = fsk_zero_words(d_word, 1, stream);
    return e;
}

// the same with two trailing words (selected count, then mask): one memset where they are one allocation's 34 words
inline hipError_t zero_counters(uint64_t* d_out32, uint64_t* d_word, uint64_t* d_word2, hipStream_t stream)
{
    if (d_word != d_out32 + 32 || d_word2 != d_out32 + 33) {
        const hipError_t e = zero_counters(d_out32, d_word, stream);
        return e == hipSuccess && d_word2 ? fsk_zero_words(d_word2, 1, stream) : e;
    }
    return fsk_zero_words(d_out32, 34, stream);
}

// ------------------------------------------------------------------ C entry points
constexpr int kRowWords = 33;    // counters[32] + one trailing word
constexpr int kRowWords2 = 34;   // counters[32] + two: a count (added), then a mask (ORed)

// device counters[32] + the trailing words of one synchronous call; `what` names the allocation in the text of a failure
struct Row {
    uint64_t* d = nullptr;
    ~Row()
    {
        if (d) (void)hipFree(d);
    }
    int alloc(const char* what, int words = kRowWords)
    {
        const hipError_t e = hipMalloc(&d, static_cast<size_t>(words) * sizeof(uint64_t));
        if (e != hipSuccess) {
            d = nullptr;
            return fsint::fail_hip(what, e);
        }
        return 0;
    }
};

// how the 33rd word of a result combines in the accumulate form: a count is added, a mask is ORed
enum WordOp { kWordAdd, kWordOr };

// a call's result into the caller's host words: stored (flags bit 0) or accumulated
inline void apply(uint64_t* out, uint64_t* word, const uint64_t (&got)[33], int flags, WordOp op)
{
    if (flags & 1) {
        for (int i = 0; i < 32; ++i) out[i] = got[i];
        if (word) *word = got[32];
    } else {
        for (int i = 0; i < 32; ++i) out[i] += got[i];
        if (word) *word = op == kWordOr ? (*word | got[32]) : *word + got[32];
    }
}

// the same with two trailing words: the count is added, the mask is ORed
inline void apply(uint64_t* out, uint64_t* count, uint64_t* mask, const uint64_t (&got)[kRowWords2], int flags)
{
    if (flags & 1) {
        for (int i = 0; i < 32; ++i) out[i] = got[i];
        if (count) *count = got[32];
        if (mask) *mask = got[33];
    } else {
        for (int i = 0; i < 32; ++i) out[i] += got[i];
        if (count) *count += got[32];
        if (mask) *mask |= got[33];
    }
}

// the result of a call over no elements
inline void store_nothing(uint64_t* out, uint64_t* word, int flags)
{
    if (flags & 1) {
        for (int i = 0; i < 32; ++i) out[i] = 0;
        if (word) *word = 0;
    }
}

inline void store_nothing(uint64_t* out, uint64_t* word, uint64_t* word2, int flags)
{
    store_nothing(out, word, flags);
    if ((flags & 1) && word2) *word2 = 0;
}

// ------------------------------------------------------------------ argument rules
// What an entry refuses before it touches the GPU, one function per rule and each the only home of its text.  A unit's *_args is
// refused(rule || rule || ...) in that unit's order: the first broken rule is the one reported and no later one is asked.  The
// array's rules are two functions because the MAPQ and selection pointers are asked for between them.
using fsint::fail_text;

// the return value of a unit's *_args: fail_text's -1 when some rule of the chain refused
inline int refused(bool any) { return any ? -1 : 0; }

// `u16_hint`: the unit's own text for elem_bytes == 2, naming the 16-bit entries that take such an array
inline int check_elem_bytes(int elem_bytes, const char* u16_hint)
{
    if (elem_bytes == 2) return fail_text(u16_hint);
    if (elem_bytes != 4 && elem_bytes != 8) return fail_text("elem_bytes must be 4 or 8");
    return 0;
}

inline int check_predicate(uint32_t require, uint32_t exclude, uint32_t min_mapq)
{
    if (require > 0xFFFFu) return fail_text("require must be a 16-bit FLAG mask (at most 0xFFFF)");
    if (exclude > 0xFFFFu) return fail_text("exclude must be a 16-bit FLAG mask (at most 0xFFFF)");
    if (min_mapq > 255u) return fail_text("min_mapq must be at most 255 (MAPQ is one byte)");
    return 0;
}

// the two further masks of samtools' view predicate (--rf, -G: flagstat_filter_rf.hip), in check_predicate's words
inline int check_predicate_rf(uint32_t include_any, uint32_t exclude_all)
{
    const bool any = include_any > 0xFFFFu;
    if (!any && exclude_all <= 0xFFFFu) return 0;
    char buf[96];
    std::snprintf(buf, sizeof buf, "%s must be a 16-bit FLAG mask (at most 0x%X)", any ? "include_any" : "exclude_all", 0xFFFFu);
    return fail_text(buf);
}

inline int check_sel_bits(int sel_bits)
{
    if (sel_bits != 1 && sel_bits != 8) return fail_text("sel_bits must be 1 (an LSB-first bitmap) or 8 (one byte per element)");
    return 0;
}

inline int check_flags(int flags)
{
    return (flags & ~3) ? fail_text("flags: bit 0 store, bit 1 superset; no other bits") : 0;
}

inline int check_array_given(const void* array, uint64_t n)
{
    return (n && !array) ? fail_text("NULL array with n > 0") : 0;
}

inline int check_mapq_given(const void* mapq, uint64_t n, uint32_t min_mapq)
{
    return (n && min_mapq && !mapq) ? fail_text("NULL mapq with min_mapq > 0 and n > 0") : 0;
}

// `text`: a unit's own wording where it names the entries that take no selection
inline int check_sel_given(const void* sel, uint64_t n, const char* text = "NULL selection with n > 0")
{
    return (n && !sel) ? fail_text(text) : 0;
}

// an array of elements of W bytes (2: the uint16 units, in their words; 4 or 8) is aligned
inline int check_array_aligned(const void* array, int W)
{
    if ((reinterpret_cast<uintptr_t>(array) & static_cast<uintptr_t>(W - 1)) == 0) return 0;
    return fail_text(W == 2   ? "array must be 2-byte aligned"
                     : W == 4 ? "array must be 4-byte aligned (elem_bytes 4)"
                              : "array must be 8-byte aligned (elem_bytes 8)");
}

// it is aligned and its n * W bytes are a size
inline int check_array_layout(const void* array, uint64_t n, int W)
{
    if (check_array_aligned(array, W)) return -1;
    if (n > (~0ull - 64) / static_cast<uint64_t>(W)) return fail_text(W == 2 ? "n * 2 is not a size" : "n * elem_bytes is not a size");
    return 0;
}

inline int check_sel_range(uint64_t sel_offset, uint64_t n)
{
    return sel_offset > ~0ull - 64 - n ? fail_text("sel_offset + n is not an index") : 0;
}

// the counters of a flat entry: needed whenever something is written
inline int check_counters(const void* out, uint64_t n, int flags)
{
    return (!out && (n || (flags & 1))) ? fail_text("NULL counters") : 0;
}

// a wave's totals are uint32: the one thing the step split still refuses once a unit's *_args has passed
inline int fail_wave_totals()
{
    return fail_text("n is too large for this grid: a wave's uint32 totals could overflow (split the array)");
}

inline int step_fits(const void* array, uint64_t n, int elem_bytes, uint32_t grid)
{
    uint64_t geo[6];
    return step_split(reinterpret_cast<uintptr_t>(array), n, elem_bytes, grid, geo) != hipSuccess ? fail_wave_totals() : 0;
}

// the bytes of d_sel a call over the whole array needs, from d_sel itself on (n > 0)
inline uint64_t sel_bytes(uint64_t n, uint64_t sel_offset, int sel_bits)
{
    uint64_t first = 0, bytes = 0;
    where_extent(n, sel_offset, sel_bits, &first, &bytes);
    return first + bytes;
}

// an input array of a call: its pointer, the name the refusals use for it, the bytes the call reads from it on
struct Input {
    const void* p;
    const char* name;
    uint64_t bytes;
};

// the optional 33rd word of a device entry: `why` completes "<name> must be device memory (<why>)"
struct DeviceWord {
    const void* p;
    const char* name;
    const char* why;
};

// a call's inputs in the order its refusals name them: what the unit puts in front (the segmented device entries: the offsets),
// then the columns
struct Inputs {
    Input in[4];
    int count = 0;
    void add(const void* p, const char* name, uint64_t bytes) { in[count++] = Input{p, name, bytes}; }
    // the columns of a call over n elements of W bytes: the array, the selection (sel_bits 0: the unit has none) up to the byte
    // that holds the last element's bit or byte, the MAPQ column (last: it is an input only when min_mapq > 0).  n == 0: none.
    void add_columns(const void* d_array, uint64_t n, uint64_t W, const void* d_sel, uint64_t sel_offset, int sel_bits,
                     const void* d_mapq, uint32_t min_mapq)
    {
        if (n == 0) return;
        add(d_array, "d_array", n * W);
        if (sel_bits) add(d_sel, "d_sel", sel_bytes(n, sel_offset, sel_bits));
        if (min_mapq) add(d_mapq, "d_mapq", n);
    }
};

inline int fail_devices(const char* a, const char* b)
{
    char buf[128];
    std::snprintf(buf, sizeof buf, "%s and %s live on different devices", a, b);
    return fsint::fail_text(buf);
}

// A device entry up to its launch: d_out is plain device memory, so is the 33rd word if there is one, on the same device, as
// is every input; the engine of that device, made current (for as long as this object lives), and the caller's stream on it.
struct DeviceCall {
    fsint::Engine* e = nullptr;
    hipStream_t s = nullptr;
    std::optional<fsint::DeviceGuard> guard;

    int open(const void* d_out, const DeviceWord& word, const Input* in, int inputs, void* stream)
    {
        return open(d_out, &word, 1, in, inputs, stream);
    }

    // the same with `nwords` trailing words, each optional
    int open(const void* d_out, const DeviceWord* words, int nwords, const Input* in, int inputs, void* stream)
    {
        int dev_out = -1, dev = -1;
        bool plain = false;
        int rc = fsint::device_of_pointer(d_out, "d_out", &dev_out, &plain);
        if (rc) return rc;
        if (!plain) return fsint::fail_text("d_out must be device memory (the counters are added with device atomics)");
        for (int k = 0; k < nwords; ++k) {
            const DeviceWord& word = words[k];
            if (!word.p) continue;
            rc = fsint::device_of_pointer(word.p, word.name, &dev, &plain);
            if (rc) return rc;
            if (!plain) {
                char buf[128];
                std::snprintf(buf, sizeof buf, "%s must be device memory (%s)", word.name, word.why);
                return fsint::fail_text(buf);
            }
            if (dev != dev_out) return fail_devices(word.name, "d_out");
        }
        for (int i = 0; i < inputs; ++i) {
            rc = fsint::device_of_pointer(in[i].p, in[i].name, &dev);
            if (rc) return rc;
            if (dev != dev_out) return fail_devices(in[i].name, "d_out");
        }
        e = fsint::engine_for_device(dev_out);
        if (!e) return -1;
        guard.emplace(e->device);
        if (!guard->ok()) return -1;
        s = static_cast<hipStream_t>(stream);
        return fsint::check_stream_device(s, e->device);
    }
};

// every allocation holds what the call touches of it
inline int check_extents(const void* d_out, const DeviceWord* words, int nwords, const Input* in, int inputs)
{
    int rc;
    if ((rc = fsint::check_extent(d_out, 32 * sizeof(uint64_t), "d_out"))) return rc;
    for (int k = 0; k < nwords; ++k)
        if (words[k].p && (rc = fsint::check_extent(words[k].p, sizeof(uint64_t), words[k].name))) return rc;
    for (int i = 0; i < inputs; ++i)
        if ((rc = fsint::check_extent(in[i].p, in[i].bytes, in[i].name))) return rc;
    return 0;
}

inline int check_extents(const void* d_out, const DeviceWord& word, const Input* in, int inputs)
{
    return check_extents(d_out, &word, 1, in, inputs);
}

inline int fits_always(fsint::Engine&) { return 0; }

// The synchronous form over device memory (n > 0, arguments checked): the inputs live on one device (the first one's); under its
// engine's lock `fits(e)` may still refuse, the extents are checked, then `launch(e, row, s)` counts in the store form into a
// row of its own (WORDS uint64) on the engine's first stream and `apply_fn(got)` takes the result to the caller's host words.
template <int WORDS, typename Fits, typename Launch, typename Apply>
int sync_call_row(const Input* in, int inputs, const char* row_what, Fits&& fits, Launch&& launch, Apply&& apply_fn)
{
    int rc, dev = -1, dev_i = -1;
    rc = fsint::device_of_pointer(in[0].p, in[0].name, &dev);
    if (rc) return rc;
    for (int i = 1; i < inputs; ++i) {
        rc = fsint::device_of_pointer(in[i].p, in[i].name, &dev_i);
        if (rc) return rc;
        if (dev_i != dev) return fail_devices(in[i].name, in[0].name);
    }
    fsint::Engine* ep = fsint::engine_for_device(dev);
    if (!ep) return -1;
    fsint::Engine& e = *ep;
    std::lock_guard<std::mutex> lk(e.mu);
    if (fsint::engine_alive(e)) return -1;
    fsint::DeviceGuard guard(e.device);
    if (!guard.ok()) return -1;
    if ((rc = fits(e))) return rc;
    for (int i = 0; i < inputs; ++i)
        if ((rc = fsint::check_extent(in[i].p, in[i].bytes, in[i].name))) return rc;
    Row row;
    if ((rc = row.alloc(row_what, WORDS))) return rc;
    uint64_t got[WORDS];
    hipStream_t s = e.stream[0];
    if ((rc = launch(e, row, s))) return rc;
    FS_HIP_TRY(hipMemcpyAsync(got, row.d, sizeof got, hipMemcpyDeviceToHost, s));
    FS_HIP_TRY(hipStreamSynchronize(s));
    apply_fn(got);
    return 0;
}

// one trailing word, combined by `op`
template <typename Fits, typename Launch>
int sync_call(const Input* in, int inputs, const char* row_what, uint64_t* out, uint64_t* word, int flags, WordOp op, Fits&& fits,
              Launch&& launch)
{
    return sync_call_row<kRowWords>(in, inputs, row_what, fits, launch,
                                    [&](const uint64_t (&got)[kRowWords]) { apply(out, word, got, flags, op); });
}

// two trailing words: a count, then a mask
template <typename Fits, typename Launch>
int sync_call2(const Input* in, int inputs, const char* row_what, uint64_t* out, uint64_t* count, uint64_t* mask, int flags, Fits&& fits,
               Launch&& launch)
{
    return sync_call_row<kRowWords2>(in, inputs, row_what, fits, launch,
                                     [&](const uint64_t (&got)[kRowWords2]) { apply(out, count, mask, got, flags); });
}

// The form over host memory (n > 0, arguments checked): the n elements cross the bus in chunks of `chunk` elements, alternating
// between the default engine's two streams and staging buffers of `slot_flags` uint16 each (the copy of chunk k + 1 overlaps the
// kernel on chunk k).  `chunk_fn(e, row, sl, pos, c)` copies the inputs of elements [pos, pos + c) into e.stage[sl] and launches
// on e.stream[sl]; every chunk's launch adds into the same row (WORDS uint64).  `fits(e)` may refuse before anything is staged;
// `apply_fn(got)` takes the result to the caller's host words.
template <int WORDS, typename Fits, typename Chunk, typename Apply>
int host_call_row(uint64_t n, uint64_t chunk, uint64_t slot_flags, const char* row_what, Fits&& fits, Chunk&& chunk_fn, Apply&& apply_fn)
{
    int rc;
    fsint::Engine* ep = fsint::default_engine();
    if (!ep) return -1;
    fsint::Engine& e = *ep;
    std::lock_guard<std::mutex> lk(e.mu);
    if (fsint::engine_alive(e)) return -1;
    fsint::DeviceGuard guard(e.device);
    if (!guard.ok()) return -1;
    fsint::lz4_gpu_other_use(e);
    Row row;
    if ((rc = row.alloc(row_what, WORDS))) return rc;
    if ((rc = fsint::engine_second(e))) return rc;
    if ((rc = fits(e))) return rc;
    const int slots = n > chunk ? 2 : 1;
    for (int i = 0; i < slots; ++i)
        if ((rc = fsint::stage_reserve(e, i, slot_flags))) return rc;
    hipStream_t s0 = e.stream[0];
    FS_HIP_TRY(hipMemsetAsync(row.d, 0, WORDS * sizeof(uint64_t), s0));
    if (slots == 2 && (rc = fsint::stream_wait_stream(e, e.stream[1], s0))) return rc;
    uint64_t k = 0;
    for (uint64_t pos = 0; pos < n; pos += chunk, ++k) {
        const int sl = static_cast<int>(k % static_cast<uint64_t>(slots));
        const uint64_t c = n - pos < chunk ? n - pos : chunk;
        if ((rc = chunk_fn(e, row, sl, pos, c))) return rc;
    }
    if (slots == 2 && (rc = fsint::stream_wait_stream(e, s0, e.stream[1]))) return rc;
    uint64_t got[WORDS];
    FS_HIP_TRY(hipMemcpyAsync(got, row.d, sizeof got, hipMemcpyDeviceToHost, s0));
    FS_HIP_TRY(hipStreamSynchronize(s0));
    if (slots == 2) FS_HIP_TRY(hipStreamSynchronize(e.stream[1]));
    apply_fn(got);
    return 0;
}

// one trailing word, combined by `op`
template <typename Fits, typename Chunk>
int host_call(uint64_t n, uint64_t chunk, uint64_t slot_flags, const char* row_what, uint64_t* out, uint64_t* word, int flags,
              WordOp op, Fits&& fits, Chunk&& chunk_fn)
{
    return host_call_row<kRowWords>(n, chunk, slot_flags, row_what, fits, chunk_fn,
                                    [&](const uint64_t (&got)[kRowWords]) { apply(out, word, got, flags, op); });
}

// two trailing words: a count, then a mask
template <typename Fits, typename Chunk>
int host_call2(uint64_t n, uint64_t chunk, uint64_t slot_flags, const char* row_what, uint64_t* out, uint64_t* count, uint64_t* mask,
               int flags, Fits&& fits, Chunk&& chunk_fn)
{
    return host_call_row<kRowWords2>(n, chunk, slot_flags, row_what, fits, chunk_fn,
                                     [&](const uint64_t (&got)[kRowWords2]) { apply(out, count, mask, got, flags); });
}

// host streaming chunk in flags (knob "chunk_flags", at least one vector)
inline uint64_t chunk_flags()
{
    const uint64_t c = fsint::knobs().chunk_flags.load();
    return c < 8 ? 8 : c;
}

}  // namespace fsdrv

#endif
