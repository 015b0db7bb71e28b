"""Segmented flagstat of a FLAG column in the integer dtype it arrives in: per segment of an ``int32`` / ``int64`` (or 16-bit)
array, the 32 counters of the elements' low 16 bits and ``high[i]``, the OR over the elements of segment ``i`` of
``element & ~0xFFFF`` (as unsigned) -- per-contig, per-sample or per-block tables straight from a pandas, Arrow or torch column,
with no narrowing copy in front, and a mask that names the segment holding an out-of-range value.

Segments are CSR offsets under the contract of ``segments`` (segment ``i`` is ``values[offsets[i]:offsets[i+1]]``; elements
outside every segment count nowhere and enter no mask; empty segments are allowed and read 0); the masks are those of ``wide``,
one per segment (``high[i] == 0``: every element of the segment was a valid 16-bit FLAG; a negative element sets bit 31 or 63).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .segments import check_offsets, count_segments_torch
from .wide import _check_tensor, _check_values, high_bits_message


def counters_segments_ints(values, offsets, superset: bool = False):
    """``(uint64[nseg, 32] counters, uint64[nseg] high)`` of the segments of a 1-D host array of dtype int16, uint16, int32,
    uint32, int64 or uint64.  16-bit input goes to ``FLAGSTATS_hip_u16_x64_segments`` (``high`` all zero), wider input to
    ``FLAGSTATS_hip_wide_x64_segments``."""
    v = _check_values(values)
    o = check_offsets(offsets, v.size)
    nseg = o.size - 1
    out, high = _checks.segment_results(nseg, 1)
    if not nseg:
        return out, high
    flags = _checks.c_flags(True, superset)
    lib = _lib.lib()
    ptr = v.ctypes.data if v.size else None
    if v.dtype.itemsize == 2:
        _lib.check(lib.FLAGSTATS_hip_u16_x64_segments(ptr, v.size, o.ctypes.data, nseg, out.ctypes.data, flags),
                   "FLAGSTATS_hip_u16_x64_segments")
    else:
        _lib.check(lib.FLAGSTATS_hip_wide_x64_segments(ptr, v.size, v.dtype.itemsize, o.ctypes.data, nseg, out.ctypes.data,
                                                       high.ctypes.data, flags), "FLAGSTATS_hip_wide_x64_segments")
    return out, high


def strict_message(high, offsets) -> str:
    """The text ``flagstats_segments_ints`` raises with: the first segment whose mask is non-zero, its range, its bits."""
    h = np.asarray(high, dtype=np.uint64).ravel()
    o = np.asarray(offsets).ravel()
    i = int(np.flatnonzero(h)[0])
    return "segment %d (offsets %d..%d): %s" % (i, int(o[i]), int(o[i + 1]), high_bits_message(int(h[i])))


def flagstats_segments_ints(values, offsets, superset: bool = False, strict: bool = True):
    """The result of ``counters_segments_ints``.  ``strict`` (default): a value outside 0..65535 inside a segment raises
    ``ValueError`` naming the first offending segment, its offsets range and the bits seen above bit 15 in it;
    ``strict=False``: the counters of the truncated values, the masks for the caller to judge."""
    out, high = counters_segments_ints(values, offsets, superset)
    if strict and high.any():
        raise ValueError(strict_message(high, np.asarray(offsets)))
    return out, high


def count_segments_device_ptr_ints(ptr: int, n: int, elem_bytes: int, offsets, superset: bool = False):
    """``(uint64[nseg, 32], uint64[nseg] high)`` of the segments of a device array of ``n`` 4-byte or 8-byte integers given as a
    raw pointer; host offsets; synchronous (``FLAGSTATS_hip_device_wide_segments_sync``)."""
    _checks.check_elem_bytes(elem_bytes, "segments.count_segments_device_ptr")
    _checks.check_raw_ints((("ptr", ptr), ("n", n)))
    ptr, n = int(ptr), int(n)
    o = check_offsets(offsets, n)
    nseg = o.size - 1
    out, high = _checks.segment_results(nseg, 1)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_device_wide_segments_sync(ptr if n else None, n, elem_bytes, o.ctypes.data, nseg,
                                                                      out.ctypes.data, high.ctypes.data,
                                                                      _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_device_wide_segments_sync")
    return out, high


def count_segments_torch_ints(t, offsets, out=None, high=None, store: bool = True, superset: bool = False):
    """Counters and high-bit masks of the segments of a 1-D contiguous integer CUDA tensor of 2-, 4- or 8-byte elements, on
    torch's current stream, nothing synchronised.

    ``offsets``: a 1-D contiguous ``int64`` CUDA tensor (nseg + 1 values) on the same device.  Its order is not checked here (that
    would synchronise): the kernel clamps what it reads, so bad offsets give undefined rows and masks, never a bad access.
    Returns ``(out, high)``: ``int64[nseg, 32]`` and ``int64[nseg]`` CUDA tensors on ``t``'s device; ``store=False`` adds into
    ``out`` and ORs into ``high`` (made zeroed when not given) instead of overwriting them.  A 2-byte tensor goes to
    ``count_segments_torch`` and cannot carry high bits: ``high`` is zeroed with ``store`` and otherwise left as it is.
    ``int(high[i])`` reads a mask as a signed 64-bit number: compare with 0, or take ``int(high[i]) & (2**64 - 1)``."""
    import torch

    _check_tensor(t)
    nseg = _checks.check_offsets_tensor(offsets)
    out, high = _checks.place_result_rows(t, nseg, store, (("out", out), ("high", high)),
                                        others=(("offsets", offsets),))
    with torch.cuda.device(t.device):
        if t.element_size() == 2:
            if store:
                high.zero_()
            count_segments_torch(t, offsets, out=out, store=store, superset=superset)
            return out, high
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(_lib.lib().FLAGSTATS_hip_device_wide_segments(t.data_ptr() if n else None, n, t.element_size(), offsets.data_ptr(),
                                                                 nseg, out.data_ptr(), high.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_wide_segments")
    return out, high
