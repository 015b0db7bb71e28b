"""Filtered segmented flagstat of a FLAG column in the integer dtype it arrives in: per segment of an ``int32`` / ``int64`` (or
16-bit) array, the counters of the reads that pass samtools' view filter (``-f require -F exclude -q min_mapq``), how many pass,
and ``high[i]``, the OR over **all** elements of segment ``i`` -- passing or not -- of ``element & ~0xFFFF`` (as unsigned):
per-contig, per-sample or per-block tables of the reads passing ``-F 0x904 -q 30`` straight from a pandas, Arrow or torch column,
all segments in one launch, with no narrowing copy and no mask array.

Segments are CSR offsets under the contract of ``segments``; the predicate is that of ``filter`` and sees the low 16 bits of an
element; the value checks and the masks are those of ``wide`` / ``segments_wide``.  One exception, as in ``wide_filter``:
``require & exclude != 0`` (legal, passes nothing) reads no element at all, so every ``high[i]`` is then 0.  Two-byte dtypes go to
the ``uint16`` segmented filter entries and cannot carry high bits.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .filter import _check_mapq_numpy, _check_mapq_torch, _check_predicate
from .segments import check_offsets
from .segments_filter import count_segments_torch_filter
from .segments_wide import strict_message
from .wide import _check_tensor, _check_values


def counters_segments_ints_filter(values, offsets, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0,
                                  superset: bool = False):
    """``(uint64[nseg, 32] counters, uint64[nseg] selected, uint64[nseg] high)`` of the segments of a 1-D host array of dtype
    int16, uint16, int32, uint32, int64 or uint64 under the filter (``mapq``: a ``uint8`` array of the same length, needed when
    ``min_mapq > 0``).  16-bit input goes to ``FLAGSTATS_hip_u16_x64_segments_filter`` (``high`` all zero), wider input to
    ``FLAGSTATS_hip_wide_x64_segments_filter``."""
    v = _check_values(values)
    q = _check_mapq_numpy(mapq, v.size)
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, q is not None)
    o = check_offsets(offsets, v.size)
    nseg = o.size - 1
    out, selected, high = _checks.segment_results(nseg, 2)
    if not nseg:
        return out, selected, high
    flags = _checks.c_flags(True, superset)
    lib = _lib.lib()
    ptr = v.ctypes.data if v.size else None
    qptr = q.ctypes.data if q is not None and q.size else None
    if v.dtype.itemsize == 2:
        _lib.check(lib.FLAGSTATS_hip_u16_x64_segments_filter(ptr, v.size, o.ctypes.data, nseg, require, exclude, qptr, min_mapq,
                                                             out.ctypes.data, selected.ctypes.data, flags),
                   "FLAGSTATS_hip_u16_x64_segments_filter")
    else:
        _lib.check(lib.FLAGSTATS_hip_wide_x64_segments_filter(ptr, v.size, v.dtype.itemsize, o.ctypes.data, nseg, require, exclude, qptr,
                                                              min_mapq, out.ctypes.data, selected.ctypes.data, high.ctypes.data, flags),
                   "FLAGSTATS_hip_wide_x64_segments_filter")
    return out, selected, high


def flagstats_segments_ints_filter(values, offsets, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0,
                                   superset: bool = False, strict: bool = True):
    """The result of ``counters_segments_ints_filter``.  ``strict`` (default): a value outside 0..65535 inside a segment --
    selected or not -- raises ``ValueError`` naming the first offending segment, its offsets range and the bits seen above bit
    15 in it; ``strict=False``: the counters of the truncated values, the masks for the caller to judge.
    ``segments_filter.segment_filter_dicts(counters, selected)`` shapes the rows."""
    out, selected, high = counters_segments_ints_filter(values, offsets, require=require, exclude=exclude, mapq=mapq,
                                                        min_mapq=min_mapq, superset=superset)
    if strict and high.any():
        raise ValueError(strict_message(high, np.asarray(offsets)))
    return out, selected, high


def count_segments_device_ptr_ints_filter(ptr: int, n: int, elem_bytes: int, offsets, require: int = 0, exclude: int = 0,
                                          mapq_ptr: int = 0, min_mapq: int = 0, superset: bool = False):
    """``(uint64[nseg, 32], uint64[nseg] selected, uint64[nseg] high)`` of the segments of a device array of ``n`` 4-byte or
    8-byte integers under the filter, array and MAPQ column (``n`` bytes; ``mapq_ptr`` 0: none) given as raw pointers; host
    offsets; synchronous (``FLAGSTATS_hip_device_wide_segments_filter_sync``)."""
    _checks.check_elem_bytes(elem_bytes, "segments_filter.count_segments_device_ptr_filter")
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("mapq_ptr", mapq_ptr)))
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq_ptr != 0)
    ptr, n, mapq_ptr = int(ptr), int(n), int(mapq_ptr)
    o = check_offsets(offsets, n)
    nseg = o.size - 1
    out, selected, high = _checks.segment_results(nseg, 2)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_device_wide_segments_filter_sync(ptr if n else None, n, elem_bytes, o.ctypes.data, nseg,
                                                                             require, exclude, mapq_ptr if n and mapq_ptr else None,
                                                                             min_mapq, out.ctypes.data, selected.ctypes.data,
                                                                             high.ctypes.data, _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_device_wide_segments_filter_sync")
    return out, selected, high


def count_segments_torch_ints_filter(t, offsets, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0, out=None,
                                     selected=None, high=None, store: bool = True, superset: bool = False):
    """Counters, selected counts and high-bit masks of the segments of a 1-D contiguous integer CUDA tensor of 2-, 4- or 8-byte
    elements under the filter (``mapq``: a 1-D contiguous ``torch.uint8`` tensor of ``t.numel()`` elements on ``t``'s device,
    needed when ``min_mapq > 0``), on torch's current stream, nothing synchronised.

    ``offsets``: a 1-D contiguous ``int64`` CUDA tensor (nseg + 1 values) on the same device.  Its order is not checked here (that
    would synchronise): the kernel clamps what it reads, so bad offsets give undefined results, never a bad access.
    Returns ``(out, selected, high)``: ``int64[nseg, 32]``, ``int64[nseg]`` and ``int64[nseg]`` CUDA tensors on ``t``'s device;
    ``store=False`` adds into ``out`` and ``selected`` and ORs into ``high`` (made zeroed when not given) instead of overwriting
    them.  A 2-byte tensor goes to ``count_segments_torch_filter`` and cannot carry high bits: ``high`` is zeroed with ``store``
    and otherwise left as it is.  ``int(high[i])`` reads a mask as a signed 64-bit number: compare with 0, or take
    ``int(high[i]) & (2**64 - 1)``."""
    import torch

    _check_tensor(t)
    nseg = _checks.check_offsets_tensor(offsets)
    _check_mapq_torch(mapq, t.numel())
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq is not None)
    out, selected, high = _checks.place_result_rows(t, nseg, store, (("out", out), ("selected", selected), ("high", high)),
                                                  others=(("offsets", offsets), ("mapq", mapq)))
    with torch.cuda.device(t.device):
        if t.element_size() == 2:
            if store:
                high.zero_()
            count_segments_torch_filter(t, offsets, require=require, exclude=exclude, mapq=mapq, min_mapq=min_mapq, out=out,
                                        selected=selected, store=store, superset=superset)
            return out, selected, high
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(_lib.lib().FLAGSTATS_hip_device_wide_segments_filter(t.data_ptr() if n else None, n, t.element_size(),
                                                                        offsets.data_ptr(), nseg, require, exclude,
                                                                        mapq.data_ptr() if mapq is not None and n else None,
                                                                        min_mapq, out.data_ptr(), selected.data_ptr(),
                                                                        high.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_wide_segments_filter")
    return out, selected, high
