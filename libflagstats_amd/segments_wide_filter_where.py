"""Segmented flagstat, in the integer dtype the FLAG column arrives in, of the reads that pass samtools' view filter AND that a
mask selects: per segment of an ``int32`` / ``int64`` (or 16-bit) array, the counters of the elements that pass
``-f require -F exclude -q min_mapq`` and that a boolean mask or an LSB-first bitmap picks, how many those are, and ``high[i]``,
the OR of ``element & ~0xFFFF`` (as unsigned) over the **selected** elements of segment ``i`` only, passing or not -- the per
row group, per-contig or per-sample ``-F 0x904 -q 30`` table over the non-null rows of an Arrow ``int32`` column under its
validity bitmap, all segments in one launch, with no narrowing copy, no combined mask and no call per segment.

Segments are CSR offsets under the contract of ``segments``; the predicate is that of ``filter`` and sees the low 16 bits of an
element (``require & exclude != 0`` is legal, counts nothing and reads no element, so every ``high[i]`` is then 0;
``min_mapq == 0`` reads no MAPQ); the selection is that of ``where`` and is indexed by ARRAY ELEMENT, not by segment; the value
checks and the masks are those of ``wide`` / ``segments_wide``.  ``high`` follows ``wide_filter_where``: the filter never
restricts it, the selection always does -- what lies in a slot that is not selected is unspecified, so it neither counts nor
makes ``high[i]`` non-zero (nor makes the strict form raise).  Two-byte dtypes go to the ``segments_filter_where`` functions and
cannot carry high bits.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .filter import _check_mapq_numpy, _check_mapq_torch, _check_predicate
from .segments import check_offsets
from .segments_filter import segment_filter_dicts
from .segments_filter_where import count_segments_torch_filter_where, counters_segments_filter_where
from .segments_wide import strict_message
from .where import _check_sel_bits, _check_selection_numpy, _check_selection_torch
from .wide import _check_tensor, _check_values


def counters_segments_ints_filter_where(values, offsets, where, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0,
                                        packed: bool = False, bit_offset: int = 0, superset: bool = False):
    """``(uint64[nseg, 32] counters, uint64[nseg] selected, uint64[nseg] high)`` of the segments of a 1-D host array of dtype
    int16, uint16, int32, uint32, int64 or uint64 under the filter (``mapq``: a ``uint8`` array of the same length, needed when
    ``min_mapq > 0``) and ``where``: a ``bool`` array of the same length, or (``packed=True``) a ``uint8`` LSB-first bitmap of at
    least ``(bit_offset + n + 7) // 8`` bytes.  ``selected[i]`` is the number of counted elements of segment ``i``; ``high[i]``
    covers its selected elements, passing or not.  16-bit input goes to ``counters_segments_filter_where`` (``high`` all zero),
    wider input to ``FLAGSTATS_hip_wide_x64_segments_filter_where``."""
    v = _check_values(values)
    w, bit_offset = _check_selection_numpy(where, v.size, packed, bit_offset)
    q = _check_mapq_numpy(mapq, v.size)
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, q is not None)
    o = check_offsets(offsets, v.size)
    nseg = o.size - 1
    if v.dtype.itemsize == 2:
        out, selected = counters_segments_filter_where(v.view(np.uint16), o, w, require=require, exclude=exclude, mapq=q,
                                                       min_mapq=min_mapq, packed=packed, bit_offset=bit_offset, superset=superset)
        return out, selected, np.zeros(nseg, dtype=np.uint64)
    out, selected, high = _checks.segment_results(nseg, 2)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_wide_x64_segments_filter_where(v.ctypes.data if v.size else None, v.size, v.dtype.itemsize,
                                                                           o.ctypes.data, nseg, require, exclude,
                                                                           q.ctypes.data if q is not None and q.size else None,
                                                                           min_mapq, w.ctypes.data if v.size else None, bit_offset,
                                                                           1 if packed else 8, out.ctypes.data, selected.ctypes.data,
                                                                           high.ctypes.data, _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_wide_x64_segments_filter_where")
    return out, selected, high


def flagstats_segments_ints_filter_where(values, offsets, where, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0,
                                         packed: bool = False, bit_offset: int = 0, strict: bool = True) -> list:
    """One ``pyflagstats.flagstats``-shaped dict per segment (``n_values`` is the number of elements of the segment that pass and
    are selected, and ``mapped`` is derived from it).  ``strict`` (default): a SELECTED value outside 0..65535 inside a segment,
    passing or not, raises ``ValueError`` naming the first offending segment, its offsets range and the bits seen above bit 15 in
    it (a value that is not selected never does); ``strict=False``: the dicts of the truncated values, each with its mask as an
    extra key ``"high_bits"``."""
    out, selected, high = counters_segments_ints_filter_where(values, offsets, where, require=require, exclude=exclude, mapq=mapq,
                                                              min_mapq=min_mapq, packed=packed, bit_offset=bit_offset)
    return _checks.with_high_bits(strict, high, lambda: strict_message(high, np.asarray(offsets)),
                                  lambda: segment_filter_dicts(out, selected))


def count_segments_device_ptr_ints_filter_where(ptr: int, n: int, elem_bytes: int, offsets, sel_ptr: int, sel_bits: int,
                                                sel_offset: int = 0, require: int = 0, exclude: int = 0, mapq_ptr: int = 0,
                                                min_mapq: int = 0, superset: bool = False):
    """``(uint64[nseg, 32], uint64[nseg] selected, uint64[nseg] high)`` of the segments of a device array of ``n`` 4-byte or
    8-byte integers under the filter and a device selection, all given as raw pointers: the MAPQ column has ``n`` bytes
    (``mapq_ptr`` 0: none); ``sel_bits`` 1 = LSB-first bitmap, 8 = one byte per element, element ``j`` being bit / byte
    ``sel_offset + j``.  Host offsets.  ``high`` covers the selected elements only.  Synchronous
    (``FLAGSTATS_hip_device_wide_segments_filter_where_sync``)."""
    _checks.check_elem_bytes(elem_bytes, "segments_filter_where.count_segments_device_ptr_filter_where")
    _check_sel_bits(sel_bits)
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("sel_ptr", sel_ptr), ("sel_offset", sel_offset), ("mapq_ptr", mapq_ptr)),
                           non_negative=("n", "sel_offset"))
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq_ptr != 0)
    ptr, n, sel_ptr, sel_offset, mapq_ptr = int(ptr), int(n), int(sel_ptr), int(sel_offset), int(mapq_ptr)
    o = check_offsets(offsets, n)
    nseg = o.size - 1
    out, selected, high = _checks.segment_results(nseg, 2)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_device_wide_segments_filter_where_sync(ptr if n else None, n, elem_bytes, o.ctypes.data, nseg,
                                                                                   require, exclude,
                                                                                   mapq_ptr if n and mapq_ptr else None, min_mapq,
                                                                                   sel_ptr if n else None, sel_offset, sel_bits,
                                                                                   out.ctypes.data, selected.ctypes.data, high.ctypes.data,
                                                                                   _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_device_wide_segments_filter_where_sync")
    return out, selected, high


def count_segments_torch_ints_filter_where(t, offsets, where, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0,
                                           packed: bool = False, bit_offset: int = 0, out=None, selected=None, high=None,
                                           store: bool = True, superset: bool = False):
    """Counters, counted numbers and high-bit masks of the segments of a 1-D contiguous integer CUDA tensor of 2-, 4- or 8-byte
    elements under the filter (``mapq``: a 1-D contiguous ``torch.uint8`` tensor of ``t.numel()`` elements on ``t``'s device,
    needed when ``min_mapq > 0``) and ``where`` -- a ``torch.bool`` tensor of ``t.numel()`` elements or (``packed=True``) a
    ``torch.uint8`` LSB-first bitmap of at least ``(bit_offset + n + 7) // 8`` bytes, on ``t``'s device -- on torch's current
    stream, nothing synchronised.

    ``offsets``: a 1-D contiguous ``int64`` CUDA tensor (nseg + 1 values) on the same device.  Its order is not checked here (that
    would synchronise): the kernel clamps what it reads, so bad offsets give undefined results, never a bad access.
    Returns ``(out, selected, high)``: ``int64[nseg, 32]``, ``int64[nseg]`` and ``int64[nseg]`` CUDA tensors on ``t``'s device;
    ``store=False`` adds into ``out`` and ``selected`` and ORs into ``high`` (made zeroed when not given) instead of overwriting
    them.  ``high[i]`` is the OR of the bits above bit 15 of the SELECTED elements of segment ``i`` only, passing or not.  A 2-byte
    tensor goes to ``count_segments_torch_filter_where`` and cannot carry high bits: ``high`` is zeroed with ``store`` and
    otherwise left as it is.  ``int(high[i])`` reads a mask as a signed 64-bit number: compare with 0, or take
    ``int(high[i]) & (2**64 - 1)``."""
    import torch

    _check_tensor(t)
    bit_offset = _check_selection_torch(where, t.numel(), packed, bit_offset)
    _check_mapq_torch(mapq, t.numel())
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq is not None)
    nseg = _checks.check_offsets_tensor(offsets)
    out, selected, high = _checks.place_result_rows(t, nseg, store, (("out", out), ("selected", selected), ("high", high)),
                                                  others=(("offsets", offsets), ("where", where), ("mapq", mapq)))
    with torch.cuda.device(t.device):
        if t.element_size() == 2:
            if store:
                high.zero_()
            count_segments_torch_filter_where(t, offsets, where, require=require, exclude=exclude, mapq=mapq, min_mapq=min_mapq,
                                              packed=packed, bit_offset=bit_offset, out=out, selected=selected, store=store,
                                              superset=superset)
            return out, selected, high
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(_lib.lib().FLAGSTATS_hip_device_wide_segments_filter_where(t.data_ptr() if n else None, n, t.element_size(),
                                                                              offsets.data_ptr(), nseg, require, exclude,
                                                                              mapq.data_ptr() if mapq is not None and n else None,
                                                                              min_mapq, where.data_ptr() if n else None, bit_offset,
                                                                              1 if packed else 8, out.data_ptr(), selected.data_ptr(),
                                                                              high.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_wide_segments_filter_where")
    return out, selected, high
