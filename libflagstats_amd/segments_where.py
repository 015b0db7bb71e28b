"""Segmented flagstat of the SELECTED elements of a FLAG column: per segment, the counters of the reads that a boolean mask or an
LSB-first bitmap picks and how many it picks -- per-contig, per-sample or per-block tables over the non-null rows of an Arrow
column, over the result of an upstream query, over a deduplication or region mask -- all segments in one launch, with no
``values[mask]`` copy and no cumulative sum of the mask at the offsets.

Segments are CSR offsets under the contract of ``segments`` (segment ``i`` is ``values[offsets[i]:offsets[i+1]]``; flags outside
every segment count nowhere; empty segments are allowed).  The selection is that of ``where`` and is indexed by ARRAY ELEMENT, not
by segment: a ``bool`` mask with one element per value or, with ``packed=True``, a ``uint8`` bitmap whose bit ``bit_offset + j``
belongs to ``values[j]``.  Next to every row of 32 counters the caller gets ``selected[i]``, the number of selected flags of
segment ``i``; with ``superset=True`` slots 0 / 16 are the primary paired reads among them and slot 9 is ``selected[i]`` minus
slot 25.
"""
from __future__ import annotations

import ctypes

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .segments import check_offsets
from .segments_filter import segment_filter_dicts
from .where import _check_numpy, _check_torch


def counters_segments_where(values, offsets, where, packed: bool = False, bit_offset: int = 0, superset: bool = False):
    """``(uint64[nseg, 32] counters, uint64[nseg] selected)`` of the segments of the 1-D ``uint16`` host array ``values`` under
    ``where``: a ``bool`` array of the same length, or (``packed=True``) a ``uint8`` LSB-first bitmap of at least
    ``(bit_offset + n + 7) // 8`` bytes (``FLAGSTATS_hip_u16_x64_segments_where``)."""
    v, w, bit_offset = _check_numpy(values, where, packed, bit_offset)
    o = check_offsets(offsets, v.size)
    nseg = o.size - 1
    out, selected = _checks.segment_results(nseg, 1)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_u16_x64_segments_where(v.ctypes.data if v.size else None, v.size, o.ctypes.data, nseg,
                                                                   w.ctypes.data if v.size else None, bit_offset, 1 if packed else 8,
                                                                   out.ctypes.data, selected.ctypes.data,
                                                                   _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_u16_x64_segments_where")
    return out, selected


def flagstats_segments_where(values, offsets, where, packed: bool = False, bit_offset: int = 0) -> list:
    """One ``pyflagstats.flagstats``-shaped dict per segment (``n_values`` is the number of selected flags of the segment and
    ``mapped`` is derived from it)."""
    return segment_filter_dicts(*counters_segments_where(values, offsets, where, packed=packed, bit_offset=bit_offset))


def count_segments_device_ptr_where(ptr: int, n: int, offsets, sel_ptr: int, sel_bits: int, sel_offset: int = 0, superset: bool = False):
    """``(uint64[nseg, 32], uint64[nseg] selected)`` of the segments of a device array of ``n`` ``uint16`` flags under a device
    selection, both given as raw pointers: ``sel_bits`` 1 = LSB-first bitmap, 8 = one byte per element; element ``j`` is bit / byte
    ``sel_offset + j``.  Host offsets.  Synchronous (``FLAGSTATS_hip_device_u16_segments_where_sync``)."""
    if sel_bits not in (1, 8) or isinstance(sel_bits, bool):
        raise ValueError("sel_bits must be 1 (an LSB-first bitmap) or 8 (one byte per element), not %r" % (sel_bits,))
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("sel_ptr", sel_ptr), ("sel_offset", sel_offset)), non_negative=("n", "sel_offset"))
    ptr, n, sel_ptr, sel_offset = int(ptr), int(n), int(sel_ptr), int(sel_offset)
    o = check_offsets(offsets, n)
    nseg = o.size - 1
    out, selected = _checks.segment_results(nseg, 1)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_device_u16_segments_where_sync(ptr if n else None, n, o.ctypes.data, nseg,
                                                                           sel_ptr if n else None, sel_offset, sel_bits,
                                                                           out.ctypes.data, selected.ctypes.data,
                                                                           _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_device_u16_segments_where_sync")
    return out, selected


def count_segments_torch_where(t, offsets, where, packed: bool = False, bit_offset: int = 0, out=None, selected=None,
                               store: bool = True, superset: bool = False):
    """Counters of the segments of the 1-D contiguous ``int16`` / ``uint16`` CUDA tensor ``t`` under ``where`` -- a ``torch.bool``
    tensor of ``t.numel()`` elements or (``packed=True``) a ``torch.uint8`` LSB-first bitmap of at least
    ``(bit_offset + n + 7) // 8`` bytes, on ``t``'s device -- on torch's current stream, nothing synchronised.

    ``offsets``: a 1-D contiguous ``int64`` CUDA tensor (nseg + 1 values) on the same device.  Its order is not checked here (that
    would synchronise): the kernel clamps what it reads, so bad offsets give undefined counters, never a bad access.
    Returns ``(out, selected)``: ``int64[nseg, 32]`` and ``int64[nseg]`` CUDA tensors on ``t``'s device; ``store=False`` adds into
    both (made zeroed when not given) instead of overwriting them."""
    import torch

    bit_offset = _check_torch(t, where, packed, bit_offset)
    nseg = _checks.check_offsets_tensor(offsets)
    out, selected = _checks.place_result_rows(t, nseg, store, (("out", out), ("selected", selected)),
                                            others=(("offsets", offsets), ("where", where)))
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(lib.FLAGSTATS_hip_device_u16_segments_where(t.data_ptr() if n else None, n, offsets.data_ptr(), nseg,
                                                               where.data_ptr() if n else None, bit_offset, 1 if packed else 8,
                                                               out.data_ptr(), selected.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_u16_segments_where")
    return out, selected
