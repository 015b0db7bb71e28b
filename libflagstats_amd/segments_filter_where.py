"""Segmented flagstat of the reads that pass samtools' view filter AND that a mask selects: per segment of a FLAG column, the
counters of the reads that pass ``-f require -F exclude -q min_mapq`` and that a boolean mask or an LSB-first bitmap picks, and
how many those are -- per-row-group, per-contig, per-sample or per-block tables of ``-F 0x904 -q 30`` over the non-null rows of
an Arrow column (a null FLAG is neither tested nor counted, nor reported in ``selected[i]``), all segments in one launch, with no
combined mask, no ``values[mask]`` copy and no cumulative sum at the offsets.

Segments are CSR offsets under the contract of ``segments``; the predicate is that of ``filter`` (``require & exclude != 0`` is
legal and counts nothing; ``min_mapq == 0`` reads no MAPQ); the selection is that of ``where`` and is indexed by ARRAY ELEMENT,
not by segment: a ``bool`` mask with one element per value or, with ``packed=True``, a ``uint8`` bitmap whose bit
``bit_offset + j`` belongs to ``values[j]``.  Next to every row of 32 counters the caller gets ``selected[i]``, the number of
flags of segment ``i`` that pass and are selected; with ``superset=True`` slots 0 / 16 are the primary paired reads among them
and slot 9 is ``selected[i]`` minus slot 25.  The filtered segmented entries are the call for "no mask".
"""
from __future__ import annotations

import ctypes

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .filter import _check_mapq_numpy, _check_mapq_torch, _check_predicate
from .segments import check_offsets
from .segments_filter import segment_filter_dicts
from .where import _check_numpy as _check_values_and_selection
from .where import _check_sel_bits, _check_torch


def counters_segments_filter_where(values, offsets, where, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0,
                                   packed: bool = False, bit_offset: int = 0, superset: bool = False):
    """``(uint64[nseg, 32] counters, uint64[nseg] selected)`` of the segments of the 1-D ``uint16`` host array ``values`` under
    the filter (``mapq``: a ``uint8`` array of the same length, needed when ``min_mapq > 0``) and ``where``: a ``bool`` array of
    the same length, or (``packed=True``) a ``uint8`` LSB-first bitmap of at least ``(bit_offset + n + 7) // 8`` bytes
    (``FLAGSTATS_hip_u16_x64_segments_filter_where``)."""
    v, w, bit_offset = _check_values_and_selection(values, where, packed, bit_offset)
    q = _check_mapq_numpy(mapq, v.size)
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, q is not None)
    o = check_offsets(offsets, v.size)
    nseg = o.size - 1
    out, selected = _checks.segment_results(nseg, 1)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_u16_x64_segments_filter_where(v.ctypes.data if v.size else None, v.size, o.ctypes.data, nseg,
                                                                          require, exclude,
                                                                          q.ctypes.data if q is not None and q.size else None, min_mapq,
                                                                          w.ctypes.data if v.size else None, bit_offset,
                                                                          1 if packed else 8, out.ctypes.data, selected.ctypes.data,
                                                                          _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_u16_x64_segments_filter_where")
    return out, selected


def flagstats_segments_filter_where(values, offsets, where, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0,
                                    packed: bool = False, bit_offset: int = 0) -> list:
    """One ``pyflagstats.flagstats``-shaped dict per segment (``n_values`` is the number of flags of the segment that pass and
    are selected, and ``mapped`` is derived from it)."""
    return segment_filter_dicts(*counters_segments_filter_where(values, offsets, where, require=require, exclude=exclude, mapq=mapq,
                                                                min_mapq=min_mapq, packed=packed, bit_offset=bit_offset))


def count_segments_device_ptr_filter_where(ptr: int, n: int, offsets, sel_ptr: int, sel_bits: int, sel_offset: int = 0, require: int = 0,
                                           exclude: int = 0, mapq_ptr: int = 0, min_mapq: int = 0, superset: bool = False):
    """``(uint64[nseg, 32], uint64[nseg] selected)`` of the segments of a device array of ``n`` ``uint16`` flags under the filter
    and a device selection, all given as raw pointers: the MAPQ column has ``n`` bytes (``mapq_ptr`` 0: none); ``sel_bits`` 1 =
    LSB-first bitmap, 8 = one byte per element, element ``j`` being bit / byte ``sel_offset + j``.  Host offsets.  Synchronous
    (``FLAGSTATS_hip_device_u16_segments_filter_where_sync``)."""
    _check_sel_bits(sel_bits)
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("sel_ptr", sel_ptr), ("sel_offset", sel_offset), ("mapq_ptr", mapq_ptr)),
                           non_negative=("n", "sel_offset"))
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq_ptr != 0)
    ptr, n, sel_ptr, sel_offset, mapq_ptr = int(ptr), int(n), int(sel_ptr), int(sel_offset), int(mapq_ptr)
    o = check_offsets(offsets, n)
    nseg = o.size - 1
    out, selected = _checks.segment_results(nseg, 1)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_device_u16_segments_filter_where_sync(ptr if n else None, n, o.ctypes.data, nseg, require,
                                                                                  exclude, mapq_ptr if n and mapq_ptr else None, min_mapq,
                                                                                  sel_ptr if n else None, sel_offset, sel_bits,
                                                                                  out.ctypes.data, selected.ctypes.data,
                                                                                  _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_device_u16_segments_filter_where_sync")
    return out, selected


def count_segments_torch_filter_where(t, offsets, where, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0,
                                      packed: bool = False, bit_offset: int = 0, out=None, selected=None, store: bool = True,
                                      superset: bool = False):
    """Counters of the segments of the 1-D contiguous ``int16`` / ``uint16`` CUDA tensor ``t`` under the filter (``mapq``: a 1-D
    contiguous ``torch.uint8`` tensor of ``t.numel()`` elements on ``t``'s device, needed when ``min_mapq > 0``) and ``where`` --
    a ``torch.bool`` tensor of ``t.numel()`` elements or (``packed=True``) a ``torch.uint8`` LSB-first bitmap of at least
    ``(bit_offset + n + 7) // 8`` bytes, on ``t``'s device -- on torch's current stream, nothing synchronised.

    ``offsets``: a 1-D contiguous ``int64`` CUDA tensor (nseg + 1 values) on the same device.  Its order is not checked here (that
    would synchronise): the kernel clamps what it reads, so bad offsets give undefined counters, never a bad access.
    Returns ``(out, selected)``: ``int64[nseg, 32]`` and ``int64[nseg]`` CUDA tensors on ``t``'s device; ``store=False`` adds into
    both (made zeroed when not given) instead of overwriting them."""
    import torch

    bit_offset = _check_torch(t, where, packed, bit_offset)
    _check_mapq_torch(mapq, t.numel())
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq is not None)
    nseg = _checks.check_offsets_tensor(offsets)
    out, selected = _checks.place_result_rows(t, nseg, store, (("out", out), ("selected", selected)),
                                            others=(("offsets", offsets), ("where", where), ("mapq", mapq)))
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(lib.FLAGSTATS_hip_device_u16_segments_filter_where(t.data_ptr() if n else None, n, offsets.data_ptr(), nseg, require,
                                                                      exclude, mapq.data_ptr() if mapq is not None and n else None,
                                                                      min_mapq, where.data_ptr() if n else None, bit_offset,
                                                                      1 if packed else 8, out.data_ptr(), selected.data_ptr(), flags,
                                                                      stream),
                   "FLAGSTATS_hip_device_u16_segments_filter_where")
    return out, selected
