"""Flagstat of the reads that pass samtools' view filter AND that a mask selects: ``-f require -F exclude -q min_mapq`` on a
FLAG column with a validity bitmap (a null FLAG is neither tested nor counted), or on the reads of a region / read-group / dedup
mask -- in one pass, with no combined mask in memory.

An element is counted when it passes the filter of :mod:`libflagstats_amd.filter` (every bit of ``require``, no bit of
``exclude`` and, with ``min_mapq > 0``, a MAPQ of at least ``min_mapq`` in the ``uint8`` column ``mapq``) and the selection of
:mod:`libflagstats_amd.where` selects it (a boolean mask, or with ``packed=True`` an LSB-first bitmap in ``uint8`` that starts
``bit_offset`` bits into its first byte).  The 32 counters are those of the counted values; next to them the caller gets
``selected``, their number.  Array, column and selection are read once, by one kernel.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .filter import _check_mapq_numpy, _check_mapq_torch, _check_predicate
from .pyflagstats import _as_dict
from .where import _check_numpy as _check_values_and_selection
from .where import _check_sel_bits, _check_torch


def counters_filter_where(values, where, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0, packed: bool = False,
                          bit_offset: int = 0, superset: bool = False):
    """``(uint64[32] counters, int selected)`` of the elements of the 1-D ``uint16`` host array ``values`` that pass the filter
    (``require``, ``exclude``, and with ``min_mapq > 0`` ``mapq[i] >= min_mapq``; ``mapq``: a ``uint8`` array of the same
    length) and that ``where`` selects: a ``bool`` array of the same length, or (``packed=True``) a ``uint8`` LSB-first bitmap of
    at least ``(bit_offset + n + 7) // 8`` bytes whose bit ``bit_offset + i`` belongs to ``values[i]``
    (``FLAGSTATS_hip_u16_x64_filter_where``)."""
    v, w, bit_offset = _check_values_and_selection(values, where, packed, bit_offset)
    q = _check_mapq_numpy(mapq, v.size)
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, q is not None)
    out = np.zeros(32, dtype=np.uint64)
    selected = ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_u16_x64_filter_where(v.ctypes.data if v.size else None, v.size, require, exclude,
                                                             q.ctypes.data if q is not None and q.size else None, min_mapq,
                                                             w.ctypes.data if v.size else None, bit_offset, 1 if packed else 8,
                                                             out.ctypes.data, ctypes.byref(selected),
                                                             _checks.c_flags(True, superset)),
               "FLAGSTATS_hip_u16_x64_filter_where")
    return out, int(selected.value)


def flagstats_filter_where(values, where, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0, packed: bool = False,
                           bit_offset: int = 0) -> dict:
    """The dict of ``pyflagstats.flagstats_x64`` over the counted values: ``n_values`` is their number and ``mapped`` is derived
    from it."""
    counters, selected = counters_filter_where(values, where, require=require, exclude=exclude, mapq=mapq, min_mapq=min_mapq,
                                               packed=packed, bit_offset=bit_offset)
    return _as_dict(counters, selected)


def count_device_ptr_filter_where(ptr: int, n: int, sel_ptr: int, sel_bits: int, require: int = 0, exclude: int = 0, mapq_ptr: int = 0,
                                  min_mapq: int = 0, sel_offset: int = 0, superset: bool = False):
    """``(uint64[32], int selected)`` of a device array of ``n`` ``uint16`` flags under the filter and a device selection, all
    given as raw pointers: the MAPQ column has ``n`` bytes (``mapq_ptr`` 0: none); ``sel_bits`` 1 = LSB-first bitmap, 8 = one byte
    per element, element ``i`` being bit / byte ``sel_offset + i``.  Synchronous (``FLAGSTATS_hip_device_u16_filter_where_sync``)."""
    _check_sel_bits(sel_bits)
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("sel_ptr", sel_ptr), ("sel_offset", sel_offset), ("mapq_ptr", mapq_ptr)),
                           non_negative=("n", "sel_offset"))
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq_ptr != 0)
    ptr, n, sel_ptr, sel_offset, mapq_ptr = int(ptr), int(n), int(sel_ptr), int(sel_offset), int(mapq_ptr)
    out = np.zeros(32, dtype=np.uint64)
    selected = ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_device_u16_filter_where_sync(ptr if n else None, n, require, exclude,
                                                                     mapq_ptr if n and mapq_ptr else None, min_mapq,
                                                                     sel_ptr if n else None, sel_offset, sel_bits, out.ctypes.data,
                                                                     ctypes.byref(selected), _checks.c_flags(True, superset)),
               "FLAGSTATS_hip_device_u16_filter_where_sync")
    return out, int(selected.value)


def count_torch_filter_where(t, where, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0, packed: bool = False,
                             bit_offset: int = 0, out=None, selected=None, store: bool = False, superset: bool = False):
    """Counters of the elements of the 1-D contiguous ``int16`` / ``uint16`` CUDA tensor ``t`` that pass the filter (``mapq``: a
    1-D contiguous ``torch.uint8`` tensor of ``t.numel()`` elements on ``t``'s device, needed when ``min_mapq > 0``) and that
    ``where`` selects -- a ``torch.bool`` tensor of ``t.numel()`` elements or (``packed=True``) a ``torch.uint8`` LSB-first
    bitmap of at least ``(bit_offset + n + 7) // 8`` bytes -- on torch's current stream, nothing synchronised.

    Returns ``(out, selected)``: ``int64[32]`` and ``int64[1]`` CUDA tensors on ``t``'s device (made zeroed when not given).
    ``store=False`` adds into both; ``store=True`` overwrites both."""
    import torch

    bit_offset = _check_torch(t, where, packed, bit_offset)
    _check_mapq_torch(mapq, t.numel())
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq is not None)
    _checks.check_result_pair(out, "selected", selected)
    out, selected = _checks.place_result_pair(t, out, "selected", selected, others=(("where", where), ("mapq", mapq)))
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(lib.FLAGSTATS_hip_device_u16_filter_where(t.data_ptr() if n else None, n, require, exclude,
                                                             mapq.data_ptr() if mapq is not None and n else None, min_mapq,
                                                             where.data_ptr() if n else None, bit_offset, 1 if packed else 8,
                                                             out.data_ptr(), selected.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_u16_filter_where")
    return out, selected
