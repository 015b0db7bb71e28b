"""Flagstat of the SELECTED elements of a FLAG column in the integer dtype it arrives in: an Arrow ``int32`` column under its
validity bitmap, an ``int64`` tensor under a ``torch.bool`` mask -- read once and in place, with no ``astype(np.uint16)`` copy and
no ``values[mask]`` compaction in front.

The selection is that of ``where`` (a boolean mask, or with ``packed=True`` an LSB-first ``uint8`` bitmap that starts
``bit_offset`` bits into its first byte); the value checks and the mask ``high`` are those of ``wide``.  ``high`` is the OR of
``element & ~0xFFFF`` over the **selected** elements only: a selection is typically a validity bitmap, and what lies in a slot
that is not selected is unspecified, so it neither counts nor makes ``high`` non-zero (nor makes the strict form raise).  This
differs on purpose from ``wide_filter``, whose ``high`` covers every element read, passing or not.  Two-byte dtypes go to the
``uint16`` ``where`` entries and cannot carry high bits.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from . import where as _where
from . import wide as _wide
from .pyflagstats import _as_dict


def counters_ints_where(values, where, packed: bool = False, bit_offset: int = 0, superset: bool = False):
    """``(uint64[32] counters, int selected, int high)`` of the elements of a 1-D host array of dtype int16, uint16, int32,
    uint32, int64 or uint64 that ``where`` selects: a ``bool`` array of the same length, or (``packed=True``) a ``uint8``
    LSB-first bitmap of at least ``(bit_offset + n + 7) // 8`` bytes whose bit ``bit_offset + i`` belongs to ``values[i]``.
    ``high`` is the OR of the bits above bit 15 of the selected elements only.  16-bit input goes to
    ``FLAGSTATS_hip_u16_x64_where`` (``high`` = 0), wider input to ``FLAGSTATS_hip_wide_x64_where``."""
    v = _wide._check_values(values)
    w, bit_offset = _where._check_selection_numpy(where, v.size, packed, bit_offset)
    if v.dtype.itemsize == 2:
        out, selected = _where.counters_where(v.view(np.uint16), w, packed=packed, bit_offset=bit_offset, superset=superset)
        return out, selected, 0
    out = np.zeros(32, dtype=np.uint64)
    selected, high = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_wide_x64_where(v.ctypes.data if v.size else None, v.size, v.dtype.itemsize,
                                                       w.ctypes.data if v.size else None, bit_offset, 1 if packed else 8,
                                                       out.ctypes.data, ctypes.byref(selected), ctypes.byref(high),
                                                       _checks.c_flags(True, superset)), "FLAGSTATS_hip_wide_x64_where")
    return out, int(selected.value), int(high.value)


def flagstats_ints_where(values, where, packed: bool = False, bit_offset: int = 0, strict: bool = True) -> dict:
    """The dict of ``pyflagstats.flagstats_x64(values[mask])``: ``n_values`` is the number of selected elements and ``mapped`` is
    derived from it.  ``strict`` (default): a SELECTED value outside 0..65535 raises ``ValueError`` naming the bits seen above
    bit 15 (a value that is not selected never does); ``strict=False``: the dict of the truncated values with the mask as an
    extra key ``"high_bits"``."""
    counters, selected, high = counters_ints_where(values, where, packed=packed, bit_offset=bit_offset)
    return _checks.with_high_bits(strict, high, lambda: _wide.high_bits_message(high), lambda: _as_dict(counters, selected))


def count_device_ptr_ints_where(ptr: int, n: int, elem_bytes: int, sel_ptr: int, sel_bits: int, sel_offset: int = 0,
                                superset: bool = False):
    """``(uint64[32], int selected, int high)`` of a device array of ``n`` 4-byte or 8-byte integers under a device selection,
    both given as raw pointers: ``sel_bits`` 1 = LSB-first bitmap, 8 = one byte per element; element ``i`` is bit / byte
    ``sel_offset + i``.  ``high`` covers the selected elements only.  Synchronous (``FLAGSTATS_hip_device_wide_where_sync``)."""
    _checks.check_elem_bytes(elem_bytes, "where.count_device_ptr_where")
    _where._check_sel_bits(sel_bits)
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("sel_ptr", sel_ptr), ("sel_offset", sel_offset)), non_negative=("n", "sel_offset"))
    ptr, n, sel_ptr, sel_offset = int(ptr), int(n), int(sel_ptr), int(sel_offset)
    out = np.zeros(32, dtype=np.uint64)
    selected, high = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_device_wide_where_sync(ptr if n else None, n, elem_bytes, sel_ptr if n else None, sel_offset,
                                                               sel_bits, out.ctypes.data, ctypes.byref(selected), ctypes.byref(high),
                                                               _checks.c_flags(True, superset)),
               "FLAGSTATS_hip_device_wide_where_sync")
    return out, int(selected.value), int(high.value)


def count_torch_ints_where(t, where, out=None, selected=None, high=None, store: bool = False, superset: bool = False,
                           packed: bool = False, bit_offset: int = 0):
    """Counters, selected count and high-bit mask of the elements of a 1-D contiguous integer CUDA tensor of 2-, 4- or 8-byte
    elements that ``where`` selects -- a ``torch.bool`` tensor of ``t.numel()`` elements or (``packed=True``) a ``torch.uint8``
    LSB-first bitmap of at least ``(bit_offset + n + 7) // 8`` bytes -- on torch's current stream, nothing synchronised.

    Returns ``(out, selected, high)``: ``int64[32]``, ``int64[1]`` and ``int64[1]`` CUDA tensors on ``t``'s device (made zeroed
    when not given).  ``store=False`` adds into ``out`` and ``selected`` and ORs into ``high``; ``store=True`` overwrites all
    three.  ``high`` is the OR of the bits above bit 15 of the SELECTED elements only (``wide_filter``'s covers every element).
    A 2-byte tensor goes to the ``uint16`` ``where`` entry and cannot carry high bits: ``high`` is left as it is (zeroed with
    ``store``).  ``int(high)`` reads the mask as a signed 64-bit number: compare with 0, or take ``int(high) & (2**64 - 1)``."""
    import torch

    _wide._check_tensor(t)
    bit_offset = _where._check_selection_torch(where, t.numel(), packed, bit_offset)
    out, selected, high = _checks.place_result_triple(t, out, selected, high, others=(("where", where),))
    if t.element_size() == 2:
        if store:
            with torch.cuda.device(t.device):
                high.zero_()
        _where.count_torch_where(t, where, out=out, selected=selected, store=store, superset=superset, packed=packed,
                                 bit_offset=bit_offset)
        return out, selected, high
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(lib.FLAGSTATS_hip_device_wide_where(t.data_ptr() if n else None, n, t.element_size(),
                                                       where.data_ptr() if n else None, bit_offset, 1 if packed else 8,
                                                       out.data_ptr(), selected.data_ptr(), high.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_wide_where")
    return out, selected, high
