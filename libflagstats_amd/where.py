"""Flagstat of the SELECTED elements of a FLAG column: the table for the reads with MAPQ >= 30, for one read group or contig,
for the non-null rows of an Arrow column -- without the ``values[mask]`` copy in front.

The selection is a boolean mask (numpy ``bool`` / ``torch.bool``: one byte per element, any non-zero byte selects) or, with
``packed=True``, an LSB-first bitmap in ``uint8`` (Arrow's validity layout, ``np.packbits(m, bitorder="little")``) that starts
``bit_offset`` bits into its first byte.  The 32 counters are those of ``values[mask]``; next to them the caller gets
``selected``, the number of elements the mask selects.  Array and selection are read once, by one kernel.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .pyflagstats import _as_dict


def _check_bit_offset(packed, bit_offset) -> int:
    _checks.check_int("bit_offset", bit_offset)
    if not 0 <= bit_offset < 1 << 63:
        raise ValueError("bit_offset must not be negative (and below 2**63), not %d" % bit_offset)
    if bit_offset and not packed:
        raise ValueError("bit_offset needs packed=True (a boolean mask has no bits to skip; slice it)")
    return int(bit_offset)


def _packed_bytes(n: int, bit_offset: int) -> int:
    return (bit_offset + n + 7) // 8


def _check_selection_numpy(where, n: int, packed, bit_offset):
    """the selection of ``n`` host values (also wide_where.py's): the contiguous array and the bit offset"""
    if not isinstance(where, np.ndarray):
        raise ValueError("where must be a numpy.ndarray, not %s" % type(where).__name__)
    if where.ndim != 1:
        raise ValueError("where must be 1-D, not %d-D" % where.ndim)
    bit_offset = _check_bit_offset(packed, bit_offset)
    if packed:
        if where.dtype != np.uint8:
            raise ValueError("where must have dtype uint8 with packed=True (an LSB-first bitmap), not %s" % where.dtype)
        need = _packed_bytes(n, bit_offset)
        if where.size < need:
            raise ValueError("where holds %d bytes, %d values from bit %d on need %d" % (where.size, n, bit_offset, need))
    else:
        if where.dtype != np.bool_:
            raise ValueError("where must have dtype bool (packed=True: a uint8 bitmap), not %s" % where.dtype)
        if where.size != n:
            raise ValueError("where must have one element per value (%d), not %d" % (n, where.size))
    return np.ascontiguousarray(where), bit_offset


def _check_numpy(values, where, packed, bit_offset):
    if not isinstance(values, np.ndarray):
        raise ValueError("values must be a numpy.ndarray, not %s" % type(values).__name__)
    if values.dtype != np.uint16:
        raise ValueError("values must have dtype uint16, not %s" % values.dtype)
    if values.ndim != 1:
        raise ValueError("values must be 1-D, not %d-D" % values.ndim)
    where, bit_offset = _check_selection_numpy(where, values.size, packed, bit_offset)
    return np.ascontiguousarray(values), where, bit_offset


def _check_selection_torch(where, n: int, packed, bit_offset) -> int:
    """the selection of a tensor of ``n`` elements (also wide_where.py's; devices are checked by the caller); the bit offset"""
    import torch

    if not isinstance(where, torch.Tensor):
        raise ValueError("where must be a torch.Tensor, not %s" % type(where).__name__)
    if where.dim() != 1 or not where.is_contiguous():
        raise ValueError("where must be 1-D and contiguous")
    bit_offset = _check_bit_offset(packed, bit_offset)
    if packed:
        if where.dtype != torch.uint8:
            raise ValueError("where must have dtype torch.uint8 with packed=True (an LSB-first bitmap), not %s" % where.dtype)
        need = _packed_bytes(n, bit_offset)
        if where.numel() < need:
            raise ValueError("where holds %d bytes, %d values from bit %d on need %d" % (where.numel(), n, bit_offset, need))
    else:
        if where.dtype != torch.bool:
            raise ValueError("where must have dtype torch.bool (packed=True: a torch.uint8 bitmap), not %s" % where.dtype)
        if where.numel() != n:
            raise ValueError("where must have one element per value (%d), not %d" % (n, where.numel()))
    return bit_offset


def _check_torch(t, where, packed, bit_offset) -> int:
    """the tensor and its selection as the torch entries take them (devices are checked by the caller); the bit offset"""
    _checks.check_u16_tensor(t)
    return _check_selection_torch(where, t.numel(), packed, bit_offset)


def _check_sel_bits(sel_bits) -> None:
    if sel_bits not in (1, 8) or isinstance(sel_bits, bool):
        raise ValueError("sel_bits must be 1 (an LSB-first bitmap) or 8 (one byte per element), not %r" % (sel_bits,))


def counters_where(values, where, packed: bool = False, bit_offset: int = 0, superset: bool = False):
    """``(uint64[32] counters, int selected)`` of the elements of the 1-D ``uint16`` host array ``values`` that ``where``
    selects: a ``bool`` array of the same length, or (``packed=True``) a ``uint8`` LSB-first bitmap of at least
    ``(bit_offset + n + 7) // 8`` bytes whose bit ``bit_offset + i`` belongs to ``values[i]``
    (``FLAGSTATS_hip_u16_x64_where``)."""
    v, w, bit_offset = _check_numpy(values, where, packed, bit_offset)
    out = np.zeros(32, dtype=np.uint64)
    selected = ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_u16_x64_where(v.ctypes.data if v.size else None, v.size, w.ctypes.data if v.size else None,
                                                      bit_offset, 1 if packed else 8, out.ctypes.data, ctypes.byref(selected),
                                                      _checks.c_flags(True, superset)), "FLAGSTATS_hip_u16_x64_where")
    return out, int(selected.value)


def flagstats_where(values, where, packed: bool = False, bit_offset: int = 0) -> dict:
    """The dict of ``pyflagstats.flagstats_x64(values[mask])``: ``n_values`` is the number of selected elements and ``mapped``
    is derived from it."""
    counters, selected = counters_where(values, where, packed=packed, bit_offset=bit_offset)
    return _as_dict(counters, selected)


def count_device_ptr_where(ptr: int, n: int, sel_ptr: int, sel_bits: int, sel_offset: int = 0, superset: bool = False):
    """``(uint64[32], int selected)`` of a device array of ``n`` ``uint16`` flags under a device selection, both given as raw
    pointers: ``sel_bits`` 1 = LSB-first bitmap, 8 = one byte per element; element ``i`` is bit / byte ``sel_offset + i``.
    Synchronous (``FLAGSTATS_hip_device_u16_where_sync``)."""
    _check_sel_bits(sel_bits)
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("sel_ptr", sel_ptr), ("sel_offset", sel_offset)), non_negative=("n", "sel_offset"))
    ptr, n, sel_ptr, sel_offset = int(ptr), int(n), int(sel_ptr), int(sel_offset)
    out = np.zeros(32, dtype=np.uint64)
    selected = ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_device_u16_where_sync(ptr if n else None, n, sel_ptr if n else None, sel_offset, sel_bits,
                                                              out.ctypes.data, ctypes.byref(selected),
                                                              _checks.c_flags(True, superset)), "FLAGSTATS_hip_device_u16_where_sync")
    return out, int(selected.value)


def count_torch_where(t, where, out=None, selected=None, store: bool = False, superset: bool = False, packed: bool = False,
                      bit_offset: int = 0):
    """Counters of the elements of the 1-D contiguous ``int16`` / ``uint16`` CUDA tensor ``t`` that ``where`` selects -- a
    ``torch.bool`` tensor of ``t.numel()`` elements or (``packed=True``) a ``torch.uint8`` LSB-first bitmap of at least
    ``(bit_offset + n + 7) // 8`` bytes -- on torch's current stream, nothing synchronised.

    Returns ``(out, selected)``: ``int64[32]`` and ``int64[1]`` CUDA tensors on ``t``'s device (made zeroed when not given).
    ``store=False`` adds into both; ``store=True`` overwrites both."""
    import torch

    bit_offset = _check_torch(t, where, packed, bit_offset)
    _checks.check_result_pair(out, "selected", selected)
    out, selected = _checks.place_result_pair(t, out, "selected", selected, others=(("where", where),))
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(lib.FLAGSTATS_hip_device_u16_where(t.data_ptr() if n else None, n, where.data_ptr() if n else None, bit_offset,
                                                      1 if packed else 8, out.data_ptr(), selected.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_u16_where")
    return out, selected
