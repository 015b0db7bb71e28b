"""Flagstat under samtools' whole view predicate of a FLAG column in the integer dtype it arrives in: ``samtools view -f require
-F exclude --rf include_any -G exclude_all -q min_mapq | samtools flagstat`` over an ``int32`` / ``int64`` (or 16-bit) array or
tensor, read once and in place -- no ``astype(np.uint16)`` copy in front and no mask array.

``wide_filter`` with the two options of ``filter_rf``: ``include_any`` (``--rf``) keeps a read only if it has at least one of these
bits, ``exclude_all`` (``-G``) drops a read only if it has all of these bits; 0 switches either off.  The whole predicate sees the
low 16 bits of an element; the value checks and the mask ``high`` are those of ``wide``.  ``high`` is the OR of
``element & ~0xFFFF`` over **all** elements, passing or not.  One exception, as in ``wide_filter``: a predicate that no FLAG
value can pass (``require & exclude != 0``, every ``include_any`` bit excluded, every ``exclude_all`` bit required) reads no
element at all, so ``high`` is then 0.  The library reduces the four masks first, as ``filter_rf`` says: a call that leaves a
plain ``require`` / ``exclude`` pair runs ``wide_filter``'s kernel.  Two-byte dtypes go to the ``uint16`` entries of
``filter_rf`` and cannot carry high bits.  Whole columns only.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from . import filter as _filter
from . import filter_rf as _filter_rf
from . import wide as _wide
from .pyflagstats import _as_dict


def counters_ints_filter_rf(values, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0, mapq=None,
                            min_mapq: int = 0, superset: bool = False):
    """``(uint64[32] counters, int selected, int high)`` of the elements of a 1-D host array of dtype int16, uint16, int32,
    uint32, int64 or uint64 that pass the predicate (``mapq``: a ``uint8`` array of the same length, needed when
    ``min_mapq > 0``).  16-bit input goes to ``FLAGSTATS_hip_u16_x64_filter_rf`` (``high`` = 0), wider input to
    ``FLAGSTATS_hip_wide_x64_filter_rf``."""
    v = _wide._check_values(values)
    q = _filter._check_mapq_numpy(mapq, v.size)
    require, exclude, include_any, exclude_all, min_mapq = _filter_rf._check_predicate_rf(require, exclude, include_any, exclude_all,
                                                                                          min_mapq, q is not None)
    if v.dtype.itemsize == 2:
        out, selected = _filter_rf.counters_filter_rf(v.view(np.uint16), require=require, exclude=exclude, include_any=include_any,
                                                      exclude_all=exclude_all, mapq=q, min_mapq=min_mapq, superset=superset)
        return out, selected, 0
    out = np.zeros(32, dtype=np.uint64)
    selected, high = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_wide_x64_filter_rf(v.ctypes.data if v.size else None, v.size, v.dtype.itemsize, require, exclude,
                                                           include_any, exclude_all,
                                                           q.ctypes.data if q is not None and q.size else None, min_mapq,
                                                           out.ctypes.data, ctypes.byref(selected), ctypes.byref(high),
                                                           _checks.c_flags(True, superset)), "FLAGSTATS_hip_wide_x64_filter_rf")
    return out, int(selected.value), int(high.value)


def flagstats_ints_filter_rf(values, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0, mapq=None,
                             min_mapq: int = 0, strict: bool = True) -> dict:
    """The dict of ``pyflagstats.flagstats_x64`` over the values that pass: ``n_values`` is their number and ``mapped`` is
    derived from it.  ``strict`` (default): a value outside 0..65535 anywhere in the column -- selected or not -- raises
    ``ValueError`` naming the bits seen above bit 15; ``strict=False``: the dict of the truncated values with the mask as an
    extra key ``"high_bits"``."""
    counters, selected, high = counters_ints_filter_rf(values, require=require, exclude=exclude, include_any=include_any,
                                                       exclude_all=exclude_all, mapq=mapq, min_mapq=min_mapq)
    return _checks.with_high_bits(strict, high, lambda: _wide.high_bits_message(high), lambda: _as_dict(counters, selected))


def count_device_ptr_ints_filter_rf(ptr: int, n: int, elem_bytes: int, require: int = 0, exclude: int = 0, include_any: int = 0,
                                    exclude_all: int = 0, mapq_ptr: int = 0, min_mapq: int = 0, superset: bool = False):
    """``(uint64[32], int selected, int high)`` of a device array of ``n`` 4-byte or 8-byte integers under the predicate, array
    and MAPQ column (``n`` bytes; ``mapq_ptr`` 0: none) given as raw pointers.  Synchronous
    (``FLAGSTATS_hip_device_wide_filter_rf_sync``)."""
    _checks.check_elem_bytes(elem_bytes, "filter_rf.count_device_ptr_filter_rf")
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("mapq_ptr", mapq_ptr)))
    require, exclude, include_any, exclude_all, min_mapq = _filter_rf._check_predicate_rf(require, exclude, include_any, exclude_all,
                                                                                          min_mapq, mapq_ptr != 0)
    ptr, n, mapq_ptr = int(ptr), int(n), int(mapq_ptr)
    out = np.zeros(32, dtype=np.uint64)
    selected, high = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_device_wide_filter_rf_sync(ptr if n else None, n, elem_bytes, require, exclude, include_any,
                                                                   exclude_all, mapq_ptr if n and mapq_ptr else None, min_mapq,
                                                                   out.ctypes.data, ctypes.byref(selected), ctypes.byref(high),
                                                                   _checks.c_flags(True, superset)),
               "FLAGSTATS_hip_device_wide_filter_rf_sync")
    return out, int(selected.value), int(high.value)


def count_torch_ints_filter_rf(t, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0, mapq=None,
                               min_mapq: int = 0, out=None, selected=None, high=None, store: bool = False, superset: bool = False):
    """Counters, selected count and high-bit mask of the elements of a 1-D contiguous integer CUDA tensor of 2-, 4- or 8-byte
    elements that pass the predicate (``mapq``: a 1-D contiguous ``torch.uint8`` tensor of ``t.numel()`` elements on ``t``'s
    device, needed when ``min_mapq > 0``) -- on torch's current stream, nothing synchronised.

    Returns ``(out, selected, high)``: ``int64[32]``, ``int64[1]`` and ``int64[1]`` CUDA tensors on ``t``'s device (made zeroed
    when not given).  ``store=False`` adds into ``out`` and ``selected`` and ORs into ``high``; ``store=True`` overwrites all
    three.  A 2-byte tensor goes to the ``uint16`` entry of ``filter_rf`` and cannot carry high bits: ``high`` is left as it is
    (zeroed with ``store``).  ``int(high)`` reads the mask as a signed 64-bit number: compare with 0, or take
    ``int(high) & (2**64 - 1)``."""
    import torch

    _wide._check_tensor(t)
    _filter._check_mapq_torch(mapq, t.numel())
    require, exclude, include_any, exclude_all, min_mapq = _filter_rf._check_predicate_rf(require, exclude, include_any, exclude_all,
                                                                                          min_mapq, mapq is not None)
    out, selected, high = _checks.place_result_triple(t, out, selected, high, others=(("mapq", mapq),))
    if t.element_size() == 2:
        if store:
            with torch.cuda.device(t.device):
                high.zero_()
        _filter_rf.count_torch_filter_rf(t, require=require, exclude=exclude, include_any=include_any, exclude_all=exclude_all,
                                         mapq=mapq, min_mapq=min_mapq, out=out, selected=selected, store=store, superset=superset)
        return out, selected, high
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(lib.FLAGSTATS_hip_device_wide_filter_rf(t.data_ptr() if n else None, n, t.element_size(), require, exclude, include_any,
                                                           exclude_all, mapq.data_ptr() if mapq is not None and n else None, min_mapq,
                                                           out.data_ptr(), selected.data_ptr(), high.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_wide_filter_rf")
    return out, selected, high
