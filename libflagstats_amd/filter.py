"""Flagstat of the reads that pass samtools' view filter: ``samtools view -f require -F exclude -q min_mapq | samtools
flagstat`` in one pass, with no mask array in memory.

An element passes when it has every bit of ``require``, no bit of ``exclude`` and -- with ``min_mapq > 0`` -- a MAPQ of at least
``min_mapq`` in the ``uint8`` column ``mapq`` that has one element per value.  The 32 counters are those of the values that pass;
next to them the caller gets ``selected``, their number.  ``require & exclude != 0`` is legal, as in samtools, and passes nothing.
The predicate is applied inside the counting kernel: the array (and the column, when ``min_mapq > 0``) is read once.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .pyflagstats import _as_dict


def _check_flag_mask(name: str, x) -> int:
    """``x`` is an int in 0..65535: one of the predicate's masks over the 16 FLAG bits"""
    _checks.check_int(name, x)
    if not 0 <= x <= 0xFFFF:
        raise ValueError("%s must be a 16-bit FLAG mask (0..65535), not %d" % (name, x))
    return int(x)


def _check_predicate(require, exclude, min_mapq, has_mapq: bool):
    for name, x in (("require", require), ("exclude", exclude)):
        _check_flag_mask(name, x)
    _checks.check_int("min_mapq", min_mapq)
    if not 0 <= min_mapq <= 255:
        raise ValueError("min_mapq must be in 0..255 (MAPQ is one byte), not %d" % min_mapq)
    if min_mapq > 0 and not has_mapq:
        raise ValueError("min_mapq > 0 needs mapq (one uint8 per value)")
    return int(require), int(exclude), int(min_mapq)


def _check_mapq_numpy(mapq, n: int):
    """a given host MAPQ column is a 1-D ``uint8`` array of ``n`` elements; returns it contiguous (``None`` stays ``None``)"""
    if mapq is None:
        return None
    if not isinstance(mapq, np.ndarray):
        raise ValueError("mapq must be a numpy.ndarray, not %s" % type(mapq).__name__)
    if mapq.dtype != np.uint8:
        raise ValueError("mapq must have dtype uint8, not %s" % mapq.dtype)
    if mapq.ndim != 1:
        raise ValueError("mapq must be 1-D, not %d-D" % mapq.ndim)
    if mapq.size != n:
        raise ValueError("mapq must have one element per value (%d), not %d" % (n, mapq.size))
    return np.ascontiguousarray(mapq)


def _check_mapq_torch(mapq, n: int) -> None:
    """a given MAPQ tensor is 1-D, contiguous, ``torch.uint8`` and has ``n`` elements"""
    import torch

    if mapq is None:
        return
    if not isinstance(mapq, torch.Tensor):
        raise ValueError("mapq must be a torch.Tensor, not %s" % type(mapq).__name__)
    if mapq.dtype != torch.uint8:
        raise ValueError("mapq must have dtype torch.uint8, not %s" % mapq.dtype)
    if mapq.dim() != 1 or not mapq.is_contiguous():
        raise ValueError("mapq must be 1-D and contiguous")
    if mapq.numel() != n:
        raise ValueError("mapq must have one element per value (%d), not %d" % (n, mapq.numel()))


def _check_numpy(values, mapq):
    if not isinstance(values, np.ndarray):
        raise ValueError("values must be a numpy.ndarray, not %s" % type(values).__name__)
    if values.dtype != np.uint16:
        raise ValueError("values must have dtype uint16, not %s" % values.dtype)
    if values.ndim != 1:
        raise ValueError("values must be 1-D, not %d-D" % values.ndim)
    return np.ascontiguousarray(values), _check_mapq_numpy(mapq, values.size)


def counters_filter(values, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0, superset: bool = False):
    """``(uint64[32] counters, int selected)`` of the elements of the 1-D ``uint16`` host array ``values`` that have every bit
    of ``require``, no bit of ``exclude`` and, with ``min_mapq > 0``, ``mapq[i] >= min_mapq`` (``mapq``: a ``uint8`` array of
    the same length) (``FLAGSTATS_hip_u16_x64_filter``)."""
    v, q = _check_numpy(values, mapq)
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, q is not None)
    out = np.zeros(32, dtype=np.uint64)
    selected = ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_u16_x64_filter(v.ctypes.data if v.size else None, v.size, require, exclude,
                                                       q.ctypes.data if q is not None and q.size else None, min_mapq,
                                                       out.ctypes.data, ctypes.byref(selected),
                                                       _checks.c_flags(True, superset)), "FLAGSTATS_hip_u16_x64_filter")
    return out, int(selected.value)


def flagstats_filter(values, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0) -> dict:
    """The dict of ``pyflagstats.flagstats_x64`` over the values that pass: ``n_values`` is their number and ``mapped`` is
    derived from it."""
    counters, selected = counters_filter(values, require=require, exclude=exclude, mapq=mapq, min_mapq=min_mapq)
    return _as_dict(counters, selected)


def count_device_ptr_filter(ptr: int, n: int, require: int = 0, exclude: int = 0, mapq_ptr: int = 0, min_mapq: int = 0,
                            superset: bool = False):
    """``(uint64[32], int selected)`` of a device array of ``n`` ``uint16`` flags under the filter, array and MAPQ column
    (``n`` bytes; ``mapq_ptr`` 0: none) given as raw pointers.  Synchronous (``FLAGSTATS_hip_device_u16_filter_sync``)."""
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("mapq_ptr", mapq_ptr)))
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq_ptr != 0)
    ptr, n, mapq_ptr = int(ptr), int(n), int(mapq_ptr)
    out = np.zeros(32, dtype=np.uint64)
    selected = ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_device_u16_filter_sync(ptr if n else None, n, require, exclude, mapq_ptr if n and mapq_ptr else None,
                                                               min_mapq, out.ctypes.data, ctypes.byref(selected),
                                                               _checks.c_flags(True, superset)), "FLAGSTATS_hip_device_u16_filter_sync")
    return out, int(selected.value)


def count_torch_filter(t, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0, out=None, selected=None, store: bool = False,
                       superset: bool = False):
    """Counters of the elements of the 1-D contiguous ``int16`` / ``uint16`` CUDA tensor ``t`` that pass the filter (``mapq``: a
    1-D contiguous ``torch.uint8`` tensor of ``t.numel()`` elements on ``t``'s device, needed when ``min_mapq > 0``) -- on
    torch's current stream, nothing synchronised.

    Returns ``(out, selected)``: ``int64[32]`` and ``int64[1]`` CUDA tensors on ``t``'s device (made zeroed when not given).
    ``store=False`` adds into both; ``store=True`` overwrites both."""
    import torch

    _checks.check_u16_tensor(t)
    _check_mapq_torch(mapq, t.numel())
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq is not None)
    _checks.check_result_pair(out, "selected", selected)
    out, selected = _checks.place_result_pair(t, out, "selected", selected, others=(("mapq", mapq),))
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(lib.FLAGSTATS_hip_device_u16_filter(t.data_ptr() if n else None, n, require, exclude,
                                                       mapq.data_ptr() if mapq is not None and n else None, min_mapq, out.data_ptr(),
                                                       selected.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_u16_filter")
    return out, selected
