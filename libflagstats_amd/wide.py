"""Flagstat of a FLAG column in the integer dtype it arrives in: ``int32`` / ``int64`` (numpy's default integer, a pandas or
Arrow column, torch's natural integer tensors) as well as 16-bit, with no ``astype(np.uint16)`` copy in front.

The low 16 bits of every element are counted exactly as ``pyflagstats.flagstats`` counts a ``uint16``; next to the 32 counters
the caller gets ``high``: the OR over all elements of ``element & ~0xFFFF`` (as unsigned).  ``high == 0`` means every element
was a valid 16-bit FLAG; a negative element sets bit 31 (4-byte elements) or bit 63 (8-byte); anything else names a value of
65,536 or more -- a wrong column, a parse error -- that a silent ``astype`` would have turned into plausible counters.
``pyflagstats.flagstats`` and ``flagstats_x64`` keep the reference's contract (``uint16`` only).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .pyflagstats import _as_dict

INT_DTYPES = ("int16", "uint16", "int32", "uint32", "int64", "uint64")


def _check_values(values) -> np.ndarray:
    if not isinstance(values, np.ndarray):
        raise ValueError("values must be a numpy.ndarray, not %s" % type(values).__name__)
    if values.dtype.name not in INT_DTYPES:
        raise ValueError("values must have an integer dtype of 2, 4 or 8 bytes (%s), not %s" % (", ".join(INT_DTYPES), values.dtype))
    if not values.dtype.isnative:
        raise ValueError("values must be in native (little-endian) byte order")
    if values.ndim != 1:
        raise ValueError("values must be 1-D, not %d-D" % values.ndim)
    return np.ascontiguousarray(values)


def _check_tensor(t) -> None:
    """``t`` is a 1-D contiguous integer tensor of 2-, 4- or 8-byte elements (where it lives is place_result_pair's business)"""
    import torch

    if not isinstance(t, torch.Tensor):
        raise ValueError("t must be a torch.Tensor, not %s" % type(t).__name__)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool or t.element_size() not in (2, 4, 8):
        raise ValueError("t must have an integer dtype of 2, 4 or 8 bytes, not %s" % t.dtype)
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError("t must be 1-D and contiguous")


def high_bits_message(high: int) -> str:
    return "values outside 0..65535: bits 0x%X set above bit 15" % high


def counters_ints(values, superset: bool = False):
    """``(uint64[32] counters, int high)`` of a 1-D host array of dtype int16, uint16, int32, uint32, int64 or uint64.
    16-bit input goes to ``FLAGSTATS_u16_x64`` (``high`` = 0), wider input to ``FLAGSTATS_hip_wide_x64``."""
    v = _check_values(values)
    out = np.zeros(32, dtype=np.uint64)
    lib = _lib.lib()
    if v.dtype.itemsize == 2:
        name = "FLAGSTATS_u16_x64_superset" if superset else "FLAGSTATS_u16_x64"
        _lib.check(getattr(lib, name)(v.ctypes.data, v.size, out.ctypes.data), name)
        return out, 0
    high = ctypes.c_uint64(0)
    _lib.check(lib.FLAGSTATS_hip_wide_x64(v.ctypes.data if v.size else None, v.size, v.dtype.itemsize, out.ctypes.data,
                                          ctypes.byref(high), _checks.c_flags(True, superset)), "FLAGSTATS_hip_wide_x64")
    return out, int(high.value)


def flagstats_ints(values, strict: bool = True) -> dict:
    """The dict of ``pyflagstats.flagstats_x64`` for an integer array of any of the six dtypes.  ``strict`` (default): a value
    outside 0..65535 raises ``ValueError`` naming the bits seen above bit 15; ``strict=False``: the dict of the truncated values
    with the mask as an extra key ``"high_bits"``."""
    counters, high = counters_ints(values)
    return _checks.with_high_bits(strict, high, lambda: high_bits_message(high), lambda: _as_dict(counters, len(values)))


def count_device_ptr_ints(ptr: int, n: int, elem_bytes: int, superset: bool = False):
    """``(uint64[32], int high)`` of a device array of ``n`` 4-byte or 8-byte integers given as a raw pointer; synchronous
    (``FLAGSTATS_hip_device_wide_sync``)."""
    _checks.check_elem_bytes(elem_bytes, "device.count_device_ptr")
    if n < 0:
        raise ValueError("n must not be negative")
    out = np.zeros(32, dtype=np.uint64)
    high = ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_device_wide_sync(ptr if n else None, n, elem_bytes, out.ctypes.data, ctypes.byref(high),
                                                         _checks.c_flags(True, superset)), "FLAGSTATS_hip_device_wide_sync")
    return out, int(high.value)


def count_torch_ints(t, out=None, high=None, store: bool = False, superset: bool = False):
    """Counters and high-bit mask of a 1-D contiguous integer CUDA tensor of 2-, 4- or 8-byte elements, on torch's current
    stream, nothing synchronised.

    Returns ``(out, high)``: ``int64[32]`` and ``int64[1]`` CUDA tensors on ``t``'s device (made zeroed when not given).
    ``store=False`` adds into ``out`` and ORs into ``high``; ``store=True`` overwrites both.  A 2-byte tensor goes to the
    ``uint16`` entries and cannot carry high bits: ``high`` is left as it is (zeroed with ``store``).  ``int(high)`` reads the
    mask as a signed 64-bit number: compare with 0, or take ``int(high) & (2**64 - 1)``."""
    import torch

    _check_tensor(t)
    _checks.check_result_pair(out, "high", high)
    out, high = _checks.place_result_pair(t, out, "high", high)
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        ptr = t.data_ptr() if t.numel() else None
        if t.element_size() == 2:
            if store:
                high.zero_()
            if store and (superset or not t.numel()):
                out.zero_()
            if not t.numel():
                return out, high
            name = ("FLAGSTATS_hip_device_u16_superset" if superset else
                    "FLAGSTATS_hip_device_u16_store" if store else "FLAGSTATS_hip_device_u16")
            _lib.check(getattr(lib, name)(ptr, t.numel(), out.data_ptr(), stream), name)
        else:
            flags = _checks.c_flags(store, superset)
            _lib.check(lib.FLAGSTATS_hip_device_wide(ptr, t.numel(), t.element_size(), out.data_ptr(), high.data_ptr(), flags, stream),
                       "FLAGSTATS_hip_device_wide")
    return out, high
