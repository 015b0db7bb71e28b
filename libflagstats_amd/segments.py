"""Segmented flagstat: one row of 32 counters per segment of a FLAG array, all segments in one launch.

Segments are given as CSR offsets: segment ``i`` is ``values[offsets[i]:offsets[i+1]]``.  Offsets are non-decreasing with
``offsets[-1] <= len(values)``; flags before ``offsets[0]`` or after ``offsets[-1]`` are ignored and empty segments are
allowed.  Every row follows the slot contract of the other entry points (``include/libflagstats_hip.h``); with
``superset=True`` slots 0 / 16 (primary paired reads) and slot 9 (the segment's length minus its slot 25) are filled too.

Typical callers: per-block counters of a column-store FLAG column (blocks of 512,000 records), per-contig counters of a
coordinate-sorted column, per-sample counters of a batch of reads held in one torch tensor.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .pyflagstats import _as_dict


def offsets_from_lengths(lengths) -> np.ndarray:
    """CSR offsets (``uint64[nseg + 1]``, starting at 0) of consecutive segments of the given lengths."""
    n = np.asarray(lengths)
    if n.ndim != 1:
        raise ValueError("lengths must be 1-D")
    if n.size and (n.dtype.kind not in "iu" or (n.dtype.kind == "i" and (n < 0).any())):
        raise ValueError("lengths must be non-negative integers")
    out = np.zeros(n.size + 1, dtype=np.uint64)
    np.cumsum(n.astype(np.uint64), out=out[1:])
    return out


def check_offsets(offsets, n: int) -> np.ndarray:
    """Validate host offsets for an array of ``n`` flags; returns them as a contiguous ``uint64`` array.  ``ValueError`` if
    they are not 1-D integers, hold fewer than one value, decrease, are negative or end beyond ``n``."""
    o = np.asarray(offsets)
    if o.ndim != 1:
        raise ValueError("offsets must be 1-D (nseg + 1 values)")
    if o.size == 0:
        raise ValueError("offsets must hold nseg + 1 >= 1 values")
    if o.dtype.kind not in "iu":
        raise ValueError("offsets must have an integer dtype, not %s" % o.dtype)
    if o.dtype.kind == "i" and int(o.min()) < 0:
        raise ValueError("offsets must not be negative")
    o = np.ascontiguousarray(o, dtype=np.uint64)
    if o.size > 1 and (o[1:] < o[:-1]).any():
        i = int(np.argmax(o[1:] < o[:-1]))
        raise ValueError("offsets must be non-decreasing: offsets[%d] = %d > offsets[%d] = %d" % (i, o[i], i + 1, o[i + 1]))
    if int(o[-1]) > n:
        raise ValueError("offsets[-1] = %d exceeds the array's %d flags" % (int(o[-1]), n))
    return o


def flagstats_segments(values, offsets, superset: bool = False) -> np.ndarray:
    """``uint64[nseg, 32]`` counters of every segment of a host ``uint16`` array (``FLAGSTATS_hip_u16_x64_segments``)."""
    v = np.asarray(values)
    if v.ndim != 1 or v.dtype != np.uint16:
        raise ValueError("values must be a 1-D uint16 array")
    o = check_offsets(offsets, v.size)
    v = np.ascontiguousarray(v)
    nseg = o.size - 1
    out = np.zeros((nseg, 32), dtype=np.uint64)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_u16_x64_segments(v.ctypes.data if v.size else None, v.size, o.ctypes.data, nseg,
                                                             out.ctypes.data, _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_u16_x64_segments")
    return out


def count_segments_device_ptr(ptr: int, n: int, offsets, superset: bool = False) -> np.ndarray:
    """``uint64[nseg, 32]`` counters of the segments of a device ``uint16`` array given as a raw pointer (e.g.
    ``DeviceFlags.ptr``); host offsets; synchronous (``FLAGSTATS_hip_device_u16_segments_sync``)."""
    o = check_offsets(offsets, n)
    nseg = o.size - 1
    out = np.zeros((nseg, 32), dtype=np.uint64)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_device_u16_segments_sync(ptr, n, o.ctypes.data, nseg, out.ctypes.data,
                                                                     _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_device_u16_segments_sync")
    return out


def count_segments_torch(t, offsets, out=None, store: bool = True, superset: bool = False):
    """Counters of the segments of a contiguous 16-bit CUDA tensor, on torch's current stream, nothing synchronised.

    ``offsets``: a 1-D contiguous ``int64`` CUDA tensor (nseg + 1 values) on the same device.  Its order is not checked here
    (that would synchronise): the kernel clamps what it reads, so bad offsets give undefined counters, never a bad access.
    Returns (or fills) an ``int64[nseg, 32]`` CUDA tensor; ``store=False`` adds into ``out`` instead of overwriting it."""
    import torch

    if not (t.is_cuda and t.is_contiguous() and t.element_size() == 2):
        raise ValueError("need a contiguous 16-bit CUDA tensor")
    if not (offsets.is_cuda and offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.is_contiguous()
            and offsets.numel() >= 1 and offsets.device == t.device):
        raise ValueError("offsets must be a 1-D contiguous int64 CUDA tensor (nseg + 1 values) on the array's device")
    nseg = offsets.numel() - 1
    if out is None:
        out = (torch.empty if store else torch.zeros)((nseg, 32), dtype=torch.int64, device=t.device)
    if not (out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == (nseg, 32)
            and out.device == t.device):
        raise ValueError("out must be a contiguous int64 CUDA tensor of shape (nseg, 32) on the array's device")
    stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
    flags = _checks.c_flags(store, superset)
    _lib.check(_lib.lib().FLAGSTATS_hip_device_u16_segments(t.data_ptr() if t.numel() else None, t.numel(), offsets.data_ptr(),
                                                            nseg, out.data_ptr(), flags, stream),
               "FLAGSTATS_hip_device_u16_segments")
    return out


def segment_dicts(counters, offsets) -> list:
    """One ``pyflagstats.flagstats``-shaped dict per counter row, each with its segment's length as ``n_values``."""
    c = np.asarray(counters)
    o = np.asarray(offsets, dtype=np.int64).ravel()
    if c.ndim != 2 or c.shape[1] != 32 or o.size != c.shape[0] + 1:
        raise ValueError("counters must be [nseg, 32] with nseg + 1 offsets")
    return [_as_dict(c[i], int(o[i + 1] - o[i])) for i in range(c.shape[0])]
