"""Flagstat of the reads that pass samtools' whole view predicate on FLAG and MAPQ: ``samtools view -f require -F exclude
--rf include_any -G exclude_all -q min_mapq | samtools flagstat`` in one pass, with no mask array in memory.

``filter`` with the two options no ``require`` / ``exclude`` pair can express once they name two bits: ``include_any``
(``--rf`` / ``--incl-flags``) keeps a read only if it has at least one of these bits, ``exclude_all`` (``-G``) drops a read only
if it has all of these bits; 0 switches either off.  ``-G 0xC`` drops the pairs of which read and mate are both unmapped,
``--rf 0x50`` keeps first or reverse.  Everything else is ``filter``'s: the counters of the values that pass, ``selected``, their
number, the MAPQ column that ``min_mapq > 0`` needs.  The library reduces the four masks first: a single ``--rf`` bit is a
required bit, a single ``-G`` bit an excluded one, and such a call runs ``filter``'s kernel; only a residue of two or more free
bits runs the kernel of its own.  ``uint16`` arrays as a whole only.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .filter import _check_flag_mask, _check_mapq_numpy, _check_mapq_torch, _check_numpy, _check_predicate  # noqa: F401
from .pyflagstats import _as_dict


def _check_predicate_rf(require, exclude, include_any, exclude_all, min_mapq, has_mapq: bool):
    """``filter``'s predicate, then the two masks it lacks, which are masks like ``require``"""
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, has_mapq)
    return require, exclude, _check_flag_mask("include_any", include_any), _check_flag_mask("exclude_all", exclude_all), min_mapq


def counters_filter_rf(values, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0, mapq=None,
                       min_mapq: int = 0, superset: bool = False):
    """``(uint64[32] counters, int selected)`` of the elements of the 1-D ``uint16`` host array ``values`` that have every bit
    of ``require``, no bit of ``exclude``, at least one bit of ``include_any`` (unless 0), not all bits of ``exclude_all``
    (unless 0) and, with ``min_mapq > 0``, ``mapq[i] >= min_mapq`` (``mapq``: a ``uint8`` array of the same length)
    (``FLAGSTATS_hip_u16_x64_filter_rf``)."""
    v, q = _check_numpy(values, mapq)
    require, exclude, include_any, exclude_all, min_mapq = _check_predicate_rf(require, exclude, include_any, exclude_all, min_mapq,
                                                                               q is not None)
    out = np.zeros(32, dtype=np.uint64)
    selected = ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_u16_x64_filter_rf(v.ctypes.data if v.size else None, v.size, require, exclude, include_any,
                                                          exclude_all, q.ctypes.data if q is not None and q.size else None, min_mapq,
                                                          out.ctypes.data, ctypes.byref(selected), _checks.c_flags(True, superset)),
               "FLAGSTATS_hip_u16_x64_filter_rf")
    return out, int(selected.value)


def flagstats_filter_rf(values, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0, mapq=None,
                        min_mapq: int = 0) -> dict:
    """The dict of ``pyflagstats.flagstats_x64`` over the values that pass: ``n_values`` is their number and ``mapped`` is
    derived from it."""
    counters, selected = counters_filter_rf(values, require=require, exclude=exclude, include_any=include_any, exclude_all=exclude_all,
                                            mapq=mapq, min_mapq=min_mapq)
    return _as_dict(counters, selected)


def count_device_ptr_filter_rf(ptr: int, n: int, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0,
                               mapq_ptr: int = 0, min_mapq: int = 0, superset: bool = False):
    """``(uint64[32], int selected)`` of a device array of ``n`` ``uint16`` flags under the predicate, array and MAPQ column
    (``n`` bytes; ``mapq_ptr`` 0: none) given as raw pointers.  Synchronous (``FLAGSTATS_hip_device_u16_filter_rf_sync``)."""
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("mapq_ptr", mapq_ptr)))
    require, exclude, include_any, exclude_all, min_mapq = _check_predicate_rf(require, exclude, include_any, exclude_all, min_mapq,
                                                                               mapq_ptr != 0)
    ptr, n, mapq_ptr = int(ptr), int(n), int(mapq_ptr)
    out = np.zeros(32, dtype=np.uint64)
    selected = ctypes.c_uint64(0)
    _lib.check(_lib.lib().FLAGSTATS_hip_device_u16_filter_rf_sync(ptr if n else None, n, require, exclude, include_any, exclude_all,
                                                                  mapq_ptr if n and mapq_ptr else None, min_mapq, out.ctypes.data,
                                                                  ctypes.byref(selected), _checks.c_flags(True, superset)),
               "FLAGSTATS_hip_device_u16_filter_rf_sync")
    return out, int(selected.value)


def count_torch_filter_rf(t, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0, mapq=None, min_mapq: int = 0,
                          out=None, selected=None, store: bool = False, superset: bool = False):
    """Counters of the elements of the 1-D contiguous ``int16`` / ``uint16`` CUDA tensor ``t`` that pass the predicate (``mapq``:
    a 1-D contiguous ``torch.uint8`` tensor of ``t.numel()`` elements on ``t``'s device, needed when ``min_mapq > 0``) -- on
    torch's current stream, nothing synchronised.

    Returns ``(out, selected)``: ``int64[32]`` and ``int64[1]`` CUDA tensors on ``t``'s device (made zeroed when not given).
    ``store=False`` adds into both; ``store=True`` overwrites both."""
    import torch

    _checks.check_u16_tensor(t)
    _check_mapq_torch(mapq, t.numel())
    require, exclude, include_any, exclude_all, min_mapq = _check_predicate_rf(require, exclude, include_any, exclude_all, min_mapq,
                                                                               mapq is not None)
    _checks.check_result_pair(out, "selected", selected)
    out, selected = _checks.place_result_pair(t, out, "selected", selected, others=(("mapq", mapq),))
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(lib.FLAGSTATS_hip_device_u16_filter_rf(t.data_ptr() if n else None, n, require, exclude, include_any, exclude_all,
                                                          mapq.data_ptr() if mapq is not None and n else None, min_mapq, out.data_ptr(),
                                                          selected.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_u16_filter_rf")
    return out, selected
