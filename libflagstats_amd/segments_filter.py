"""Filtered segmented flagstat: per segment of a FLAG array, the counters of the reads that pass samtools' view filter
(``-f require -F exclude -q min_mapq``) and how many pass -- per-contig, per-sample or per-block tables of the reads passing
``-F 0x904 -q 30``, all segments in one launch, with no mask array and no zeroed copy of the column in memory.

Segments are CSR offsets under the contract of ``segments`` (segment ``i`` is ``values[offsets[i]:offsets[i+1]]``; flags outside
every segment count nowhere; empty segments are allowed); the predicate is that of ``filter`` (``require & exclude != 0`` is legal
and passes nothing; ``min_mapq == 0`` reads no MAPQ).  Next to every row of 32 counters the caller gets ``selected[i]``, the number
of flags of segment ``i`` that pass; with ``superset=True`` slots 0 / 16 are the primary paired reads among them and slot 9 is
``selected[i]`` minus slot 25.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .filter import _check_mapq_torch, _check_numpy, _check_predicate
from .pyflagstats import _as_dict
from .segments import check_offsets


def flagstats_segments_filter(values, offsets, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0,
                              superset: bool = False):
    """``(uint64[nseg, 32] counters, uint64[nseg] selected)`` of the segments of the 1-D ``uint16`` host array ``values`` under
    the filter (``mapq``: a ``uint8`` array of the same length, needed when ``min_mapq > 0``)
    (``FLAGSTATS_hip_u16_x64_segments_filter``)."""
    v, q = _check_numpy(values, mapq)
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, q is not None)
    o = check_offsets(offsets, v.size)
    nseg = o.size - 1
    out, selected = _checks.segment_results(nseg, 1)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_u16_x64_segments_filter(v.ctypes.data if v.size else None, v.size, o.ctypes.data, nseg,
                                                                    require, exclude,
                                                                    q.ctypes.data if q is not None and q.size else None, min_mapq,
                                                                    out.ctypes.data, selected.ctypes.data,
                                                                    _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_u16_x64_segments_filter")
    return out, selected


def count_segments_device_ptr_filter(ptr: int, n: int, offsets, require: int = 0, exclude: int = 0, mapq_ptr: int = 0,
                                     min_mapq: int = 0, superset: bool = False):
    """``(uint64[nseg, 32], uint64[nseg] selected)`` of the segments of a device array of ``n`` ``uint16`` flags under the filter,
    array and MAPQ column (``n`` bytes; ``mapq_ptr`` 0: none) given as raw pointers; host offsets.  Synchronous
    (``FLAGSTATS_hip_device_u16_segments_filter_sync``)."""
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("mapq_ptr", mapq_ptr)))
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq_ptr != 0)
    ptr, n, mapq_ptr = int(ptr), int(n), int(mapq_ptr)
    o = check_offsets(offsets, n)
    nseg = o.size - 1
    out, selected = _checks.segment_results(nseg, 1)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_device_u16_segments_filter_sync(ptr if n else None, n, o.ctypes.data, nseg, require, exclude,
                                                                            mapq_ptr if n and mapq_ptr else None, min_mapq,
                                                                            out.ctypes.data, selected.ctypes.data,
                                                                            _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_device_u16_segments_filter_sync")
    return out, selected


def count_segments_torch_filter(t, offsets, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0, out=None, selected=None,
                                store: bool = True, superset: bool = False):
    """Counters of the segments of the 1-D contiguous ``int16`` / ``uint16`` CUDA tensor ``t`` under the filter (``mapq``: a 1-D
    contiguous ``torch.uint8`` tensor of ``t.numel()`` elements on ``t``'s device, needed when ``min_mapq > 0``), on torch's
    current stream, nothing synchronised.

    ``offsets``: a 1-D contiguous ``int64`` CUDA tensor (nseg + 1 values) on the same device.  Its order is not checked here (that
    would synchronise): the kernel clamps what it reads, so bad offsets give undefined counters, never a bad access.
    Returns ``(out, selected)``: ``int64[nseg, 32]`` and ``int64[nseg]`` CUDA tensors on ``t``'s device; ``store=False`` adds into
    both (made zeroed when not given) instead of overwriting them."""
    import torch

    _checks.check_u16_tensor(t)
    nseg = _checks.check_offsets_tensor(offsets)
    _check_mapq_torch(mapq, t.numel())
    require, exclude, min_mapq = _check_predicate(require, exclude, min_mapq, mapq is not None)
    out, selected = _checks.place_result_rows(t, nseg, store, (("out", out), ("selected", selected)),
                                            others=(("offsets", offsets), ("mapq", mapq)))
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(lib.FLAGSTATS_hip_device_u16_segments_filter(t.data_ptr() if n else None, n, offsets.data_ptr(), nseg, require, exclude,
                                                                mapq.data_ptr() if mapq is not None and n else None, min_mapq,
                                                                out.data_ptr(), selected.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_u16_segments_filter")
    return out, selected


def segment_filter_dicts(counters, selected) -> list:
    """One ``pyflagstats.flagstats``-shaped dict per counter row, each with the number of its segment's flags that pass as
    ``n_values`` (``mapped`` is derived from it)."""
    c = np.asarray(counters)
    s = np.asarray(selected).ravel()
    if c.ndim != 2 or c.shape[1] != 32 or s.size != c.shape[0]:
        raise ValueError("counters must be [nseg, 32] with nseg selected counts")
    return [_as_dict(c[i], int(s[i])) for i in range(c.shape[0])]
