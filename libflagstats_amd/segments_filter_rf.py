"""Filtered segmented flagstat under samtools' whole view predicate on FLAG and MAPQ: per segment of a FLAG array, the counters
of the reads that pass ``-f require -F exclude --rf include_any -G exclude_all -q min_mapq`` and how many pass -- per-contig,
per-sample or per-block tables of the reads passing ``-F 0x904 --rf 0x50 -q 30``, all segments in one launch, with no mask array
in memory.

``segments_filter`` with the two options of ``filter_rf``: ``include_any`` (``--rf`` / ``--incl-flags``) keeps a read only if it
has at least one of these bits, ``exclude_all`` (``-G``) drops a read only if it has all of these bits; 0 switches either off.
Segments are CSR offsets under the contract of ``segments``; everything else is ``segments_filter``'s: ``selected[i]``, the
number of flags of segment ``i`` that pass, the MAPQ column that ``min_mapq > 0`` needs, ``superset=True``.  The library reduces
the four masks first, as for whole columns: a predicate that passes nothing launches nothing, one that a ``require`` /
``exclude`` pair can express runs ``segments_filter``'s kernel, and only a residue of two or more free bits runs the kernel of
its own.  ``uint16`` arrays only.
"""
from __future__ import annotations

import ctypes

from . import _checks, _lib
from ._checks import STORE, SUPERSET  # noqa: F401  (kept as this module's names)
from .filter_rf import _check_predicate_rf
from .segments import check_offsets
from .segments_filter import _check_mapq_torch, _check_numpy, segment_filter_dicts  # noqa: F401  (segment_filter_dicts re-exported)


def flagstats_segments_filter_rf(values, offsets, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0,
                                 mapq=None, min_mapq: int = 0, superset: bool = False):
    """``(uint64[nseg, 32] counters, uint64[nseg] selected)`` of the segments of the 1-D ``uint16`` host array ``values`` under
    the predicate (``mapq``: a ``uint8`` array of the same length, needed when ``min_mapq > 0``)
    (``FLAGSTATS_hip_u16_x64_segments_filter_rf``)."""
    v, q = _check_numpy(values, mapq)
    require, exclude, include_any, exclude_all, min_mapq = _check_predicate_rf(require, exclude, include_any, exclude_all, min_mapq,
                                                                               q is not None)
    o = check_offsets(offsets, v.size)
    nseg = o.size - 1
    out, selected = _checks.segment_results(nseg, 1)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_u16_x64_segments_filter_rf(v.ctypes.data if v.size else None, v.size, o.ctypes.data, nseg,
                                                                       require, exclude, include_any, exclude_all,
                                                                       q.ctypes.data if q is not None and q.size else None, min_mapq,
                                                                       out.ctypes.data, selected.ctypes.data,
                                                                       _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_u16_x64_segments_filter_rf")
    return out, selected


def count_segments_device_ptr_filter_rf(ptr: int, n: int, offsets, require: int = 0, exclude: int = 0, include_any: int = 0,
                                        exclude_all: int = 0, mapq_ptr: int = 0, min_mapq: int = 0, superset: bool = False):
    """``(uint64[nseg, 32], uint64[nseg] selected)`` of the segments of a device array of ``n`` ``uint16`` flags under the
    predicate, array and MAPQ column (``n`` bytes; ``mapq_ptr`` 0: none) given as raw pointers; host offsets.  Synchronous
    (``FLAGSTATS_hip_device_u16_segments_filter_rf_sync``)."""
    _checks.check_raw_ints((("ptr", ptr), ("n", n), ("mapq_ptr", mapq_ptr)))
    require, exclude, include_any, exclude_all, min_mapq = _check_predicate_rf(require, exclude, include_any, exclude_all, min_mapq,
                                                                               mapq_ptr != 0)
    ptr, n, mapq_ptr = int(ptr), int(n), int(mapq_ptr)
    o = check_offsets(offsets, n)
    nseg = o.size - 1
    out, selected = _checks.segment_results(nseg, 1)
    if nseg:
        _lib.check(_lib.lib().FLAGSTATS_hip_device_u16_segments_filter_rf_sync(ptr if n else None, n, o.ctypes.data, nseg, require,
                                                                               exclude, include_any, exclude_all,
                                                                               mapq_ptr if n and mapq_ptr else None, min_mapq,
                                                                               out.ctypes.data, selected.ctypes.data,
                                                                               _checks.c_flags(True, superset)),
                   "FLAGSTATS_hip_device_u16_segments_filter_rf_sync")
    return out, selected


def count_segments_torch_filter_rf(t, offsets, require: int = 0, exclude: int = 0, include_any: int = 0, exclude_all: int = 0,
                                   mapq=None, min_mapq: int = 0, out=None, selected=None, store: bool = True,
                                   superset: bool = False):
    """Counters of the segments of the 1-D contiguous ``int16`` / ``uint16`` CUDA tensor ``t`` under the predicate (``mapq``: a
    1-D contiguous ``torch.uint8`` tensor of ``t.numel()`` elements on ``t``'s device, needed when ``min_mapq > 0``), on torch's
    current stream, nothing synchronised.

    ``offsets``: a 1-D contiguous ``int64`` CUDA tensor (nseg + 1 values) on the same device.  Its order is not checked here (that
    would synchronise): the kernel clamps what it reads, so bad offsets give undefined counters, never a bad access.
    Returns ``(out, selected)``: ``int64[nseg, 32]`` and ``int64[nseg]`` CUDA tensors on ``t``'s device; ``store=False`` adds into
    both (made zeroed when not given) instead of overwriting them."""
    import torch

    _checks.check_u16_tensor(t)
    nseg = _checks.check_offsets_tensor(offsets)
    _check_mapq_torch(mapq, t.numel())
    require, exclude, include_any, exclude_all, min_mapq = _check_predicate_rf(require, exclude, include_any, exclude_all, min_mapq,
                                                                               mapq is not None)
    out, selected = _checks.place_result_rows(t, nseg, store, (("out", out), ("selected", selected)),
                                            others=(("offsets", offsets), ("mapq", mapq)))
    lib = _lib.lib()
    with torch.cuda.device(t.device):
        stream = ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)
        n = t.numel()
        flags = _checks.c_flags(store, superset)
        _lib.check(lib.FLAGSTATS_hip_device_u16_segments_filter_rf(t.data_ptr() if n else None, n, offsets.data_ptr(), nseg, require,
                                                                   exclude, include_any, exclude_all,
                                                                   mapq.data_ptr() if mapq is not None and n else None, min_mapq,
                                                                   out.data_ptr(), selected.data_ptr(), flags, stream),
                   "FLAGSTATS_hip_device_u16_segments_filter_rf")
    return out, selected
