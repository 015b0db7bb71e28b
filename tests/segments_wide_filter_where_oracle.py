"""The segmented flagstat of int32 / int64 columns under samtools' filter and a selection together
(csrc/flagstat_segments_wide_filter_where.hip) in numpy: what a call over a column of 4-byte or 8-byte integers, a MAPQ column, a
selection and CSR offsets must report.

Expected triples never come from the code under test.  Rows and ``selected`` are ``segments_where_oracle.want`` of the elements'
low 16 bits under ``filter_where_oracle.combined_mask`` (the elements that pass AND that the mask selects); ``high[i]`` is the OR
of ``element & ~0xFFFF`` over the elements of segment ``i`` that ``mask`` selects, passing or not -- and 0 everywhere when
``require & exclude != 0``, a pair that reads nothing.  (test_segments_wide_filter_where_host.py checks this against a
per-element, per-segment Python loop and against oracle.flagstat_c of the compacted, narrowed segment.)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filter_where_oracle  # noqa: E402
import segments_where_oracle  # noqa: E402
from wide_where_oracle import BITMAP, BYTES, UNSIGNED, low16, pack, poison  # noqa: E402,F401  (re-exported for the tests)


def counted_mask(values, mask, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0) -> np.ndarray:
    """bool[n]: element j passes the filter on its low 16 bits and the mask selects it"""
    return filter_where_oracle.combined_mask(low16(values), mask, require, exclude, mapq, min_mapq)


def want_high(values, offsets, mask, require: int = 0, exclude: int = 0) -> np.ndarray:
    """uint64[nseg]: the OR of ``element & ~0xFFFF`` over the mask-selected elements of every segment"""
    v = np.ascontiguousarray(values)
    u = v.view(UNSIGNED[v.dtype.itemsize])
    m = np.asarray(mask, dtype=bool).ravel()
    o = np.asarray(offsets, dtype=np.int64).ravel()
    high = np.zeros(max(o.size - 1, 0), dtype=np.uint64)
    if require & exclude:
        return high
    low = u.dtype.type(0xFFFF)
    for i in range(o.size - 1):
        b, e = int(o[i]), int(o[i + 1])
        if e > b:
            picked = u[b:e][m[b:e]]
            if picked.size:
                high[i] = np.uint64(np.bitwise_or.reduce(picked & ~low))
    return high


def want(values, offsets, mask, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0, superset: bool = False):
    """(uint64[nseg, 32] rows, uint64[nseg] selected, uint64[nseg] high) of ``values`` (a 4-byte or 8-byte integer array) under
    the filter and the boolean ``mask`` (one bool per ELEMENT of values), per segment"""
    v = np.ascontiguousarray(values)
    m = np.asarray(mask, dtype=bool).ravel()
    assert v.ndim == 1 and m.size == v.size
    rows, selected = segments_where_oracle.want(low16(v), offsets, counted_mask(v, m, require, exclude, mapq, min_mapq), superset)
    return rows, selected, want_high(v, offsets, m, require, exclude)
