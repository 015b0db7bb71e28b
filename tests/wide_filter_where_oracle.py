"""The filtered and selected flagstat of int32 / int64 columns (fsk_launch_wide_filter_where,
csrc/flagstat_wide_filter_where.hip) in numpy: what a call over a column of 4-byte or 8-byte integers, a MAPQ column and a
selection must report.

Expected values never come from the code under test: the counters are where_oracle.want_counters (oracle.flagstat_c of
``values[mask]``, superset slots from oracle.samtools_counts and the definition) of the low 16 bits of the column under
``filter_oracle.filter_mask & mask``, ``selected`` is that mask's sum, and ``high`` is the OR of ``element & ~0xFFFF`` over the
elements that ``mask`` selects, passing or not -- 0 when ``require & exclude != 0``, a pair that reads nothing."""
import numpy as np

import filter_oracle
import where_oracle
from wide_where_oracle import UNSIGNED, low16  # noqa: F401  (re-exported)


def counted_mask(values, mask, require: int, exclude: int, mapq=None, min_mapq: int = 0) -> np.ndarray:
    """bool[n]: element i passes the filter on its low 16 bits and the mask selects it"""
    return filter_oracle.filter_mask(low16(values), require, exclude, mapq, min_mapq) & np.asarray(mask, dtype=bool)


def want_high(values, mask, require: int = 0, exclude: int = 0) -> int:
    if require & exclude:
        return 0
    v = np.ascontiguousarray(values)
    u = v.view(UNSIGNED[v.dtype.itemsize])
    picked = u[np.asarray(mask, dtype=bool)]
    return int(np.bitwise_or.reduce(picked & ~u.dtype.type(0xFFFF))) if picked.size else 0


def want(oracle_mod, values, mask, require: int = 0, exclude: int = 0, mapq=None, min_mapq: int = 0, superset: bool = False):
    """(uint64[32] counters, selected, high) of ``values`` (a 4-byte or 8-byte integer array) under the filter and ``mask``"""
    both = counted_mask(values, mask, require, exclude, mapq, min_mapq)
    counters = where_oracle.want_counters(oracle_mod, low16(values), both, superset=superset)
    return counters, int(both.sum()), want_high(values, mask, require, exclude)
